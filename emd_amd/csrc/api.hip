// api.hip -- the C ABI of include/emd_raster.h: argument checking, workspace carving, stage sequencing.
// No device memory is allocated or freed here; errors are returned as codes + a thread-local message.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "det_backward.h"

static thread_local char g_err[512] = "";

void emd_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- profiling ------------------------------------------------------------------------------------------------
#include <mutex>
#include <vector>
namespace {
struct ProfRec { int stage; hipEvent_t a, b; bool b_shared; };
bool g_prof_on = false;
std::mutex g_prof_mu;
std::vector<ProfRec> g_prof_recs;
std::vector<hipEvent_t> g_prof_pool;
hipEvent_t g_prof_open[EMD_PROF_STAGES];
const char* kStageNames[EMD_PROF_STAGES] = {"preprocess", "scan_duplicate", "radix_sort", "tile_ranges", "render_forward",
                                            "render_backward", "preprocess_backward", "other"};
hipEvent_t prof_event() {
    if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}
}  // namespace

void emd_prof_begin(int stage, hipStream_t st) {
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    hipEvent_t e = prof_event();
    if (!e) return;
    (void)hipEventRecord(e, st);
    g_prof_open[stage] = e;
}

void emd_prof_end(int stage, hipStream_t st) {
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof_open[stage]) return;
    hipEvent_t e = prof_event();
    if (!e) return;
    (void)hipEventRecord(e, st);
    g_prof_recs.push_back({stage, g_prof_open[stage], e, false});
    g_prof_open[stage] = nullptr;
}

void emd_prof_switch(int ended, int started, hipStream_t st) {
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    hipEvent_t e = prof_event();
    if (!e) return;
    (void)hipEventRecord(e, st);
    if (g_prof_open[ended]) { g_prof_recs.push_back({ended, g_prof_open[ended], e, true}); g_prof_open[ended] = nullptr; }
    g_prof_open[started] = e;
}

namespace {
__global__ void __launch_bounds__(EMD_BLOCK) k_zero_words(uint32_t* __restrict__ p, size_t head, size_t quads, size_t words) {
    // [0, head) single words up to 16-byte alignment, then `quads` uint4 stores, then the tail words
    const size_t i = (size_t)blockIdx.x * EMD_BLOCK + threadIdx.x, stride = (size_t)gridDim.x * EMD_BLOCK;
    if (i < head) p[i] = 0u;
    uint4* q = (uint4*)(p + head);
    for (size_t k = i; k < quads; k += stride) q[k] = make_uint4(0u, 0u, 0u, 0u);
    const size_t tail0 = head + quads * 4;
    if (tail0 + i < words && i < 4) p[tail0 + i] = 0u;
}
}  // namespace

// Per-step inputs of a replayed training step, selected on the device in one launch (see EmdStepSelect in emd_raster.h): what a
// host-driven loop does with a handful of tiny copies and index ops per step (camera upload, frame number, frame time, the
// coarse-to-fine level of the step) when the whole step is one hipGraph whose inputs must live at fixed device addresses.
__global__ void __launch_bounds__(EMD_WAVE) k_select_step_inputs(EmdStepSelect a) {
    const long long row = a.sel[0];
    const int lane = threadIdx.x;
    if (a.status_log && a.status && a.prev_sel) {            // the status words of the step before (its forward is long done): logged by row
        const long long prev = a.prev_sel[0];
        if (prev >= 0 && prev < a.rows && lane < 4) a.status_log[4 * prev + lane] = a.status[lane];
    }
    if (row < 0 || row >= a.rows) {                          // flush-only call (sel = -1 after the last step)
        if (a.prev_sel && lane == 0) a.prev_sel[0] = -1;
        return;
    }
    for (int j = lane; j < a.row_floats; j += EMD_WAVE) a.out_row[j] = a.table[(size_t)row * a.row_floats + j];
    if (lane == 0) {
        if (a.prev_sel) a.prev_sel[0] = row;
        if (a.next_sel) a.sel[0] = a.next_sel[row];           // the row of the NEXT launch: a replay loop then needs no host-side write at all
        if (a.frames && a.frame_out) {
            const int f = a.frames[row];
            a.frame_out[0] = f;
            if (a.t_out) a.t_out[0] = (float)f / (float)(a.num_frames > 1 ? a.num_frames - 1 : 1);
        }
        if (a.k_fine_out) {
            // int_lininterp(step, k_min, k_max, until) of rigid.py:147-148,194-201, with the reference's float division + truncation
            long long step = a.steps ? a.steps[row] : row;
            step = step < 0 ? 0 : (step > a.k_until ? a.k_until : step);
            a.k_fine_out[0] = (int)((double)a.k_min + (double)(a.k_max - a.k_min) * (double)step / (double)a.k_until);
        }
    }
}

int emd_zero_async(void* p, size_t bytes, hipStream_t st) {
    if (!p || bytes == 0) return EMD_OK;
    if (((uintptr_t)p & 3) || (bytes & 3)) { emd_set_error("emd_zero_async: pointer / size not a multiple of 4 bytes"); return EMD_ERR_INVALID; }
    const size_t words = bytes / 4;
    size_t head = ((16 - ((uintptr_t)p & 15)) & 15) / 4;
    if (head > words) head = words;
    const size_t quads = (words - head) / 4;
    size_t blocks = (quads + EMD_BLOCK - 1) / EMD_BLOCK;
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_zero_words, dim3((unsigned)blocks), dim3(EMD_BLOCK), 0, st, (uint32_t*)p, head, quads, words);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

// debug mode (EmdSettings.debug): a stage's faults are reported under its name
static int stage_sync(bool dbg, hipStream_t st, const char* name) {
    if (!dbg) return EMD_OK;
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) { emd_set_error("stage %s failed: %s", name, hipGetErrorString(e)); return EMD_ERR_HIP; }
    return EMD_OK;
}

// The inputs PreArgs (K1) and PreBwdArgs (K8, the camera gradient) share, from the public arguments; the motion block only under EMD_FLAG_MOTION.
template <class P, class A> static void fill_inputs(P& p, const A& a, const GeomWs& g) {
    p.s = a.s; p.N = a.num_gaussians; p.M = a.sh_coeffs; p.flags = a.flags;
    p.means3D = a.means3D; p.shs = a.shs; p.colors_precomp = a.colors_precomp; p.opacities = a.opacities;
    p.scales = a.scales; p.rotations = a.rotations; p.cov3D_precomp = a.cov3D_precomp;
    if (a.flags & EMD_FLAG_MOTION) p.motion = a.motion; else memset(&p.motion, 0, sizeof(p.motion));
    p.radii = a.radii; p.g = g; p.sdev = a.settings_dev;
}
static void fill_bwd_inputs(PreBwdArgs& p, const EmdBwdArgs& a, const GeomWs& g) {
    fill_inputs(p, a, g);
    p.grad_rec = (float*)a.bwd_ws; p.bwd_stride = emd_bwd_stride(a.num_extra); p.num_extra = a.num_extra;
    p.shs_prezeroed = 0;
}

// What both backward entries need of the forward's state, behind check_common: the pointers, num_extra, the device settings, the sizes of geom_ws and bwd_ws
// (`rest_fits`: the entry's other workspaces are large enough -- one EMD_ERR_WORKSPACE for all of them), the alignment of the accumulator rows.  Carves g.
static int check_bwd_state(const EmdBwdArgs* a, const char* who, GeomWs* g, bool rest_fits) {
    if (!a->radii || !a->geom_ws || !a->bin_ws || !a->img_ws || !a->bwd_ws || !a->status || !a->out_color || !a->out_depth) {
        emd_set_error("%s: null state pointer", who); return EMD_ERR_INVALID;
    }
    if (a->num_extra < 0 || a->num_extra > EMD_MAX_EXTRA) { emd_set_error("%s: num_extra %d not in 0..%d", who, a->num_extra, EMD_MAX_EXTRA); return EMD_ERR_INVALID; }
    if ((a->flags & EMD_FLAG_SDEV_TANFOV) && !a->settings_dev) { emd_set_error("%s: EMD_FLAG_SDEV_TANFOV without settings_dev", who); return EMD_ERR_INVALID; }
    emd_carve_geom((void*)a->geom_ws, a->num_gaussians, g);
    const size_t need = emd_bwd_bytes(a->num_gaussians, a->num_extra);
    if (g->bytes > a->geom_bytes || need > a->bwd_bytes || !rest_fits) {
        emd_set_error("%s: workspace too small (geom %zu/%zu bwd %zu/%zu%s)", who, a->geom_bytes, g->bytes, a->bwd_bytes, need, rest_fits ? "" : "; another workspace of the call is short");
        return EMD_ERR_WORKSPACE;
    }
    if ((uintptr_t)a->bwd_ws & 63) { emd_set_error("%s: bwd_ws must be 64-byte aligned (an accumulator row is one 64-byte line)", who); return EMD_ERR_INVALID; }
    return EMD_OK;
}

extern "C" {

int emd_abi_version(void) { return EMD_ABI_VERSION; }

int emd_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
    return EMD_OK;
}

const char* emd_profile_stage_name(int stage) { return (stage >= 0 && stage < EMD_PROF_STAGES) ? kStageNames[stage] : ""; }

int emd_profile_read(double* ms, int64_t* count, int max_stages) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof_recs) {
        float t = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess && r.stage < max_stages) {
            if (ms) ms[r.stage] += (double)t;
            if (count) count[r.stage] += 1;
        }
        g_prof_pool.push_back(r.a);                 // a shared end event is the next record's `a`: pooled there
        if (!r.b_shared) g_prof_pool.push_back(r.b);
    }
    g_prof_recs.clear();
    return EMD_PROF_STAGES;
}

const char* emd_last_error(void) { return g_err; }

int emd_raster_workspace_size(const EmdDims* dims, size_t out[4]) {
    if (!dims || !out) { emd_set_error("workspace_size: null argument"); return EMD_ERR_INVALID; }
    if (dims->num_gaussians < 0 || dims->image_height <= 0 || dims->image_width <= 0 || dims->bin_capacity < 0) {
        emd_set_error("workspace_size: bad dims N=%d H=%d W=%d cap=%lld", dims->num_gaussians, dims->image_height,
                      dims->image_width, (long long)dims->bin_capacity);
        return EMD_ERR_INVALID;
    }
    GeomWs g; BinWs b; ImgWs im;
    const int gx = (dims->image_width + EMD_TILE_X - 1) / EMD_TILE_X, gy = (dims->image_height + EMD_TILE_Y - 1) / EMD_TILE_Y;
    emd_carve_geom(nullptr, dims->num_gaussians, &g);
    emd_carve_bin(nullptr, dims->bin_capacity, gx * gy, &b);
    emd_carve_img(nullptr, dims->image_height, dims->image_width, &im);
    out[0] = g.bytes; out[1] = b.bytes; out[2] = im.bytes;
    if (dims->num_extra < 0 || dims->num_extra > EMD_MAX_EXTRA) { emd_set_error("workspace_size: num_extra %d not in 0..%d", dims->num_extra, EMD_MAX_EXTRA); return EMD_ERR_INVALID; }
    out[3] = emd_bwd_bytes(dims->num_gaussians, dims->num_extra);
    return EMD_OK;
}

static int check_common(const EmdSettings& s, int N, int M, const float* means3D, const float* shs,
                        const float* colors, const float* opac, const float* scales, const float* rots,
                        const float* cov, int flags, const EmdMotion& mo) {
    if (N < 0 || s.image_height <= 0 || s.image_width <= 0) { emd_set_error("bad sizes N=%d H=%d W=%d", N, s.image_height, s.image_width); return EMD_ERR_INVALID; }
    if (N > 0 && (!means3D || !opac)) { emd_set_error("means3D / opacities must not be null"); return EMD_ERR_INVALID; }
    if ((shs != nullptr) == (colors != nullptr) && N > 0) { emd_set_error("provide exactly one of shs / colors_precomp"); return EMD_ERR_INVALID; }
    const bool sr = scales && rots;
    if (((scales != nullptr) != (rots != nullptr)) || (sr == (cov != nullptr) && N > 0)) {
        emd_set_error("provide exactly one of (scales, rotations) / cov3D_precomp"); return EMD_ERR_INVALID;
    }
    if (s.sh_degree < 0 || s.sh_degree > 3) { emd_set_error("sh_degree %d not in 0..3", s.sh_degree); return EMD_ERR_INVALID; }
    if (shs && M < (s.sh_degree + 1) * (s.sh_degree + 1)) { emd_set_error("shs holds %d coefficients, degree %d needs %d", M, s.sh_degree, (s.sh_degree + 1) * (s.sh_degree + 1)); return EMD_ERR_INVALID; }
    if (!(flags & EMD_FLAG_SDEV_TANFOV) && (!(s.tanfovx > 0.f) || !(s.tanfovy > 0.f))) { emd_set_error("tanfov must be positive"); return EMD_ERR_INVALID; }
    if (flags & EMD_FLAG_MOTION) {
        if (mo.actor_id && (!mo.actor_pose || mo.num_actors <= 0)) { emd_set_error("motion: actor_id given without actor_pose"); return EMD_ERR_INVALID; }
        if (cov) { emd_set_error("motion: cov3D_precomp cannot be combined with the fused motion transform"); return EMD_ERR_INVALID; }
    }
    if ((flags & EMD_FLAG_RAW_PARAMS) && cov) { emd_set_error("raw params: cov3D_precomp has no raw form"); return EMD_ERR_INVALID; }
    return EMD_OK;
}

int emd_raster_forward(EmdFwdArgs* a, void* hip_stream) {
    if (!a) { emd_set_error("forward: null args"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    const int N = a->num_gaussians;
    int rc = check_common(a->s, N, a->sh_coeffs, a->means3D, a->shs, a->colors_precomp, a->opacities, a->scales,
                          a->rotations, a->cov3D_precomp, a->flags, a->motion);
    if (rc) return rc;
    if (!a->out_color || !a->out_depth || !a->out_alpha || !a->radii || !a->status || !a->geom_ws || !a->bin_ws || !a->img_ws) {
        emd_set_error("forward: null output / workspace pointer"); return EMD_ERR_INVALID;
    }
    if ((a->flags & EMD_FLAG_NORMAL) && !a->out_normal) { emd_set_error("forward: EMD_FLAG_NORMAL without out_normal"); return EMD_ERR_INVALID; }
    if (a->bin_capacity < 0) { emd_set_error("forward: negative bin_capacity"); return EMD_ERR_INVALID; }
    if ((int64_t)N >= (int64_t)1 << 28) { emd_set_error("forward: %d Gaussians; a list word holds a 28-bit Gaussian id beside the pair's quadrant mask", N); return EMD_ERR_INVALID; }
    if (a->num_extra < 0 || a->num_extra > EMD_MAX_EXTRA) { emd_set_error("forward: num_extra %d not in 0..%d", a->num_extra, EMD_MAX_EXTRA); return EMD_ERR_INVALID; }
    for (int k = 0; k < a->num_extra; k++)
        if (!a->colors_extra[k] || !a->out_extra[k]) { emd_set_error("forward: extra colour set %d: null colours / output", k); return EMD_ERR_INVALID; }
    if ((a->flags & EMD_FLAG_SDEV_TANFOV) && !a->settings_dev) { emd_set_error("forward: EMD_FLAG_SDEV_TANFOV without settings_dev"); return EMD_ERR_INVALID; }
    const int gx = (a->s.image_width + EMD_TILE_X - 1) / EMD_TILE_X, gy = (a->s.image_height + EMD_TILE_Y - 1) / EMD_TILE_Y;
    GeomWs g; BinWs b; ImgWs im;
    emd_carve_geom(a->geom_ws, N, &g);
    emd_carve_bin(a->bin_ws, a->bin_capacity, gx * gy, &b);
    emd_carve_img(a->img_ws, a->s.image_height, a->s.image_width, &im);
    if (g.bytes > a->geom_bytes || b.bytes > a->bin_bytes || im.bytes > a->img_bytes) {
        emd_set_error("forward: workspace too small (geom %zu/%zu bin %zu/%zu img %zu/%zu)", a->geom_bytes, g.bytes,
                      a->bin_bytes, b.bytes, a->img_bytes, im.bytes);
        return EMD_ERR_WORKSPACE;
    }
    const bool dbg = a->s.debug != 0;
    PreArgs pa;   // (the status word is written by the binning stage)
    fill_inputs(pa, *a, g);
    pa.status = a->status;
    pa.shs_res0 = a->shs_residual[0]; pa.shs_res1 = a->shs_residual[1];
    if ((pa.shs_res0 || pa.shs_res1) && !a->shs) { emd_set_error("raster_forward: shs_residual needs shs"); return EMD_ERR_INVALID; }
    if (pa.shs_res1 && !pa.shs_res0) { pa.shs_res0 = pa.shs_res1; pa.shs_res1 = nullptr; }
    emd_prof_begin(PROF_PREPROCESS, st);
    // With an auxiliary stream the colour half of K1 (SH colour, clamp bits, colour Jacobian: needed by K6 only) runs BESIDE the binning
    // stage: fork after the geometry half, join in front of K6.  (Measured in round 3 and OFF by default in the binding: the halves cost
    // 0.075 + 0.122 ms apart against 0.159 ms fused, and beside the colour half's 31 250 workgroups the binning kernels wait for slots:
    // 684 against 700 it/s.  Kept as an option for callers whose binning is longer.)  Both edges are events, so a capturing stream records them as graph
    // dependencies.  Every return between fork and join joins first: the caller may free or reuse the workspaces on an error.
    hipStream_t aux = (hipStream_t)a->aux_stream;
    const bool split = aux != nullptr && aux != st && N > 0 && !dbg;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    auto join = [&]() -> int {
        if (!ev_join) return EMD_OK;
        hipError_t e1 = hipStreamWaitEvent(st, ev_join, 0);
        (void)hipEventDestroy(ev_fork); (void)hipEventDestroy(ev_join);
        ev_fork = ev_join = nullptr;
        if (e1 != hipSuccess) { emd_set_error("forward: joining the auxiliary stream failed: %s", hipGetErrorString(e1)); return EMD_ERR_HIP; }
        return EMD_OK;
    };
    rc = emd_launch_preprocess(pa, split ? 1 : 0, st);
    if (rc) return rc;
    if (split) {
        EMD_HIP_CHECK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        EMD_HIP_CHECK(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
        EMD_HIP_CHECK(hipEventRecord(ev_fork, st));
        EMD_HIP_CHECK(hipStreamWaitEvent(aux, ev_fork, 0));
        rc = emd_launch_preprocess(pa, 2, aux);
        hipError_t e2 = hipEventRecord(ev_join, aux);
        if (rc || e2 != hipSuccess) { (void)join(); if (!rc) { emd_set_error("forward: hipEventRecord on the auxiliary stream failed"); rc = EMD_ERR_HIP; } return rc; }
    }
    if ((rc = stage_sync(dbg, st, "preprocess"))) return rc;
    rc = emd_launch_binning(a->s, a->flags, N, g, b, a->bin_capacity, a->status, st);
    if (rc) { (void)join(); return rc; }
    if ((rc = stage_sync(dbg, st, "binning"))) return rc;
    a->num_rendered = -1;
    a->num_visible = -1;
    if (!(a->flags & EMD_FLAG_NO_SYNC)) {
        EmdStatus hs;
        EMD_HIP_CHECK(hipMemcpyAsync(&hs, a->status, sizeof(hs), hipMemcpyDeviceToHost, st));
        EMD_HIP_CHECK(hipStreamSynchronize(st));
        a->num_rendered = hs.num_rendered;
        a->num_visible = hs.num_visible;
        if (hs.overflow & 2u) {
            (void)join();
            emd_set_error("forward: a visible Gaussian lies beyond 65 536 x the near plane; repeat with EMD_FLAG_WIDE_DEPTH_SORT");
            return EMD_ERR_DEPTH_RANGE;
        }
        if (hs.overflow) {
            (void)join();
            emd_set_error("forward: %u (tile, Gaussian) pairs exceed bin_capacity %lld", hs.num_rendered, (long long)a->bin_capacity);
            return EMD_ERR_CAPACITY;
        }
    }
    { int jrc = join(); if (jrc) return jrc; }          // K6 reads the colours
    emd_prof_switch(PROF_RANGES, PROF_RENDER_FWD, st);
    EmdExtra ex;
    memset(&ex, 0, sizeof(ex));
    ex.num = a->num_extra;
    for (int k = 0; k < a->num_extra; k++) { ex.colors[k] = a->colors_extra[k]; ex.out[k] = a->out_extra[k]; }
    if (a->loop_stats && a->num_extra > 0) { emd_set_error("forward: loop_stats (diagnostic counters) only without extra colour sets"); return EMD_ERR_INVALID; }
    rc = emd_launch_render_forward(a->s, a->settings_dev, a->flags, g, b, im, a->out_color, a->out_depth, a->out_normal, a->out_alpha, &ex,
                                   (unsigned long long*)a->loop_stats, st);
    emd_prof_end(PROF_RENDER_FWD, st);
    if (rc) return rc;
    return stage_sync(dbg, st, "render_forward");
}

int emd_raster_backward(const EmdBwdArgs* a, void* hip_stream) {
    if (!a) { emd_set_error("backward: null args"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    const int N = a->num_gaussians;
    int rc = check_common(a->s, N, a->sh_coeffs, a->means3D, a->shs, a->colors_precomp, a->opacities, a->scales,
                          a->rotations, a->cov3D_precomp, a->flags, a->motion);
    if (rc) return rc;
    const int gx = (a->s.image_width + EMD_TILE_X - 1) / EMD_TILE_X, gy = (a->s.image_height + EMD_TILE_Y - 1) / EMD_TILE_Y;
    GeomWs g; BinWs b; ImgWs im;
    emd_carve_bin((void*)a->bin_ws, a->bin_capacity, gx * gy, &b);
    emd_carve_img((void*)a->img_ws, a->s.image_height, a->s.image_width, &im);
    rc = check_bwd_state(a, "backward", &g, b.bytes <= a->bin_bytes && im.bytes <= a->img_bytes);
    if (rc) return rc;
    if ((a->flags & EMD_FLAG_ABSGRAD) && !a->dL_dmeans2D_abs) { emd_set_error("backward: EMD_FLAG_ABSGRAD without dL_dmeans2D_abs"); return EMD_ERR_INVALID; }
    // EMD_FLAG_DETERMINISTIC: no float atomics anywhere in this pass
    const bool det = (a->flags & EMD_FLAG_DETERMINISTIC) != 0;
    const size_t det_slots = 4 * (size_t)(a->bin_capacity > 0 ? a->bin_capacity : 1);       // contribution slots: one per quadrant and list entry
    DetWs dw;
    memset(&dw, 0, sizeof(dw));
    if (det) {
        if (a->pair_stats) { emd_set_error("backward: pair_stats (diagnostic counters of the float atomics) cannot be combined with EMD_FLAG_DETERMINISTIC"); return EMD_ERR_INVALID; }
        if (!emd_det_slots_fit((int64_t)det_slots)) { emd_set_error("backward: EMD_FLAG_DETERMINISTIC: 4 x bin_capacity %lld exceeds 32-bit slot numbers", (long long)a->bin_capacity); return EMD_ERR_INVALID; }
        emd_carve_det(a->det_ws, N, a->bin_capacity, a->num_extra, &dw);
        rc = emd_det_check_ws("backward: EMD_FLAG_DETERMINISTIC", a->det_ws, a->det_bytes, dw.bytes, 64, EMD_ERR_INVALID, "emd_raster_det_workspace_size");
        if (rc) return rc;
    }
    const bool dbg = a->s.debug != 0;
    // the two halves of the pass may arrive as two calls (EMD_FLAG_BWD_RENDER_ONLY, then EMD_FLAG_BWD_PROJECT_ONLY on the same workspaces)
    const bool do_render = !(a->flags & EMD_FLAG_BWD_PROJECT_ONLY), do_project = !(a->flags & EMD_FLAG_BWD_RENDER_ONLY);
    if (!do_render && !do_project) { emd_set_error("backward: EMD_FLAG_BWD_RENDER_ONLY and EMD_FLAG_BWD_PROJECT_ONLY exclude each other"); return EMD_ERR_INVALID; }
    // The dense dL/dshs ([N,16,3]: 192 B per Gaussian, three quarters of them zero rows) is zeroed by K7's own workgroups, a slice each, under its pixel
    // loops (which leave nine tenths of the HBM bandwidth idle), and K8, behind it on the stream, stores the rows of the contributing Gaussians only.  Only
    // when this very call runs both kernels, K7 is launched at all (a tile grid exists), its default instantiation runs (the deterministic one does not fill) and
    // K8 takes its staged path (shs given, 16 coefficients); every other call keeps the dense K8: the two-call form, EMD_FLAG_DETERMINISTIC, the factored SH
    // gradient (no dL_dshs), M != 16.
    const bool shs_prefill = do_render && do_project && !det && a->dL_dshs && a->shs && a->sh_coeffs == 16 && N > 0 && gx * gy > 0;
    if (do_render) {
        emd_prof_begin(PROF_OTHER, st);
        if (!(a->flags & EMD_FLAG_BWD_WS_CLEAN)) { int zrc = emd_zero_async(a->bwd_ws, emd_bwd_bytes(N, a->num_extra), st); if (zrc) return zrc; }
        float* pose_grad = nullptr;       // accumulated by K8 with atomics; cleared by K7's first workgroup
        int pose_grad_n = 0;
        if ((a->flags & EMD_FLAG_MOTION) && a->dL_dactor_pose && a->motion.num_actors > 0) {
            pose_grad = a->dL_dactor_pose;
            pose_grad_n = a->motion.num_actors * EMD_ACTOR_STRIDE;
        }
        emd_prof_switch(PROF_OTHER, PROF_RENDER_BWD, st);
        EmdExtra ex;
        memset(&ex, 0, sizeof(ex));
        ex.num = a->num_extra;
        for (int k = 0; k < a->num_extra; k++) {
            if (!a->colors_extra[k] || !a->out_extra[k]) { emd_set_error("backward: extra colour set %d: null colours / forward output", k); return EMD_ERR_INVALID; }
            ex.colors[k] = a->colors_extra[k]; ex.out[k] = (float*)a->out_extra[k]; ex.dL_dout[k] = a->dL_dextra[k];
        }
        if (a->pair_stats && (a->num_extra > 0 || (a->flags & EMD_FLAG_ABSGRAD) || a->dL_dnormal)) {
            emd_set_error("backward: pair_stats (diagnostic counters) only with the plain call: no extra colour sets, absgrad or normal gradient");
            return EMD_ERR_INVALID;
        }
        rc = emd_launch_render_backward(a->s, a->settings_dev, a->flags, g, b, im, a->out_color, a->out_depth, a->out_normal, a->dL_dcolor,
                                        a->dL_ddepth, a->dL_dalpha, a->dL_dnormal, &ex, (float*)a->bwd_ws, pose_grad, pose_grad_n,
                                        shs_prefill ? (float4*)a->dL_dshs : nullptr, shs_prefill ? (size_t)N * 12 : 0,
                                        (unsigned long long*)a->pair_stats, det ? dw.r.rows : nullptr, st);
        if (rc) return rc;
        if (det) {
            // every contribution row sits in its survivor's slot: list the slots per Gaussian (a stable sort: ascending slot order inside a Gaussian,
            // a function of the bit-exact binning alone) and sum each list in the pinned order into the accumulator rows K8 expects
            rc = emd_launch_det_render_keys(gx * gy, b, a->status, dw.r.s.keys_in, dw.counts, st);
            if (rc) return rc;
            rc = emd_det_sort_and_sum(dw.r, N, dw.counts, dw.counts + 1, (float*)a->bwd_ws, emd_bwd_stride(a->num_extra), st);
            if (rc) return rc;
        }
        if (!do_project && a->dL_dsh_color) {      // the SH factor right behind K7: a view-parallel step starts gathering it under K8
            rc = emd_launch_sh_factor(N, emd_bwd_visible_words(a->flags, a->radii, g), g, (const float*)a->bwd_ws, emd_bwd_stride(a->num_extra), a->dL_dsh_color, st);
            if (rc) return rc;
        }
        if ((rc = stage_sync(dbg, st, "render_backward"))) return rc;
        if (!do_project) { emd_prof_end(PROF_RENDER_BWD, st); return EMD_OK; }
    }
    PreBwdArgs pb;
    fill_bwd_inputs(pb, *a, g);
    pb.dL_dmeans3D = a->dL_dmeans3D; pb.dL_dmeans2D = a->dL_dmeans2D; pb.dL_dmeans2D_abs = a->dL_dmeans2D_abs;
    pb.dL_dshs = a->dL_dshs; pb.dL_dcolors = a->dL_dcolors; pb.dL_dopacities = a->dL_dopacities;
    pb.dL_dscales = a->dL_dscales; pb.dL_drotations = a->dL_drotations; pb.dL_dcov3D = a->dL_dcov3D;
    pb.dL_dactor_pose = a->dL_dactor_pose; pb.dL_dresidual_dx = a->dL_dresidual_dx; pb.dL_dresidual_dq = a->dL_dresidual_dq;
    pb.dL_dsh_color = a->dL_dsh_color;
    pb.shs_prezeroed = shs_prefill ? 1 : 0;
    for (int k = 0; k < EMD_MAX_EXTRA; k++) pb.dL_dextra[k] = k < a->num_extra ? a->dL_dcolors_extra[k] : nullptr;
    const bool det_pose = det && (a->flags & EMD_FLAG_MOTION) && a->dL_dactor_pose && a->motion.num_actors > 0;
    pb.pose_rows = det_pose ? dw.p.rows : nullptr;
    if (do_render) emd_prof_switch(PROF_RENDER_BWD, PROF_PREPROCESS_BWD, st); else emd_prof_begin(PROF_PREPROCESS_BWD, st);
    rc = emd_launch_preprocess_backward(pb, st);
    if (!rc && det_pose && a->motion.actor_id && N > 0) {
        // K8 stored the pose gradient of every visible actor-bound point: the points by actor (stable: ascending point index), the rows summed in the
        // pinned order.  Actors without a visible point keep the zeros K7's first workgroup wrote.
        rc = emd_launch_det_pose_keys(N, a->radii, a->motion.actor_id, dw.p.s.keys_in, st);
        if (rc) return rc;
        rc = emd_det_sort_and_sum(dw.p, a->motion.num_actors, nullptr, dw.counts + 2, a->dL_dactor_pose, EMD_ACTOR_STRIDE, st);
    }
    emd_prof_end(PROF_PREPROCESS_BWD, st);
    if (rc) return rc;
    return stage_sync(dbg, st, "preprocess_backward");
}

int emd_backward_fill_slice(uint64_t count, uint32_t grid, uint32_t block, uint64_t out[2]) {
    if (!out || grid == 0 || block >= grid) { emd_set_error("backward_fill_slice: bad argument (grid=%u block=%u)", grid, block); return EMD_ERR_INVALID; }
    emd_fill_slice(count, emd_fill_per(count, grid), block, &out[0], &out[1]);
    return EMD_OK;
}

static int check_det_dims(const EmdDims* dims, const char* who) {
    if (!dims) { emd_set_error("%s: null argument", who); return EMD_ERR_INVALID; }
    if (dims->num_gaussians < 0 || dims->bin_capacity < 0 || dims->num_extra < 0 || dims->num_extra > EMD_MAX_EXTRA) {
        emd_set_error("%s: bad dims N=%d cap=%lld num_extra=%d", who, dims->num_gaussians, (long long)dims->bin_capacity, dims->num_extra);
        return EMD_ERR_INVALID;
    }
    return EMD_OK;
}

int emd_raster_det_workspace_size(const EmdDims* dims, size_t* bytes) {
    int rc = check_det_dims(dims, "det_workspace_size");
    if (rc) return rc;
    if (!bytes) { emd_set_error("det_workspace_size: null argument"); return EMD_ERR_INVALID; }
    DetWs w;
    emd_carve_det(nullptr, dims->num_gaussians, dims->bin_capacity, dims->num_extra, &w);
    *bytes = w.bytes;
    return EMD_OK;
}

int emd_raster_det_layout(const EmdDims* dims, int32_t num_actors, size_t out[15]) {
    int rc = check_det_dims(dims, "det_layout");
    if (rc) return rc;
    if (!out) { emd_set_error("det_layout: null argument"); return EMD_ERR_INVALID; }
    DetWs w;
    emd_carve_det(nullptr, dims->num_gaussians, dims->bin_capacity, dims->num_extra, &w);
    const DetSortWs &r = w.r.s, &p = w.p.s;
    const void* at[15] = {w.r.rows, r.keys[0], r.keys[1], r.vals[0], r.vals[1], w.counts, w.p.rows, p.keys[0], p.keys[1], p.vals[0], p.vals[1],
                          nullptr, nullptr, r.keys_in, p.keys_in};
    for (int i = 0; i < 15; i++) out[i] = emd_det_offset(at[i]);
    out[11] = (size_t)emd_det_sorted_buf(dims->num_gaussians);
    out[12] = (size_t)emd_det_sorted_buf(num_actors);
    return EMD_OK;
}

int emd_camera_grad_workspace_size(int32_t num_gaussians, size_t* bytes) {
    if (!bytes || num_gaussians < 0) { emd_set_error("camera_grad_workspace_size: bad argument (N=%d)", num_gaussians); return EMD_ERR_INVALID; }
    *bytes = emd_camera_grad_bytes(num_gaussians);
    return EMD_OK;
}

int emd_raster_backward_camera(const EmdBwdArgs* a, float* dL_dcamera, void* workspace, size_t workspace_bytes, void* hip_stream) {
    if (!a) { emd_set_error("backward_camera: null args"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    const int N = a->num_gaussians;
    int rc = check_common(a->s, N, a->sh_coeffs, a->means3D, a->shs, a->colors_precomp, a->opacities, a->scales,
                          a->rotations, a->cov3D_precomp, a->flags, a->motion);
    if (rc) return rc;
    if (!dL_dcamera) { emd_set_error("backward_camera: null dL_dcamera"); return EMD_ERR_INVALID; }
    if (a->dL_dnormal) {
        // the normal image depends on the view matrix (nv = V nw and its sign flip): that path has no camera gradient yet -- refused, not left out
        emd_set_error("backward_camera: the camera gradient does not cover the normal image; call without dL_dnormal");
        return EMD_ERR_INVALID;
    }
    GeomWs g;
    rc = check_bwd_state(a, "backward_camera", &g, workspace && workspace_bytes >= emd_camera_grad_bytes(N));
    if (rc) return rc;
    if ((uintptr_t)workspace & 15) { emd_set_error("backward_camera: workspace must be 16-byte aligned"); return EMD_ERR_INVALID; }
    PreBwdArgs pb;
    memset(&pb, 0, sizeof(pb));                // (no gradient outputs: the kernel writes the workspace and dL_dcamera only)
    fill_bwd_inputs(pb, *a, g);
    rc = emd_launch_camera_backward(pb, (float*)workspace, dL_dcamera, st);
    if (rc) return rc;
    return stage_sync(a->s.debug != 0, st, "camera_backward");
}

// The binning stage on caller-supplied projection outputs (tests/test_binning_gpu.py): the records go where K1 leaves them, the stage runs as in the forward.
int emd_raster_binning(const EmdBinningArgs* a, void* hip_stream) {
    if (!a) { emd_set_error("binning: null args"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    const int N = a->num_gaussians;
    if (a->flags & ~EMD_FLAG_WIDE_DEPTH_SORT) { emd_set_error("binning: flags 0x%x: only EMD_FLAG_WIDE_DEPTH_SORT is read", a->flags); return EMD_ERR_INVALID; }
    if (N < 0 || a->image_height <= 0 || a->image_width <= 0 || a->bin_capacity < 0) {
        emd_set_error("binning: bad sizes N=%d H=%d W=%d cap=%lld", N, a->image_height, a->image_width, (long long)a->bin_capacity); return EMD_ERR_INVALID;
    }
    if ((int64_t)N >= (int64_t)1 << 28) { emd_set_error("binning: %d Gaussians; a list word holds a 28-bit Gaussian id beside the pair's quadrant mask", N); return EMD_ERR_INVALID; }
    const int gx = (a->image_width - 1) / EMD_TILE_X + 1, gy = (a->image_height - 1) / EMD_TILE_Y + 1;
    if (gx >= 1024 || gy >= 1024) { emd_set_error("binning: image too large: %d x %d tiles (max 1023)", gx, gy); return EMD_ERR_INVALID; }
    if (!a->geom_ws || !a->bin_ws || !a->status || (N > 0 && (!a->depth_key || !a->binrec))) { emd_set_error("binning: null pointer"); return EMD_ERR_INVALID; }
    GeomWs g; BinWs b;
    emd_carve_geom(a->geom_ws, N, &g);
    emd_carve_bin(a->bin_ws, a->bin_capacity, gx * gy, &b);
    if (g.bytes > a->geom_bytes || b.bytes > a->bin_bytes) {
        emd_set_error("binning: workspace too small (geom %zu/%zu bin %zu/%zu)", a->geom_bytes, g.bytes, a->bin_bytes, b.bytes);
        return EMD_ERR_WORKSPACE;
    }
    if (N > 0) {
        EMD_HIP_CHECK(hipMemcpyAsync(g.depth_key, a->depth_key, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
        EMD_HIP_CHECK(hipMemcpyAsync(g.binrec, a->binrec, (size_t)N * 8, hipMemcpyDeviceToDevice, st));
    }
    { int zrc = emd_zero_async(a->status, sizeof(EmdStatus), st); if (zrc) return zrc; }      // (K1 clears it: the depth sort ORs into the overflow word)
    EmdSettings s;
    memset(&s, 0, sizeof(s));
    s.image_height = a->image_height; s.image_width = a->image_width; s.near_plane = a->near_plane;
    const int rc = emd_launch_binning(s, a->flags, N, g, b, a->bin_capacity, a->status, st);
    emd_prof_end(PROF_RANGES, st);
    if (rc) return rc;
    if (a->tile_order) EMD_HIP_CHECK(hipMemcpyAsync(a->tile_order, b.tile_order, (size_t)gx * gy * 4, hipMemcpyDeviceToDevice, st));
    return EMD_OK;
}

int emd_raster_export_binning(const EmdDims* dims, const void* geom_ws, size_t geom_bytes, const void* bin_ws, size_t bin_bytes,
                              int64_t num_rendered, uint64_t* keys, uint32_t* ids, uint32_t* ranges, uint32_t* quad_masks,
                              void* hip_stream) {
    if (!dims || !bin_ws || !geom_ws) { emd_set_error("export_binning: null argument"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    const int gx = (dims->image_width + EMD_TILE_X - 1) / EMD_TILE_X, gy = (dims->image_height + EMD_TILE_Y - 1) / EMD_TILE_Y;
    GeomWs g; BinWs b;
    emd_carve_geom((void*)geom_ws, dims->num_gaussians, &g);
    emd_carve_bin((void*)bin_ws, dims->bin_capacity, gx * gy, &b);
    if (g.bytes > geom_bytes || b.bytes > bin_bytes || num_rendered > dims->bin_capacity || num_rendered < 0) { emd_set_error("export_binning: bad sizes"); return EMD_ERR_WORKSPACE; }
    // the sort moves (tile id, Gaussian id) pairs; upstream's 64-bit key is tile id << 32 | depth bits of the Gaussian
    if ((keys || ids || quad_masks) && num_rendered) { int rc = emd_launch_export_keys(num_rendered, g, b, keys, ids, quad_masks, st); if (rc) return rc; }
    if (ranges) EMD_HIP_CHECK(hipMemcpyAsync(ranges, b.ranges, (size_t)gx * gy * 8, hipMemcpyDeviceToDevice, st));
    return EMD_OK;
}

int emd_raster_export_geometry(const EmdDims* dims, const void* geom_ws, size_t geom_bytes, float* means2D,
                               float* depths, float* conic_opacity, float* rgb, float* normal, uint32_t* tiles_touched,
                               void* hip_stream) {
    if (!dims || !geom_ws) { emd_set_error("export_geometry: null argument"); return EMD_ERR_INVALID; }
    GeomWs g;
    emd_carve_geom((void*)geom_ws, dims->num_gaussians, &g);
    if (g.bytes > geom_bytes) { emd_set_error("export_geometry: workspace too small"); return EMD_ERR_WORKSPACE; }
    return emd_launch_export_geometry(dims->num_gaussians, g, means2D, depths, conic_opacity, rgb, normal, tiles_touched,
                                      (hipStream_t)hip_stream);
}

int emd_raster_export_contributed(const EmdDims* dims, const void* geom_ws, size_t geom_bytes, uint32_t* contributed, void* hip_stream) {
    if (!dims || !geom_ws || !contributed) { emd_set_error("export_contributed: null argument"); return EMD_ERR_INVALID; }
    if (dims->num_gaussians < 0) { emd_set_error("export_contributed: bad dims N=%d", dims->num_gaussians); return EMD_ERR_INVALID; }
    GeomWs g;
    emd_carve_geom((void*)geom_ws, dims->num_gaussians, &g);
    if (g.bytes > geom_bytes) { emd_set_error("export_contributed: workspace too small"); return EMD_ERR_WORKSPACE; }
    if (dims->num_gaussians > 0)
        EMD_HIP_CHECK(hipMemcpyAsync(contributed, g.contrib, (size_t)dims->num_gaussians * 4, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
    return EMD_OK;
}

int emd_motion_forward(int32_t n, const float* means, const float* quats, const float* opacities,
                       const EmdMotion* motion, float* world_means, float* world_quats, float* opacities_out,
                       void* hip_stream) {
    if (n < 0 || !means || !motion) { emd_set_error("motion_forward: bad argument"); return EMD_ERR_INVALID; }
    if (motion->actor_id && (!motion->actor_pose || motion->num_actors <= 0)) { emd_set_error("motion_forward: actor_id without actor_pose"); return EMD_ERR_INVALID; }
    return emd_launch_motion_forward(n, means, quats, opacities, *motion, world_means, world_quats, opacities_out,
                                     (hipStream_t)hip_stream);
}

int emd_motion_backward(int32_t n, const float* means, const float* quats, const float* opacities,
                        const EmdMotion* motion, const float* dL_dworld_means, const float* dL_dworld_quats,
                        const float* dL_dopacities_out, float* dL_dmeans, float* dL_dquats, float* dL_dopacities,
                        float* dL_dactor_pose, float* dL_dresidual_dx, float* dL_dresidual_dq, void* hip_stream) {
    if (n < 0 || !means || !motion) { emd_set_error("motion_backward: bad argument"); return EMD_ERR_INVALID; }
    if (motion->actor_id && (!motion->actor_pose || motion->num_actors <= 0)) { emd_set_error("motion_backward: actor_id without actor_pose"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    if (dL_dactor_pose && motion->num_actors > 0)
        { int zrc = emd_zero_async(dL_dactor_pose, (size_t)motion->num_actors * EMD_ACTOR_STRIDE * sizeof(float), st); if (zrc) return zrc; }
    return emd_launch_motion_backward(n, means, quats, opacities, *motion, dL_dworld_means, dL_dworld_quats,
                                      dL_dopacities_out, dL_dmeans, dL_dquats, dL_dopacities, dL_dactor_pose,
                                      dL_dresidual_dx, dL_dresidual_dq, st);
}

// The workspace of the stand-alone motion backward's deterministic form: the pose half of DetWs alone -- the [n][EMD_ACTOR_STRIDE] pose gradient of
// every actor-bound point (k_motion_backward_det) and the sort of the points by actor id.  The mode serves the n whose 4 n fit the slot numbers.
static bool motion_det_fits(int64_t n) { return emd_det_slots_fit(4 * n); }
static void carve_motion_det(void* base, int64_t n, DetUnitWs* w) { emd_carve_det_unit(base, (size_t)(n > 0 ? n : 1), EMD_ACTOR_STRIDE, EMD_ACTOR_STRIDE, w); }

size_t emd_motion_det_workspace_size(int32_t n) {
    if (!motion_det_fits(n)) return 0;
    DetUnitWs w;
    carve_motion_det(nullptr, n, &w);
    return w.bytes;
}

int emd_motion_det_workspace_offsets(int32_t n, int32_t num_actors, size_t out[6]) {
    if (!out || !motion_det_fits(n) || num_actors < 1) { emd_set_error("motion_det_workspace_offsets: bad argument (n = %d, num_actors = %d)", n, num_actors); return EMD_ERR_INVALID; }
    DetUnitWs w;
    carve_motion_det(nullptr, n, &w);
    emd_det_unit_offsets(w, num_actors, out);
    return EMD_OK;
}

// emd_motion_backward with the pose gradient summed in a pinned order: rows, a stable compacting sort by actor, the segmented
// row sum.  The per-point outputs are the default entry's.
int emd_motion_backward_det(int32_t n, const float* means, const float* quats, const float* opacities,
                            const EmdMotion* motion, const float* dL_dworld_means, const float* dL_dworld_quats,
                            const float* dL_dopacities_out, float* dL_dmeans, float* dL_dquats, float* dL_dopacities,
                            float* dL_dactor_pose, float* dL_dresidual_dx, float* dL_dresidual_dq, void* det_ws, size_t det_bytes,
                            void* hip_stream) {
    if (n < 0 || !means || !motion) { emd_set_error("motion_backward_det: bad argument"); return EMD_ERR_INVALID; }
    if (motion->actor_id && (!motion->actor_pose || motion->num_actors <= 0)) { emd_set_error("motion_backward_det: actor_id without actor_pose"); return EMD_ERR_INVALID; }
    if (!motion_det_fits(n)) { emd_set_error("motion_backward_det: the deterministic mode serves 4 n <= 2^32 - 1 - %d (n = %d)", EMD_SORT_TILE, n); return EMD_ERR_INVALID; }
    // everything is decided here, before the first launch
    const bool pose = dL_dactor_pose && motion->num_actors > 0;
    DetUnitWs w;
    memset(&w, 0, sizeof(w));
    if (pose) {
        carve_motion_det(det_ws, n, &w);
        const int wrc = emd_det_check_ws("motion_backward_det", det_ws, det_bytes, w.bytes, 256, EMD_ERR_WORKSPACE, "emd_motion_det_workspace_size");
        if (wrc) return wrc;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (pose) { int zrc = emd_zero_async(dL_dactor_pose, (size_t)motion->num_actors * EMD_ACTOR_STRIDE * sizeof(float), st); if (zrc) return zrc; }
    int rc = emd_launch_motion_backward_det(n, means, quats, opacities, *motion, dL_dworld_means, dL_dworld_quats, dL_dopacities_out, dL_dmeans, dL_dquats,
                                            dL_dopacities, dL_dresidual_dx, dL_dresidual_dq, w.r.rows, w.r.s.keys_in, st);
    if (rc || !pose || n == 0) return rc;
    return emd_det_sort_and_sum(w.r, motion->num_actors, nullptr, w.counts, dL_dactor_pose, EMD_ACTOR_STRIDE, st);
}

int emd_sh_forward(int32_t n, int32_t degree, int32_t sh_coeffs, const float* dirs, const float* coeffs, float* rgb,
                   void* hip_stream) {
    if (n < 0 || degree < 0 || degree > 3 || sh_coeffs < (degree + 1) * (degree + 1) || !dirs || !coeffs || !rgb) {
        emd_set_error("sh_forward: bad argument (n=%d degree=%d K=%d)", n, degree, sh_coeffs); return EMD_ERR_INVALID;
    }
    return emd_launch_sh_forward(n, degree, sh_coeffs, dirs, coeffs, rgb, (hipStream_t)hip_stream);
}

int emd_sh_backward(int32_t n, int32_t degree, int32_t sh_coeffs, const float* dirs, const float* coeffs,
                    const float* dL_drgb, float* dL_dcoeffs, float* dL_ddirs, void* hip_stream) {
    if (n < 0 || degree < 0 || degree > 3 || sh_coeffs < (degree + 1) * (degree + 1) || !dirs || !coeffs || !dL_drgb) {
        emd_set_error("sh_backward: bad argument (n=%d degree=%d K=%d)", n, degree, sh_coeffs); return EMD_ERR_INVALID;
    }
    return emd_launch_sh_backward(n, degree, sh_coeffs, dirs, coeffs, dL_drgb, dL_dcoeffs, dL_ddirs, (hipStream_t)hip_stream);
}

int emd_sh_grad_from_factors(int32_t n, int32_t num_views, int32_t degree, int32_t sh_coeffs, const float* means3D,
                             const EmdMotion* motion, int32_t pose_per_view, const float* campos, const float* sh_color_grads,
                             float scale, float* dL_dshs, void* hip_stream) {
    if (n < 0 || num_views < 1 || degree < 0 || degree > 3 || sh_coeffs < (degree + 1) * (degree + 1) || sh_coeffs > 16 ||
        (n > 0 && (!means3D || !campos || !sh_color_grads || !dL_dshs))) {
        emd_set_error("sh_grad_from_factors: bad argument"); return EMD_ERR_INVALID;
    }
    EmdMotion mo;
    memset(&mo, 0, sizeof(mo));
    if (motion) mo = *motion;
    return emd_launch_sh_grad_from_factors(n, num_views, degree, sh_coeffs, means3D, mo, pose_per_view ? 1 : 0, campos, sh_color_grads, scale, dL_dshs,
                                           (hipStream_t)hip_stream);
}

int emd_densification_stats(int32_t n, const int32_t* radii, const float* dL_dmeans2D, float* grad_accum, float* denom,
                            float* max_radii2D, void* hip_stream) {
    if (n < 0 || (n > 0 && (!radii || !dL_dmeans2D))) { emd_set_error("densification_stats: bad argument"); return EMD_ERR_INVALID; }
    return emd_launch_densification_stats(n, radii, dL_dmeans2D, grad_accum, denom, max_radii2D, (hipStream_t)hip_stream);
}

int emd_actor_pose_forward(int32_t num_actors, const float* q_f, const float* t_f, const uint8_t* valid, const float* dt,
                           const float* dq, float* pose, const int32_t* frame_dev, void* hip_stream) {
    if (num_actors < 0 || (num_actors > 0 && (!q_f || !t_f || !pose))) { emd_set_error("actor_pose_forward: bad argument"); return EMD_ERR_INVALID; }
    return emd_launch_actor_pose_forward(num_actors, q_f, t_f, valid, dt, dq, pose, frame_dev, (hipStream_t)hip_stream);
}

int emd_actor_pose_backward(int32_t num_actors, const float* q_f, const float* dt, const float* dq, const float* dL_dpose,
                            float* dL_dq_f, float* dL_dt_f, float* dL_ddt, float* dL_ddq, const int32_t* frame_dev, void* hip_stream) {
    if (num_actors < 0 || (num_actors > 0 && (!q_f || !dL_dpose || !dL_dq_f || !dL_dt_f))) { emd_set_error("actor_pose_backward: bad argument"); return EMD_ERR_INVALID; }
    return emd_launch_actor_pose_backward(num_actors, q_f, dt, dq, dL_dpose, dL_dq_f, dL_dt_f, dL_ddt, dL_ddq, frame_dev, (hipStream_t)hip_stream);
}

int emd_select_step_inputs(const EmdStepSelect* a, void* hip_stream) {
    if (!a || !a->sel) { emd_set_error("select_step_inputs: null args"); return EMD_ERR_INVALID; }
    if (a->rows < 0 || a->row_floats < 0 || (a->row_floats > 0 && (!a->table || !a->out_row)) || (a->k_fine_out && a->k_until < 1)) {
        emd_set_error("select_step_inputs: bad sizes / null table"); return EMD_ERR_INVALID;
    }
    hipLaunchKernelGGL(k_select_step_inputs, dim3(1), dim3(EMD_WAVE), 0, (hipStream_t)hip_stream, *a);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_l1_loss_ws(int64_t n, const float* a, const float* b, float* loss, float* grad, uint32_t* scratch, void* hip_stream) {
    if (n < 0 || !loss || (n > 0 && !a)) { emd_set_error("l1_loss: bad argument"); return EMD_ERR_INVALID; }
    if (((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)grad & 15)) { emd_set_error("l1_loss: a, b, grad must be 16-byte aligned"); return EMD_ERR_INVALID; }
    if ((uintptr_t)scratch & 7) { emd_set_error("l1_loss: scratch must be 8-byte aligned"); return EMD_ERR_INVALID; }
    return emd_launch_l1_loss((size_t)n, a, b, loss, grad, scratch, (hipStream_t)hip_stream);
}

int emd_l1_loss(int64_t n, const float* a, const float* b, float* loss, float* grad, void* hip_stream) {
    return emd_l1_loss_ws(n, a, b, loss, grad, nullptr, hip_stream);
}

int emd_abs_mean_backward(int64_t n, const float* x, const float* g, float* grad, void* hip_stream) {
    if (n < 0 || (n > 0 && (!x || !g || !grad))) { emd_set_error("abs_mean_backward: bad argument"); return EMD_ERR_INVALID; }
    if (((uintptr_t)x & 15) || ((uintptr_t)grad & 15)) { emd_set_error("abs_mean_backward: x, grad must be 16-byte aligned"); return EMD_ERR_INVALID; }
    return emd_launch_abs_mean_backward((size_t)n, x, g, grad, (hipStream_t)hip_stream);
}

int emd_residual_l1_backward(int64_t n, const float* up_a, const float* up_b, const float* x_a, const float* x_b, const float* g_a,
                             const float* g_b, float* grad_a, float* grad_b, void* hip_stream) {
    if (n < 0 || (n > 0 && (!x_a || !x_b || !grad_a || !grad_b))) { emd_set_error("residual_l1_backward: bad argument"); return EMD_ERR_INVALID; }
    if ((((uintptr_t)up_a) | ((uintptr_t)up_b) | ((uintptr_t)x_a) | ((uintptr_t)x_b) | ((uintptr_t)grad_a) | ((uintptr_t)grad_b)) & 15) {
        emd_set_error("residual_l1_backward: the tensors must be 16-byte aligned"); return EMD_ERR_INVALID;
    }
    return emd_launch_residual_l1_backward((size_t)n, up_a, up_b, x_a, x_b, g_a, g_b, grad_a, grad_b, (hipStream_t)hip_stream);
}

int emd_activations_forward(int32_t n, const float* log_scales, float* scales, const float* raw_quats, float* quats,
                            const float* opacity_logits, float* opacities, void* hip_stream) {
    if (n < 0) { emd_set_error("activations_forward: negative n"); return EMD_ERR_INVALID; }
    return emd_launch_activations(n, log_scales, scales, raw_quats, quats, opacity_logits, opacities, (hipStream_t)hip_stream);
}

}  // extern "C"
