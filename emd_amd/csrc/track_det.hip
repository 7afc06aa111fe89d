// track_det.hip -- the per-actor chain of embed.hip (embedding sums -> track heads -> pose row) and the gradient of the DeformableNodes encoder input
// without float atomics.  A unit of its own: embed.hip's kernels are pinned instruction for instruction
// (profiles/track_det_isa.txt), and a further kernel inside that unit changed the code of its neighbours (section 8.14).  The per-actor helpers the
// two units share -- te_eval / te_column2, wave_sum_all, head_of / head_row / head_coarse, heads_eval -- and the argument checks are ONE text,
// track_heads.h, which both include (embed.hip kept its instructions across the move: profiles/shared_source_isa.txt).  That header holds no atomic.
//
//   emd_actor_row_sum_det            out[a] = the pinned segmented sum (segsum.h) of the rows i with ids[i] == a, in ascending i
//   emd_track_heads_forward_det      the embedding sums by that row sum when the ids are not sorted by actor (or E > 8), then embed.hip's heads
//   emd_track_heads_backward_det     k_track_heads<true> without atomics, then embed.hip's own k_track_embed_bwd (per point, no reduction)
//   emd_tracked_pose_backward_det    k_tracked_pose<true> without atomics
// Head gradients: every actor STORES its share of the eight head tensors to its own slot of a slab [A][pitch]; one launch adds the slots per element in
// ascending actor index in fp64 from 0.0 and rounds once.  Temporal table: the gather form of embed_det.hip over the two levels (te_gather_body.inc).
#include <string.h>

#include "common.h"
#include "det_reduce.h"
#include "quat_math.h"
#include "temporal_sample.h"
#include "track_heads.h"

namespace {

// The slot of one actor in the slab: the eight head tensors back to back, as EmdTrackedPoseArgs.head_acc has them -- w_tc [3 w], b_tc [3], w_tf [3 w],
// b_tf [3], w_rc [w], b_rc [1], w_rf [w], b_rf [1]: 8 w + 8 floats, w = dim + embed_dim.
__host__ __device__ constexpr int slot_w(int h, int w) { return h == 0 ? 0 : h == 1 ? 3 * w + 3 : h == 2 ? 6 * w + 6 : 7 * w + 7; }
__host__ __device__ constexpr int slot_b(int h, int w) { return h == 0 ? 3 * w : h == 1 ? 6 * w + 3 : h == 2 ? 7 * w + 6 : 8 * w + 7; }
inline int slot_floats(int w) { return 8 * w + 8; }
inline int slab_pitch(int w) { return (slot_floats(w) + 15) / 16 * 16; }

struct TrackDetWs {
    float* slab;             // [A][pitch] every actor's share of the head gradients
    float* dh;               // [A][2][64] every actor's per-lane dL/dh_c, dL/dh_f
    DetSortWs s;             // n points -> actor ids (the row sum, whose rows are the caller's)
    uint32_t* counts;        // [16] device-side counts: [0] points the sort kept
    size_t bytes;
};
void carve_track_det(void* base, int num_actors, int head_width, int64_t n_points, int row_width, TrackDetWs* w) {
    char* p = (char*)base;
    size_t off = 0;
    const size_t A = (size_t)(num_actors > 0 ? num_actors : 1), n = (size_t)(n_points > 0 ? n_points : 1);
    const bool chain = head_width > 0, sum = row_width > 0 && n_points > 0;
    w->slab = (float*)(p + off); off = emd_align_up(off + (chain ? A * slab_pitch(head_width) * sizeof(float) : 0), 256);
    w->dh = (float*)(p + off); off = emd_align_up(off + (chain ? A * 2 * EMD_WAVE * sizeof(float) : 0), 256);
    if (sum) emd_carve_det_sort(p, off, n, row_width < 32 ? row_width : 32, &w->s);
    else memset(&w->s, 0, sizeof(w->s));
    w->counts = emd_carve_det_counts(p, off);
    w->bytes = off + 256;
}
bool track_det_sizes_ok(int num_actors, int head_width, int64_t n, int row_width) {
    return num_actors >= 0 && head_width >= 0 && head_width <= EMD_WAVE && emd_det_track_points_fit(n) && row_width >= 0 && row_width <= 64;
}
// the workspace of a call with these sizes, carved at ws and checked (missing, short or misaligned: EMD_ERR_WORKSPACE)
int carve_checked(const char* who, void* ws, size_t have, int num_actors, int head_width, int64_t n_points, int row_width, TrackDetWs* w) {
    carve_track_det(ws, num_actors, head_width, n_points, row_width, w);
    return emd_det_check_ws(who, ws, have, w->bytes, 256, EMD_ERR_WORKSPACE, "emd_track_det_workspace_size");
}

// ---- (a) per-actor row sum ------------------------------------------------------------------------------------------------------------------------
// keys of the compacting sort (an id outside [0, A) contributes nothing) and the +0.0 of every actor's row: an actor without a point keeps it
__global__ void __launch_bounds__(EMD_BLOCK) k_row_sum_keys(int n, int A, const int32_t* __restrict__ ids, uint32_t* __restrict__ keys_in, float* __restrict__ out,
                                                            int width, int out_pitch) {
    const size_t i = (size_t)blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i < (size_t)n) { const int id = ids[i]; keys_in[i] = (id >= 0 && id < A) ? (uint32_t)id : 0xFFFFFFFFu; }
    if (i < (size_t)A * width) { const size_t a = i / width; out[a * out_pitch + (i - a * width)] = 0.f; }
}
// ids sorted by actor: point i belongs to the actor a with start[a] <= i < start[a + 1] (start[0] = 0, start[A] = n) -- the sorted list without a sort
__global__ void __launch_bounds__(EMD_BLOCK) k_row_sum_keys_seg(int n, int A, const int32_t* __restrict__ start, uint32_t* __restrict__ keys, uint32_t* __restrict__ slots,
                                                                float* __restrict__ out, int width, int out_pitch) {
    const size_t i = (size_t)blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i < (size_t)n) {
        int lo = 0, hi = A - 1;                                  // the last a with start[a] <= i, inside [0, A - 1] whatever the table holds
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (start[mid] <= (int)i) lo = mid; else hi = mid - 1;
        }
        keys[i] = (uint32_t)lo; slots[i] = (uint32_t)i;
    }
    if (i < (size_t)A * width) { const size_t a = i / width; out[a * out_pitch + (i - a * width)] = 0.f; }
}

int row_sum(int n, int width, const float* rows, int row_pitch, const int32_t* ids, int A, const int32_t* seg, float* out, int out_pitch, const TrackDetWs& w,
            hipStream_t st) {
    const size_t work = (size_t)n > (size_t)A * width ? (size_t)n : (size_t)A * width;
    const unsigned blocks = (unsigned)((work + EMD_BLOCK - 1) / EMD_BLOCK);
    const int w0 = width < 32 ? width : 32;
    SegSumArgs ss;
    ss.n_cap = (size_t)n; ss.rows = rows; ss.row_pitch = row_pitch; ss.width = w0; ss.out = out; ss.out_pitch = out_pitch; ss.partials = w.s.partials;
    if (seg) {
        hipLaunchKernelGGL(k_row_sum_keys_seg, dim3(blocks), dim3(EMD_BLOCK), 0, st, n, A, seg, w.s.keys[0], w.s.vals[0], out, width, out_pitch);
        EMD_LAUNCH_CHECK();
        ss.keys = w.s.keys[0]; ss.slots = w.s.vals[0]; ss.n_dev = nullptr;
        int rc = emd_launch_segmented_row_sum(ss, st);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(k_row_sum_keys, dim3(blocks), dim3(EMD_BLOCK), 0, st, n, A, ids, w.s.keys_in, out, width, out_pitch);
        EMD_LAUNCH_CHECK();
        const DetReduction r = {const_cast<float*>(rows), w.s, (size_t)n, row_pitch, w0};      // the caller's rows: read, never written
        int rc = emd_det_sort_and_sum(r, A, nullptr, w.counts, out, out_pitch, st);
        if (rc) return rc;
        const int buf = emd_det_sorted_buf(A);
        ss.keys = w.s.keys[buf]; ss.slots = w.s.vals[buf]; ss.n_dev = w.counts;
    }
    if (width > 32) {                                            // the second column band over the same sorted list
        ss.rows = rows + 32; ss.out = out + 32; ss.width = width - 32;
        return emd_launch_segmented_row_sum(ss, st);
    }
    return EMD_OK;
}

// ---- (b) the backward of the actor chain ------------------------------------------------------------------------------------------------------------
struct ChainBwd {
    EmdTrackedPoseArgs p;                        // the heads form fills p.track alone
    const float *g_pose, *g_trans, *g_rot;       // the pose row's gradient (pose form) or the offsets' (heads form)
    float *d_q_all, *d_t_all, *d_weight, *d_embeddings, *d_mean;
    float* slab; int pitch;
    float* dh;
};

// One 1024-thread workgroup per actor, as k_tracked_pose<true>.  Wave 0 runs heads and pose row; the other waves clear what the workgroup owns.  Then
// the table gradient in gather form: slots q = 4 level + 2 r + (0: ha, 1: hb) name the at most eight touched rows; the lane of (q, column c) owns
// element (row[q], c) when no earlier slot names the same row (a slot of the row past the end names none), and adds ITS contributions in the default
// kernel's issue order -- column j ascending, coarse before fine, r = 0, 1, then (ha, x0), (hb, x0), (ha, x1), (hb, x1) --, each product formed as
// te_scatter forms it, in fp64 from 0.0, rounded once and written.
#define TRK_THREADS 1024
template <bool POSE>
__global__ void __launch_bounds__(TRK_THREADS) k_track_chain_bwd_det(ChainBwd b) {
    __shared__ float s_dh[2][EMD_WAVE], s_wx0[EMD_WAVE], s_wx1[EMD_WAVE], s_dmean[8];
    __shared__ int s_x0[EMD_WAVE], s_inx1[EMD_WAVE];
    const EmdTrackArgs& a = b.p.track;
    const int act = blockIdx.x, A = a.num_actors, dim = a.dim, E = a.embed_dim, width = dim + E;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float t = a.t_dev ? a.t_dev[0] : a.t;
    const int k_fine = a.k_fine_dev ? min(max(a.k_fine_dev[0], 1), a.rows) : a.k_fine;
    const TeSample sc = te_rows(t, a.k_coarse, a.rows), sf = te_rows(t, k_fine, a.rows);
    const int frame = POSE ? (b.p.frame_dev ? min(max(b.p.frame_dev[0], 0), b.p.num_frames - 1) : b.p.frame) : 0;
    float* G = b.d_weight + (size_t)act * a.rows * dim;
    // every element of what the workgroup owns is defined by this call: +0.0 where nothing is added
    for (int i = threadIdx.x; i < a.rows * dim; i += TRK_THREADS) G[i] = 0.f;
    if (POSE) {
        for (int f = threadIdx.x; f < b.p.num_frames; f += TRK_THREADS) {
            if (f == frame) continue;
            float* dq = b.d_q_all + ((size_t)f * A + act) * 4;
            float* dt = b.d_t_all + ((size_t)f * A + act) * 3;
            dq[0] = dq[1] = dq[2] = dq[3] = 0.f; dt[0] = dt[1] = dt[2] = 0.f;
        }
    }
    if (wave == 1 && lane < dim) {
        const TeCol c = te_col(lane, dim);
        s_x0[lane] = c.x0; s_inx1[lane] = c.inx1 ? 1 : 0; s_wx0[lane] = c.wx0; s_wx1[lane] = c.wx1;
    }
    if (wave == 0) {
        const float cnt = a.count[act];
        float hc = 0.f, hf = 0.f, wrow[8], hbias[8];
        if (lane < dim) te_column2(a.weight + (size_t)act * a.rows * dim, dim, sc, sf, lane, &hc, &hf);
        else if (lane < width) hc = hf = a.emb_sum[(size_t)act * E + (lane - dim)] / cnt;
#pragma unroll
        for (int o = 0; o < 8; o++) {
            wrow[o] = lane < width ? a.head_w[head_of(o)][head_row(o) * width + lane] : 0.f;
            hbias[o] = a.head_b[head_of(o)][head_row(o)];
        }
        float out[8], ow, oz, gt[3], gw, gz;
        heads_eval(wrow, hbias, hc, hf, out, &ow, &oz);
        if (POSE) {
            // the pose row of this actor, with the default's arithmetic (pose_row_backward, quat_math.h: no contraction)
            const float* q_f = b.p.q_all + ((size_t)frame * A + act) * 4;
            const float* gp = b.g_pose + (size_t)act * EMD_ACTOR_STRIDE;
            float qf[4], gp_in[12], dqf[4], dr[4];
#pragma unroll
            for (int k = 0; k < 4; k++) qf[k] = q_f[k];
#pragma unroll
            for (int k = 0; k < 12; k++) gp_in[k] = gp[k];
            const float dtv[3] = {out[0] + out[3], out[1] + out[4], out[2] + out[5]};
            const float dqv[4] = {ow, 0.f, 0.f, oz};
            pose_row_backward(qf, true, dtv, true, dqv, gp_in, dqf, gt, dr);
            if (lane == 0) {
                float* dq = b.d_q_all + ((size_t)frame * A + act) * 4;
                float* dt = b.d_t_all + ((size_t)frame * A + act) * 3;
#pragma unroll
                for (int k = 0; k < 4; k++) dq[k] = dqf[k];
#pragma unroll
                for (int k = 0; k < 3; k++) dt[k] = gp_in[4 + k];
            }
            gw = dr[0]; gz = dr[3];
        } else {
            gt[0] = b.g_trans[3 * act]; gt[1] = b.g_trans[3 * act + 1]; gt[2] = b.g_trans[3 * act + 2];
            gw = b.g_rot[4 * act]; gz = b.g_rot[4 * act + 3];
        }
        // ---- heads: the products of heads_backward, STORED to the actor's slot (+0.0 where the default skips the add of a zero gradient); the
        // expressions are heads_backward's own, under the unit's default contraction as there ----
        const float dth = gw * (-oz) + gz * ow;
        const float go[8] = {gt[0], gt[1], gt[2], gt[0], gt[1], gt[2], dth, dth};
        float* slot = b.slab + (size_t)act * b.pitch;
        float dhc = 0.f, dhf = 0.f;
#pragma unroll
        for (int o = 0; o < 8; o++) {
            const bool on = go[o] != 0.f;
            if (lane < width) slot[slot_w(head_of(o), width) + head_row(o) * width + lane] = on ? go[o] * (head_coarse(o) ? hc : hf) : 0.f;
            if (lane == 0) slot[slot_b(head_of(o), width) + head_row(o)] = on ? go[o] : 0.f;
            if (head_coarse(o)) dhc += go[o] * wrow[o]; else dhf += go[o] * wrow[o];
        }
        s_dh[0][lane] = dhc; s_dh[1][lane] = dhf;
        b.dh[((size_t)act * 2 + 0) * EMD_WAVE + lane] = dhc; b.dh[((size_t)act * 2 + 1) * EMD_WAVE + lane] = dhf;
        if (lane >= dim && lane < width) {
            if (POSE) s_dmean[lane - dim] = (dhc + dhf) / cnt;
            else b.d_mean[(size_t)act * E + (lane - dim)] = dhc + dhf;
        }
    }
    __syncthreads();                                             // (also: the clears above are done)
    if ((int)threadIdx.x < 8 * dim) {
        const int q = threadIdx.x / dim, c = threadIdx.x - q * dim;
        int row_of[8]; bool valid[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const TeSample& s = u < 4 ? sc : sf;
            const int r = (u >> 1) & 1;
            row_of[u] = (u & 1) ? s.hb[r] : s.ha[r];
            valid[u] = !(r == 1 && !s.in1);
        }
        int R = 0; bool owner = false;
#pragma unroll
        for (int u = 0; u < 8; u++) if (u == q) { R = row_of[u]; owner = valid[u]; }
#pragma unroll
        for (int u = 0; u < 8; u++) if (u < q && valid[u] && row_of[u] == R) owner = false;
        if (owner) {
#pragma clang fp contract(off)
            double acc = 0.0;
            for (int j = 0; j < dim; j++) {
                const int x0 = s_x0[j];
                const bool m0 = x0 == c, m1 = s_inx1[j] && x0 + 1 == c;
                if (!m0 && !m1) continue;
                const float wx0 = s_wx0[j], wx1 = s_wx1[j];
#pragma unroll
                for (int lvl = 0; lvl < 2; lvl++) {
                    const TeSample& s = lvl ? sf : sc;
                    const float g = s_dh[lvl][j];
#include "te_gather_body.inc"
                }
            }
            G[(size_t)R * dim + c] = (float)acc;
        }
    }
    if (POSE && b.d_embeddings && E > 0) {
        const int lo = a.segment_start[act], hi = a.segment_start[act + 1];
        for (int i = (lo * E) + (int)threadIdx.x; i < hi * E; i += TRK_THREADS) b.d_embeddings[i] = s_dmean[i % E];
    }
}

// the slots of the slab, added per element in ascending actor index in fp64 from 0.0, rounded once; every destination element is written
struct SlabReduce { const float* slab; int pitch, A, width; float* dst_w[4]; float* dst_b[4]; };
__global__ void __launch_bounds__(EMD_BLOCK) k_head_slab_reduce(SlabReduce r) {
    const int e = blockIdx.x * EMD_BLOCK + threadIdx.x, w = r.width;
    if (e >= 8 * w + 8) return;
    double acc = 0.0;
    for (int a = 0; a < r.A; a++) acc += (double)r.slab[(size_t)a * r.pitch + e];
    float* dst = nullptr;
#pragma unroll
    for (int h = 0; h < 4; h++) {
        if (e >= slot_w(h, w) && e < slot_b(h, w)) dst = r.dst_w[h] + (e - slot_w(h, w));
        const int rows_h = h < 2 ? 3 : 1;
        if (e >= slot_b(h, w) && e < slot_b(h, w) + rows_h) dst = r.dst_b[h] + (e - slot_b(h, w));
    }
    *dst = (float)acc;
}

int reduce_slab(const TrackDetWs& w, int A, int width, float* const (&d_w)[4], float* const (&d_b)[4], hipStream_t st) {
    SlabReduce r;
    r.slab = w.slab; r.pitch = slab_pitch(width); r.A = A; r.width = width;
    for (int h = 0; h < 4; h++) { r.dst_w[h] = d_w[h]; r.dst_b[h] = d_b[h]; }
    hipLaunchKernelGGL(k_head_slab_reduce, dim3((unsigned)((slot_floats(width) + EMD_BLOCK - 1) / EMD_BLOCK)), dim3(EMD_BLOCK), 0, st, r);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

}  // namespace

extern "C" size_t emd_track_det_workspace_size(int32_t num_actors, int32_t head_width, int64_t num_points, int32_t row_width) {
    if (!track_det_sizes_ok(num_actors, head_width, num_points, row_width)) return 0;
    TrackDetWs w;
    carve_track_det(nullptr, num_actors, head_width, num_points, row_width, &w);
    return w.bytes;
}

extern "C" int emd_track_det_workspace_offsets(int32_t num_actors, int32_t head_width, int64_t num_points, int32_t row_width, size_t out[8]) {
    if (!out || !track_det_sizes_ok(num_actors, head_width, num_points, row_width)) {
        emd_set_error("track_det_workspace_offsets: bad argument (num_actors = %d, head_width = %d, num_points = %lld, row_width = %d)", num_actors, head_width,
                      (long long)num_points, row_width);
        return EMD_ERR_INVALID;
    }
    TrackDetWs w;
    carve_track_det(nullptr, num_actors, head_width, num_points, row_width, &w);
    const int buf = emd_det_sorted_buf(num_actors);
    out[0] = emd_det_offset(w.slab); out[1] = head_width > 0 ? (size_t)slab_pitch(head_width) : 0; out[2] = emd_det_offset(w.dh);
    out[3] = emd_det_offset(w.s.keys_in); out[4] = emd_det_offset(w.s.keys[buf]); out[5] = emd_det_offset(w.s.vals[buf]);
    out[6] = emd_det_offset(w.counts); out[7] = w.bytes;
    return EMD_OK;
}

extern "C" int emd_actor_row_sum_det(int32_t n, int32_t width, const float* rows, int32_t row_pitch, const int32_t* ids, int32_t num_actors,
                                     const int32_t* segment_start, float* out, int32_t out_pitch, void* ws, size_t ws_bytes, void* hip_stream) {
    if (n < 0 || num_actors < 0 || width < 1 || width > 64 || row_pitch < width || out_pitch < width || !emd_det_track_points_fit(n)) {
        emd_set_error("actor_row_sum_det: need 1 <= width <= 64 and width <= row_pitch, out_pitch (n %d, actors %d, width %d, pitches %d / %d)", n, num_actors, width,
                      row_pitch, out_pitch);
        return EMD_ERR_INVALID;
    }
    if (n == 0 || num_actors == 0) return EMD_OK;
    if (!rows || !out || (!ids && !segment_start)) { emd_set_error("actor_row_sum_det: null rows / ids / out pointer"); return EMD_ERR_INVALID; }
    TrackDetWs w;
    const int rc = carve_checked("actor_row_sum_det", ws, ws_bytes, num_actors, 0, n, width, &w);
    if (rc) return rc;
    return row_sum(n, width, rows, row_pitch, ids, num_actors, segment_start, out, out_pitch, w, (hipStream_t)hip_stream);
}

extern "C" int emd_track_heads_forward_det(const EmdTrackArgs* a, void* ws, size_t ws_bytes, void* hip_stream) {
    int rc = check_track(a, "track_heads_forward_det");
    if (rc || a->num_actors == 0) return rc;
    if (!a->trans || !a->rot) { emd_set_error("track_heads_forward_det: null output"); return EMD_ERR_INVALID; }
    const int E = a->embed_dim;
    // sorted ids and a narrow embedding: the default forward has no atomics (k_track_embed_sum_seg) and is used as it is
    if (!(E > 0 && a->num_points > 0) || (a->segment_start && E <= 8)) return emd_track_heads_forward(a, hip_stream);
    TrackDetWs w;
    rc = carve_checked("track_heads_forward_det", ws, ws_bytes, a->num_actors, 0, a->num_points, E, &w);
    if (rc) return rc;
    rc = row_sum(a->num_points, E, a->embeddings, E, a->point_ids, a->num_actors, a->segment_start, a->emb_sum, E, w, (hipStream_t)hip_stream);
    if (rc) return rc;
    EmdTrackArgs heads = *a;                     // the sums are there: without points the default entry launches k_track_heads<false> alone
    heads.num_points = 0;
    return emd_track_heads_forward(&heads, hip_stream);
}

extern "C" int emd_track_heads_backward_det(const EmdTrackArgs* a, const EmdTrackGrads* g, void* ws, size_t ws_bytes, void* hip_stream) {
    int rc = check_track(a, "track_heads_backward_det");
    if (rc || a->num_actors == 0) return rc;
    if (!g || !g->g_trans || !g->g_rot || !g->d_weight || !g->d_mean) { emd_set_error("track_heads_backward_det: null gradient pointer"); return EMD_ERR_INVALID; }
    for (int h = 0; h < 4; h++) if (!g->d_head_w[h] || !g->d_head_b[h]) { emd_set_error("track_heads_backward_det: null head gradient %d", h); return EMD_ERR_INVALID; }
    const int A = a->num_actors, E = a->embed_dim, width = a->dim + E;
    TrackDetWs w;
    rc = carve_checked("track_heads_backward_det", ws, ws_bytes, A, width, 0, 0, &w);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    ChainBwd b;
    memset(&b, 0, sizeof(b));
    b.p.track = *a;
    b.g_trans = g->g_trans; b.g_rot = g->g_rot; b.d_weight = g->d_weight; b.d_mean = g->d_mean;
    b.slab = w.slab; b.pitch = slab_pitch(width); b.dh = w.dh;
    hipLaunchKernelGGL(k_track_chain_bwd_det<false>, dim3(A), dim3(TRK_THREADS), 0, st, b);
    EMD_LAUNCH_CHECK();
    rc = reduce_slab(w, A, width, g->d_head_w, g->d_head_b, st);
    if (rc) return rc;
    if (g->d_embeddings && E > 0 && a->num_points > 0) {
        return emd_launch_track_embed_bwd(a->num_points, E, a->point_ids, a->count, g->d_mean, g->d_embeddings, st);
    }
    return EMD_OK;
}

extern "C" int emd_tracked_pose_backward_det(const EmdTrackedPoseArgs* p, const EmdTrackedPoseGrads* g, void* ws, size_t ws_bytes, void* hip_stream) {
    int rc = check_tracked(p, "tracked_pose_backward_det");
    if (rc || p->track.num_actors == 0) return rc;
    if (!g || !g->g_pose || !g->d_q_all || !g->d_t_all || !g->d_weight) { emd_set_error("tracked_pose_backward_det: null gradient pointer"); return EMD_ERR_INVALID; }
    for (int h = 0; h < 4; h++) if (!g->d_head_w[h] || !g->d_head_b[h]) { emd_set_error("tracked_pose_backward_det: null head gradient %d", h); return EMD_ERR_INVALID; }
    const int A = p->track.num_actors, width = p->track.dim + p->track.embed_dim;
    TrackDetWs w;
    rc = carve_checked("tracked_pose_backward_det", ws, ws_bytes, A, width, 0, 0, &w);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    ChainBwd b;
    memset(&b, 0, sizeof(b));
    b.p = *p;
    b.g_pose = g->g_pose; b.d_q_all = g->d_q_all; b.d_t_all = g->d_t_all; b.d_weight = g->d_weight; b.d_embeddings = g->d_embeddings;
    b.slab = w.slab; b.pitch = slab_pitch(width); b.dh = w.dh;
    hipLaunchKernelGGL(k_track_chain_bwd_det<true>, dim3(A), dim3(TRK_THREADS), 0, st, b);
    EMD_LAUNCH_CHECK();
    return reduce_slab(w, A, width, g->d_head_w, g->d_head_b, st);
}
