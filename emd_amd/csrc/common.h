// common.h -- shared host/device definitions of the gfx950 street-Gaussian rasterizer.
// Wave = 64 lanes, 256-thread workgroups, 16x16 tiles.  No CUDA compatibility layer: HIP for CDNA4 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <type_traits>

#include "../../include/emd_raster.h"

#define EMD_WAVE 64
#define EMD_BLOCK 256
#define EMD_NUM_TILE_PIX (EMD_TILE_X * EMD_TILE_Y)

// Per-Gaussian projected record: 4 x float4 = 64 B, one half cache line, gathered by the render kernels.
//   r0 = (x_pix, y_pix, depth, opacity)   r1 = (conic A, B, C, bits)   r2 = (r, g, b, 0)   r3 = (nx, ny, nz, 0)
// r1.w bits: 0..2 = SH colour channel clamped (zero gradient).
#define EMD_REC_F4 4

// Per-Gaussian gradient accumulator written by the render backward: 12 payload floats = 48 B (3 x float4)
//   [0..1] d/d mean2D (pixel units)  [2] d/d depth  [3] d/d opacity
//   [4..6] d/d conic (A,B,C)         [7..9] d/d rgb
//   [10..11] sum |d/d mean2D| (EMD_FLAG_ABSGRAD)
// followed by (r, g, b, -) per extra colour set.  The row PITCH (emd_bwd_stride below) is the payload rounded up to whole 64-byte lines.
#define EMD_BWD_PAYLOAD 12
#define EMD_BWD_PITCH_ALIGN 16          // floats: a row starts on a 64-byte line and covers whole lines

struct GeomWs {
    float4* rec;             // [N][4]
    float4* shjac;           // [N][3] d rgb_c / d (unit view direction): row c = (d/dx, d/dy, d/dz, -); written by K1 for
                             // visible Gaussians so that K8 need not re-read the 192 B of SH coefficients
    uint2* binrec;           // [N] by Gaussian id (K1): x = ENUMERATED tile rectangle x0 | y0 << 10 | width << 20 (upstream's rectangle cut down to the
                             //   alpha >= 1/255 box) | skip-left / skip-right << 30, y = its height | skip-top / skip-bottom << 10 | upstream's tiles
                             //   touched << 12.  A skip bit: the outer quadrant column / row of the rectangle's first / last tile lies outside the box
    uint32_t* depth_key;     // [N] by Gaussian id: float bits of the view depth, 0xFFFFFFFF when not visible (K1)
    uint32_t* gkeys[2];      // [N] ping-pong of the Gaussian depth sort
    uint32_t* gvals[2];      // [N] Gaussian ids in depth order after the sort (in the pair the sort's launcher returns)
    uint2* bin_s;            // [N] the same records in depth order
    uint32_t* ghist;         // radix histograms of the depth sort [bins][ceil(N / sort tile)]
    uint32_t* block_sums;    // [ceil(N/256)] pairs emitted per block of 256 depth-ordered Gaussians (added up by the last depth pass)
    uint32_t* contrib;       // [N] by Gaussian id: 0 from K1; 1 once the render backward has staged a row with a non-zero float for the Gaussian, i.e. has
                             //   added to its accumulator row.  What K8 takes for "visible" (not under EMD_FLAG_DETERMINISTIC, whose K7 does not write it)
    size_t bytes;
};

struct BinWs {
    uint32_t* tkeys[2];      // [capacity] ping-pong: tile id of every (tile, Gaussian) pair
    uint32_t* vals[2];       // [capacity] list word: Gaussian id | quadrant mask of the pair << 28 (footprint.h)
    uint32_t* ranges;        // [T][2]
    uint32_t* tile_order;    // [T] tile ids by descending list length: dispatch order of the render kernels
    uint32_t* hist;          // radix histograms [bins][num_sort_blocks]
    uint32_t* surv;          // [4 * capacity] per (tile, quadrant): the Gaussian ids of the list entries whose footprint reaches the quadrant, in
                             //   list order, written by the render forward for the render backward (at 4 * range start + quadrant * list length)
    uint32_t* quad_need;     // [4 * T] how many of them lie in front of the quadrant's deepest contributor (what the backward walks)
    int sorted_buf;          // which ping-pong buffer holds the sorted list after forward: emd_radix_result_buf of the tile sort
    size_t bytes;
};

struct ImgWs {
    float* final_T;          // [H*W]
    uint32_t* n_contrib;     // [H*W]
    size_t bytes;
};

static inline size_t emd_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// sort geometry
#define EMD_SORT_ITEMS 8                        // keys per thread
#define EMD_SORT_TILE (EMD_BLOCK * EMD_SORT_ITEMS)
#define EMD_RADIX_BITS 8
#define EMD_RADIX_BINS (1 << EMD_RADIX_BITS)

static inline int emd_tile_bits(int num_tiles) {
    int b = 0;
    while ((1 << b) < num_tiles) b++;
    return b;
}
// Upstream key = tile_id << 32 | depth bits.  Sorted here as radix passes over the depth bits of the visible Gaussians,
// then ceil(tile bits / 8) passes of equal width over the tile ids of the duplicates (binning.hip).
// Depth bits: a visible Gaussian lies beyond the near plane, and positive floats order like their bit patterns, so the sort runs on
// (bits - bits(near plane)), which fits 27 bits for depths up to 65 536 x the near plane (13 km at 0.2 m): three passes of
// nine bits.  A key outside that range raises bit 1 of EmdStatus.overflow and the caller repeats the call with
// EMD_FLAG_WIDE_DEPTH_SORT: four passes of eight bits over all 32.
#define EMD_DEPTH_BITS_NARROW 9
#define EMD_DEPTH_PASSES_NARROW 3
#define EMD_DEPTH_RANGE_NARROW (EMD_DEPTH_BITS_NARROW * EMD_DEPTH_PASSES_NARROW)
#define EMD_DEPTH_PASSES_WIDE (32 / EMD_RADIX_BITS)
#define EMD_DEPTH_BINS_MAX (1 << EMD_DEPTH_BITS_NARROW)
static inline int emd_tile_passes(int num_tiles) { return (emd_tile_bits(num_tiles) + EMD_RADIX_BITS - 1) / EMD_RADIX_BITS; }
static inline int emd_tile_pass_bits(int num_tiles) {
    const int p = emd_tile_passes(num_tiles);
    return p ? (emd_tile_bits(num_tiles) + p - 1) / p : 0;
}
// Which pair of a sort's ping-pong buffers holds the pairs after `passes` passes (radix_sort.h).  Pass 0 of a compacting sort reads the raw keys
// and writes pair 0; every other pass writes the pair it did not read, starting from pair 0.  The sort's launcher picks the buffers of every pass
// with this function and returns its value; BinWs::sorted_buf below is the same function of the tile sort's pass count.
static inline int emd_radix_result_buf(bool compacting, int passes) { return passes < 1 ? 0 : (passes - (compacting ? 1 : 0)) & 1; }

static inline void emd_carve_geom(void* base, int N, GeomWs* w) {
    char* p = (char*)base;
    size_t off = 0;
    const size_t n = (size_t)(N > 0 ? N : 1);
    w->rec = (float4*)(p + off); off = emd_align_up(off + n * EMD_REC_F4 * sizeof(float4), 256);
    w->shjac = (float4*)(p + off); off = emd_align_up(off + n * 3 * sizeof(float4), 256);
    w->binrec = (uint2*)(p + off); off = emd_align_up(off + n * 8, 256);
    w->depth_key = (uint32_t*)(p + off); off = emd_align_up(off + n * 4, 256);
    for (int i = 0; i < 2; i++) { w->gkeys[i] = (uint32_t*)(p + off); off = emd_align_up(off + n * 4, 256); }
    for (int i = 0; i < 2; i++) { w->gvals[i] = (uint32_t*)(p + off); off = emd_align_up(off + n * 4, 256); }
    w->bin_s = (uint2*)(p + off); off = emd_align_up(off + n * 8, 256);
    size_t nsb = (n + EMD_SORT_TILE - 1) / EMD_SORT_TILE;
    w->ghist = (uint32_t*)(p + off); off = emd_align_up(off + nsb * EMD_DEPTH_BINS_MAX * 4, 256);
    size_t nb = (n + EMD_BLOCK - 1) / EMD_BLOCK;
    w->block_sums = (uint32_t*)(p + off); off = emd_align_up(off + (nb + 8) * 4, 256);
    w->contrib = (uint32_t*)(p + off); off = emd_align_up(off + n * 4, 256);
    w->bytes = off + 256;
}

static inline void emd_carve_bin(void* base, int64_t capacity, int num_tiles, BinWs* w) {
    char* p = (char*)base;
    size_t off = 0;
    size_t cap = (size_t)(capacity > 0 ? capacity : 1);
    for (int i = 0; i < 2; i++) { w->tkeys[i] = (uint32_t*)(p + off); off = emd_align_up(off + cap * 4, 256); }
    for (int i = 0; i < 2; i++) { w->vals[i] = (uint32_t*)(p + off); off = emd_align_up(off + cap * 4, 256); }
    w->ranges = (uint32_t*)(p + off); off = emd_align_up(off + (size_t)num_tiles * 8, 256);
    w->tile_order = (uint32_t*)(p + off); off = emd_align_up(off + (size_t)num_tiles * 4, 256);
    size_t nsb = (cap + EMD_SORT_TILE - 1) / EMD_SORT_TILE;
    w->hist = (uint32_t*)(p + off); off = emd_align_up(off + nsb * EMD_RADIX_BINS * 4, 256);
    w->surv = (uint32_t*)(p + off); off = emd_align_up(off + cap * 16, 256);
    w->quad_need = (uint32_t*)(p + off); off = emd_align_up(off + (size_t)num_tiles * 16, 256);
    w->sorted_buf = emd_radix_result_buf(false, emd_tile_passes(num_tiles));
    w->bytes = off + 256;
}

static inline void emd_carve_img(void* base, int H, int W, ImgWs* w) {
    char* p = (char*)base;
    size_t off = 0, hw = (size_t)H * W;
    w->final_T = (float*)(p + off); off = emd_align_up(off + hw * 4, 256);
    w->n_contrib = (uint32_t*)(p + off); off = emd_align_up(off + hw * 4, 256);
    w->bytes = off + 256;
}

// ---- error plumbing (api.hip) -------------------------------------------------------------------
void emd_set_error(const char* fmt, ...);
#define EMD_HIP_CHECK(expr)                                                                          \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess) {                                                                      \
            emd_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return EMD_ERR_HIP;                                                                      \
        }                                                                                            \
    } while (0)
#define EMD_LAUNCH_CHECK() EMD_HIP_CHECK(hipGetLastError())

// Runtime flags -> template arguments (host code): f is called with a std::integral_constant of the value and its result is returned, so a launcher
// nests these around one generic lambda that names the kernel.  with_int serves LO .. HI: values at or below LO take LO, at or above HI take HI.
template <class F> static auto with_bool(bool b, F&& f) {
    if (b) return f(std::true_type{});
    else return f(std::false_type{});
}
template <int LO, int HI, class F> static auto with_int(int v, F&& f) {
    if constexpr (LO == HI) return f(std::integral_constant<int, LO>{});
    else if (v <= LO) return f(std::integral_constant<int, LO>{});
    else return with_int<LO + 1, HI>(v, f);
}

// Zero `bytes` (a multiple of 4, `p` 4-byte aligned) with a KERNEL on `st` (api.hip).  Not hipMemsetAsync: a memset node captured into a
// hipGraph on ROCm 7.2 / gfx950 replays with a corrupt 16-byte fill pattern from the second replay on (every fourth word of the
// destination came back as garbage: tests/test_boundary_gpu.py's graph test caught it), and a kernel node costs the same.
int emd_zero_async(void* p, size_t bytes, hipStream_t st);

// ---- per-stage HIP-event timing (api.hip); no-ops unless emd_profile_enable(1) ------------------------------
enum { PROF_PREPROCESS = 0, PROF_DUPLICATE, PROF_SORT, PROF_RANGES, PROF_RENDER_FWD, PROF_RENDER_BWD, PROF_PREPROCESS_BWD, PROF_OTHER };
void emd_prof_begin(int stage, hipStream_t st);
void emd_prof_end(int stage, hipStream_t st);
void emd_prof_switch(int ended, int started, hipStream_t st);   // one event closes `ended` and opens `started`

// ---- stage launchers (one per translation unit) -------------------------------------------------
struct PreArgs {
    EmdSettings s;
    int N, M, flags;
    const float *means3D, *shs, *colors_precomp, *opacities, *scales, *rotations, *cov3D_precomp;
    EmdMotion motion;
    int32_t* radii;
    GeomWs g;
    EmdStatus* status;
    const float* sdev;       // device copy of bg / viewmatrix / projmatrix / campos (EmdFwdArgs.settings_dev) or null
    const float *shs_res0, *shs_res1;   // optional residuals of the SH coefficients (EmdFwdArgs.shs_residual) or null
};
int emd_launch_preprocess(const PreArgs& a, int part, hipStream_t st);       // preprocess.hip; part 0 = whole kernel, 1 = geometry half, 2 = colour half
int emd_launch_binning(const EmdSettings& s, int flags, int N, const GeomWs& g, const BinWs& b, int64_t capacity, EmdStatus* status,
                       hipStream_t st);                                       // binning.hip
int emd_launch_export_keys(int64_t D, const GeomWs& g, const BinWs& b, uint64_t* keys, uint32_t* ids, uint32_t* quad_masks, hipStream_t st);  // binning.hip
// extra colour sets composited by the same list walk as the main colours (EmdFwdArgs.colors_extra ...)
struct EmdExtra {
    int num;
    const float* colors[EMD_MAX_EXTRA];    // [N,3]
    float* out[EMD_MAX_EXTRA];             // [3,H,W]
    const float* dL_dout[EMD_MAX_EXTRA];   // [3,H,W] or null (backward)
};
// pitch in floats of an accumulator row of the render backward: EMD_BWD_PAYLOAD floats + (r, g, b, -) per extra colour set, rounded up to whole
// 64-byte lines (16, 16, 32 floats for 0, 1, 2 extra sets).  A device-scope float atomic is performed line by line on the memory side: a row that
// starts on a line costs one request where a 48-byte pitch cost 1.5 on average.  Nobody writes the pad floats: a clean workspace stays clean.
__host__ __device__ constexpr int emd_bwd_stride(int num_extra) {
    return (EMD_BWD_PAYLOAD + 4 * num_extra + EMD_BWD_PITCH_ALIGN - 1) / EMD_BWD_PITCH_ALIGN * EMD_BWD_PITCH_ALIGN;
}
// bytes of the accumulator rows of N Gaussians (EmdBwdArgs.bwd_ws; one row when N = 0, as the other workspaces keep one element)
static inline size_t emd_bwd_bytes(int N, int num_extra) { return (size_t)(N > 0 ? N : 1) * emd_bwd_stride(num_extra) * sizeof(float); }
int emd_launch_render_forward(const EmdSettings& s, const float* sdev, int flags, const GeomWs& g, const BinWs& b, const ImgWs& im,
                              float* out_color, float* out_depth, float* out_normal, float* out_alpha, const EmdExtra* x,
                              unsigned long long* loop_stats, hipStream_t st);   // render.hip
int emd_launch_render_backward(const EmdSettings& s, const float* sdev, int flags, const GeomWs& g, const BinWs& b, const ImgWs& im,
                               const float* out_color, const float* out_depth, const float* out_normal,
                               const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                               const float* dL_dnormal, const EmdExtra* x, float* grad_rec, float* zero_buf, int zero_n,
                               float4* fill_base, size_t fill_n,
                               unsigned long long* pair_stats, float* det_part, hipStream_t st);  // render.hip (zero_buf: small table cleared by block 0
                               // for K8; fill_base / fill_n: null / 0, or fill_n float4 the kernel's workgroups zero, a slice each (emd_fill_slice) -- the dense
                               // dL/dshs rows, of which K8 then stores the contributing ones only; ignored by the deterministic variant;
                               // det_part: null, or the deterministic variant -- every row STORED to its survivor's slot there, grad_rec untouched)
// The slice [lo, hi) of `count` float4 that workgroup `block` of `grid` zeroes for the kernel behind it: per = ceil(count / grid) elements rounded up
// to whole 64-lane store instructions (1 KB contiguous each), so the slices are disjoint, ascending and cover [0, count) exactly; the workgroups past
// the end (count < 64 grid leaves most of them without work) get lo == hi == count.  64-bit: count = 12 N passes 2^32 at N = 358 M.  The launcher forms
// `per` once (a 64-bit division is a loop of some hundred instructions on the device) and the kernel's workgroups take their slice from it.
__host__ __device__ inline uint64_t emd_fill_per(uint64_t count, uint32_t grid) {
    const uint64_t g = grid ? grid : 1u;
    return ((count + g - 1) / g + 63u) & ~(uint64_t)63u;
}
__host__ __device__ inline void emd_fill_slice(uint64_t count, uint64_t per, uint32_t block, uint64_t* lo, uint64_t* hi) {
    const uint64_t a = (uint64_t)block * per;
    *lo = a < count ? a : count;
    *hi = count - *lo < per ? count : *lo + per;
}
// EMD_FLAG_DETERMINISTIC: keys_in[slot] = Gaussian id of the survivor that owns contribution slot `slot` (below 4 D; 0xFFFFFFFF for the survivors
// the render backward does not walk), *count = 4 D                                                                                     // render.hip
int emd_launch_det_render_keys(int num_tiles, const BinWs& b, const EmdStatus* status, uint32_t* keys_in, uint32_t* count, hipStream_t st);
// ... and keys_in[i] = actor id of point i when it is visible and bound to an actor, else 0xFFFFFFFF                                   // preprocess.hip
int emd_launch_det_pose_keys(int N, const int32_t* radii, const int32_t* actor_id, uint32_t* keys_in, hipStream_t st);
struct PreBwdArgs {
    EmdSettings s;
    int N, M, flags;
    const float *means3D, *shs, *colors_precomp, *opacities, *scales, *rotations, *cov3D_precomp;
    EmdMotion motion;
    const int32_t* radii;
    GeomWs g;
    float* grad_rec;        // [N][bwd_stride]; read, and its payload cleared row by row under EMD_FLAG_BWD_WS_CLEAN
    int bwd_stride, num_extra;
    float* dL_dextra[EMD_MAX_EXTRA];   // [N,3] gradient of every extra colour set
    float *dL_dmeans3D, *dL_dmeans2D, *dL_dmeans2D_abs, *dL_dshs, *dL_dcolors, *dL_dopacities, *dL_dscales,
        *dL_drotations, *dL_dcov3D, *dL_dactor_pose, *dL_dresidual_dx, *dL_dresidual_dq, *dL_dsh_color;
    const float* sdev;
    int shs_prezeroed;      // 1: the render backward of this call zeroed every dL/dshs row (emd_launch_render_backward's fill): the staged path stores the
                            // 16-byte pieces of the compacted Gaussians' rows only.  0: every row is written here
    float* pose_rows;       // EMD_FLAG_DETERMINISTIC: [N][EMD_ACTOR_STRIDE], the pose gradient of every visible actor-bound point is STORED here instead of
                            // being added to dL_dactor_pose with atomics (api.hip sorts the points by actor and sums the rows: segsum.h); else null
};

// Camera-dependent settings from their device copy (uniform scalar loads), replacing the by-value fields.
__device__ __forceinline__ void emd_settings_from_device(EmdSettings& S, const float* __restrict__ sdev, int flags) {
    if (!sdev) return;
    if (flags & EMD_FLAG_SDEV_TANFOV) { S.tanfovx = sdev[38]; S.tanfovy = sdev[39]; }
#pragma unroll
    for (int k = 0; k < 3; k++) S.bg[k] = sdev[k];
#pragma unroll
    for (int k = 0; k < 16; k++) { S.viewmatrix[k] = sdev[3 + k]; S.projmatrix[k] = sdev[19 + k]; }
#pragma unroll
    for (int k = 0; k < 3; k++) S.campos[k] = sdev[35 + k];
}
// The per-Gaussian words the projection backward and its siblings (k_sh_factor, the camera gradient) test with `> 0` for "this Gaussian has a gradient
// row": the contributed words K7 set, or the radii under EMD_FLAG_DETERMINISTIC (the pose rows and their sort keys there are keyed by the radii, and the
// deterministic K7 does not write the words).  Kernel-uniform, so the load behind it stays unconditional.
__host__ __device__ inline const int32_t* emd_bwd_visible_words(int flags, const int32_t* radii, const GeomWs& g) {
    return (flags & EMD_FLAG_DETERMINISTIC) ? radii : reinterpret_cast<const int32_t*>(g.contrib);
}
int emd_launch_preprocess_backward(const PreBwdArgs& a, hipStream_t st);     // preprocess.hip
// the clamp-masked colour gradient of every Gaussian (the factor of its rank-one dL/dshs) from the render backward's accumulator rows
// (`radii`: the words of emd_bwd_visible_words, declared above the projection backward's launcher -- a row is read where its word is > 0)
int emd_launch_sh_factor(int N, const int32_t* radii, const GeomWs& g, const float* grad_rec, int bwd_stride, float* dL_dsh_color, hipStream_t st);
// camera_grad.hip: dL/d(viewmatrix, projmatrix, campos) from the accumulator rows K7 left (read, not cleared), between the two halves of the
// backward.  `partials`: emd_camera_grad_bytes(N) bytes, 16-byte aligned, one 36-float row per workgroup; every one of the 35 outputs is written.
size_t emd_camera_grad_rows(int N);
size_t emd_camera_grad_bytes(int N);
int emd_launch_camera_backward(const PreBwdArgs& a, float* partials, float* dL_dcamera, hipStream_t st);

// ---- launchers behind the stand-alone entry points of api.hip ----------------------------------------------------------------------------
int emd_launch_export_geometry(int N, const GeomWs& g, float* means2D, float* depths, float* conic_opacity, float* rgb,
                               float* normal, uint32_t* tiles_touched, hipStream_t st);                                                  // preprocess.hip
// standalone_ops.hip
int emd_launch_abs_mean_backward(size_t n, const float* x, const float* g, float* out, hipStream_t st);
int emd_launch_residual_l1_backward(size_t n, const float* up_a, const float* up_b, const float* x_a, const float* x_b, const float* g_a,
                                    const float* g_b, float* out_a, float* out_b, hipStream_t st);
int emd_launch_motion_forward(int n, const float* means, const float* quats, const float* opac, const EmdMotion& mo,
                              float* wm, float* wq, float* wo, hipStream_t st);
int emd_launch_motion_backward(int n, const float* means, const float* quats, const float* opac, const EmdMotion& mo,
                               const float* g_wm, const float* g_wq, const float* g_wo, float* d_means, float* d_quats,
                               float* d_opac, float* d_pose, float* d_rdx, float* d_rdq, hipStream_t st);
// the deterministic form: the pose rows of the bound points and their actors as keys instead of atomics on d_pose (pose_rows == NULL: none asked for)
int emd_launch_motion_backward_det(int n, const float* means, const float* quats, const float* opac, const EmdMotion& mo,
                                   const float* g_wm, const float* g_wq, const float* g_wo, float* d_means, float* d_quats,
                                   float* d_opac, float* d_rdx, float* d_rdq, float* pose_rows, uint32_t* keys_in, hipStream_t st);
int emd_launch_sh_forward(int n, int deg, int M, const float* dirs, const float* coeffs, float* rgb, hipStream_t st);
int emd_launch_sh_backward(int n, int deg, int M, const float* dirs, const float* coeffs, const float* g_rgb,
                           float* d_coeffs, float* d_dirs, hipStream_t st);
int emd_launch_sh_grad_from_factors(int n, int V, int deg, int M, const float* means, const EmdMotion& mo, int pose_per_view,
                                    const float* campos, const float* gc, float scale, float* d_shs, hipStream_t st);
int emd_launch_densification_stats(int n, const int32_t* radii, const float* g2d, float* accum, float* denom, float* max_radii,
                                   hipStream_t st);
int emd_launch_actor_pose_forward(int A, const float* q, const float* t, const uint8_t* valid, const float* dt, const float* dq,
                                  float* pose, const int32_t* frame_dev, hipStream_t st);
int emd_launch_actor_pose_backward(int A, const float* q, const float* dt, const float* dq, const float* g_pose, float* d_q,
                                   float* d_t, float* d_dt, float* d_dq, const int32_t* frame_dev, hipStream_t st);
int emd_launch_l1_loss(size_t n, const float* a, const float* b, float* loss, float* grad, uint32_t* scratch, hipStream_t st);
int emd_launch_activations(int n, const float* ls, float* sc, const float* rq, float* q, const float* lo, float* o, hipStream_t st);
