// densify.hip -- adaptive density control on the SoA parameter + Adam-state buffers, on the device.
//
//   densify  = densify_and_clone + densify_and_split        S3Gaussian/scene/gaussian_model.py:515-603,696-701
//   prune    = prune / prune_points                          S3Gaussian/scene/gaussian_model.py:441-479,683-695
//   (OmniRe's per-class version of the same logic: models/gaussians/vanilla.py:206-376)
//
// The reference performs each of them with boolean-mask indexing (a device-to-host sync per mask), `torch.cat` / `repeat` on
// every parameter and both Adam moments (~60 launches and as many temporaries), and draws the split samples from the global
// CUDA generator (`torch.normal`, gaussian_model.py:543) -- a different stream on every rank.  Here one event is
//   k_densify_decide   one pass over the N Gaussians: per point a code (keep / clone / split / drop) from the accumulated
//                      statistics, the activated scale and opacity; per 256-point block the number of survivors / clones / splits
//   k_densify_scan     exclusive prefix sums of the block counts (one workgroup per column) + the column totals
//                      [ONE host read: the totals = the new point count.  Round 6: the scan used to be torch.cumsum over [3, N] -- three rows
//                       of 3 M elements, i.e. three workgroups: 7.3 ms of the event's 8.2 at 3 M Gaussians, profiles/r06_density_event.txt]
//   k_densify_index    for every OUTPUT row its source row and kind (position = block offset + ballot prefix), in the reference's order:
//                      survivors (in order), clones (in order), split samples replica 0 (in order), replica 1 (in order)
//   k_densify_gather   one launch for ALL tensors (7 parameters + 14 Adam moments + statistics) and ONE rule for both projects' events:
//                      output row <- source row; the moments and statistics of new rows are zero (a densification zeroes the statistics
//                      of every row); split samples get xyz = R(q) (std * n) + xyz with n ~ N(0, 1) from Philox4x32-10 keyed by
//                      (seed, SOURCE Gaussian index, replica) -- identical on every rank without communication; a reduced row gets
//                      scaling = log(exp(s) / 1.6)  (= 0.8 * 2 in float).  OmniRe's refinement (EMD_DENSIFY_MODE_REFINE) differs only in
//                      WHICH rows are reduced: every copy of a split source (kind + 16), the original included.
// HBM-bound: every surviving byte is read and written once.
#include <string.h>

#include "common.h"
#include "device_utils.h"
#include "radix_sort.h"

namespace {

enum { CODE_KEEP = 1, CODE_CLONE = 2, CODE_SPLIT = 4 };

// ---- 0/1 columns of a 256-thread block: counts per block (decide), exclusive position inside the block (index) --------------------------------
// Every thread of the block calls these (threads past the end with all flags false).
template <int NC>
__device__ __forceinline__ void block_flag_counts(const bool (&f)[NC], int32_t* __restrict__ counts, int nblocks) {
    __shared__ uint32_t s_cnt[NC][EMD_BLOCK / EMD_WAVE];
    const int wave = threadIdx.x / EMD_WAVE, lane = threadIdx.x % EMD_WAVE;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const unsigned long long b = __ballot(f[c]);
        if (lane == 0) s_cnt[c][wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (threadIdx.x < NC) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < EMD_BLOCK / EMD_WAVE; w++) t += s_cnt[threadIdx.x][w];
        counts[(size_t)threadIdx.x * nblocks + blockIdx.x] = (int32_t)t;
    }
}
// position of the thread's 1 among the 1s of its column = block offset + 1s of the waves before + 1s of the lanes before
template <int NC>
__device__ __forceinline__ void block_flag_positions(const bool (&f)[NC], const int32_t* __restrict__ offsets, int nblocks, int (&pos)[NC]) {
    __shared__ uint32_t s_cnt[NC][EMD_BLOCK / EMD_WAVE];
    const int wave = threadIdx.x / EMD_WAVE, lane = threadIdx.x % EMD_WAVE;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int in_wave[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const unsigned long long b = __ballot(f[c]);
        in_wave[c] = __popcll(b & lt);
        if (lane == 0) s_cnt[c][wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NC; c++) {
        int before = offsets[(size_t)c * nblocks + blockIdx.x];
        for (int w = 0; w < wave; w++) before += (int)s_cnt[c][w];
        pos[c] = before + in_wave[c];
    }
}

// exclusive prefix sums over the blocks, in place; one 1024-thread workgroup per column; totals[c] = the column's sum
__global__ void __launch_bounds__(1024) k_densify_scan(int nblocks, int32_t* __restrict__ counts, int32_t* __restrict__ totals) {
    __shared__ int32_t s_wave[16];
    __shared__ int32_t s_carry;
    int32_t* col = counts + (size_t)blockIdx.x * nblocks;
    const int lane = threadIdx.x % EMD_WAVE, wave = threadIdx.x / EMD_WAVE;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < nblocks; base += 1024) {
        const int i = base + (int)threadIdx.x;
        const int32_t v = i < nblocks ? col[i] : 0;
        int32_t x = v;                                  // inclusive scan inside the wave
#pragma unroll
        for (int off = 1; off < EMD_WAVE; off <<= 1) { const int32_t y = __shfl_up(x, off); if (lane >= off) x += y; }
        if (lane == EMD_WAVE - 1) s_wave[wave] = x;
        __syncthreads();
        int32_t before = s_carry;
        for (int w = 0; w < wave; w++) before += s_wave[w];
        if (i < nblocks) col[i] = before + x - v;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = before + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = s_carry;
}

__global__ void __launch_bounds__(EMD_BLOCK) k_densify_decide(EmdDensifyArgs a, int32_t* __restrict__ code, int32_t* __restrict__ counts /*[3][nblocks]*/) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    const bool live = i < a.num_points;
    int c = 0;
    if (live) {
    const float s0 = expf(a.scaling[3 * i]), s1 = expf(a.scaling[3 * i + 1]), s2 = expf(a.scaling[3 * i + 2]);
    const float smax = fmaxf(s0, fmaxf(s1, s2));
    c = CODE_KEEP;
    if (a.mode == EMD_DENSIFY_MODE_DENSIFY) {
        // grads = xyz_gradient_accum / denom, NaN -> 0 (gaussian_model.py:697-698); clone: small Gaussians, split: large ones
        float g = a.grad_accum[i] / a.denom[i];
        if (g != g) g = 0.f;
        const bool hot = g >= a.grad_threshold;                       // (torch.norm of the [N,1] column = |g|; g >= 0)
        const bool small_ = smax <= a.size_threshold;                     // the host's product, rounded once (EmdDensifyArgs)
        if (hot && small_) c |= CODE_CLONE;
        if (hot && !small_) c = CODE_SPLIT;                           // the original is removed after its two samples are appended
    } else {
        // prune (gaussian_model.py:683-692): opacity below the threshold, or -- once max_screen_size is set -- too large on screen or in
        // the world
        const float op = 1.f / (1.f + expf(-a.opacity[i]));
        bool drop = op < a.min_opacity;
        if (a.max_screen_size > 0.f) drop = drop || a.max_radii2D[i] > a.max_screen_size || smax > a.size_threshold;
        if (a.extra_drop && a.extra_drop[i]) drop = true;
        if (drop) c = 0;
    }
    code[i] = c;
    }
    const bool f[3] = {(c & CODE_KEEP) != 0, (c & CODE_CLONE) != 0, (c & CODE_SPLIT) != 0};
    block_flag_counts<3>(f, counts, (int)gridDim.x);
}

// offsets: exclusive prefix sums of the block counts (k_densify_scan); totals: the three column sums
__global__ void __launch_bounds__(EMD_BLOCK) k_densify_index(int n, const int32_t* __restrict__ code, const int32_t* __restrict__ offsets,
                                                             const int32_t* __restrict__ totals, int32_t* __restrict__ src, int32_t* __restrict__ kind) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    const int c = i < n ? code[i] : 0;
    const bool f[3] = {(c & CODE_KEEP) != 0, (c & CODE_CLONE) != 0, (c & CODE_SPLIT) != 0};
    int pos[3];
    block_flag_positions<3>(f, offsets, (int)gridDim.x, pos);
    const int n_keep = totals[0], n_clone = totals[1], n_split = totals[2];
    if (c & CODE_KEEP) { const int j = pos[0]; src[j] = i; kind[j] = 0; }
    if (c & CODE_CLONE) { const int j = n_keep + pos[1]; src[j] = i; kind[j] = 1; }
    if (c & CODE_SPLIT) {
        const int j0 = n_keep + n_clone + pos[2], j1 = j0 + n_split;
        src[j0] = i; kind[j0] = 2;
        src[j1] = i; kind[j1] = 3;
    }
}

// Philox4x32-10 (Salmon et al., SC'11): counter = (gaussian index, replica, 0, 0), key = (seed lo, seed hi)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    uint32_t c[4] = {c0, c1, 0u, 0u};
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}

// three standard normals of (seed, index, replica): Box-Muller on uniforms in (0, 1]
__device__ __forceinline__ void normal3(uint64_t seed, uint32_t index, uint32_t rep, float n[3]) {
    uint32_t r[4];
    philox4x32_10(index, rep, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const float u0 = ((float)(r[0] >> 8) + 1.f) * (1.f / 16777216.f), u1 = (float)(r[1] >> 8) * (1.f / 16777216.f);
    const float u2 = ((float)(r[2] >> 8) + 1.f) * (1.f / 16777216.f), u3 = (float)(r[3] >> 8) * (1.f / 16777216.f);
    const float ra = sqrtf(-2.f * logf(u0)), rb = sqrtf(-2.f * logf(u2));
    n[0] = ra * cosf(6.28318530717958648f * u1);
    n[1] = ra * sinf(6.28318530717958648f * u1);
    n[2] = rb * cosf(6.28318530717958648f * u3);
}

// One coordinate of a split sample: new_xyz = R(q) (std * n) + xyz with q normalised as build_rotation does (general_utils.py:245-266;
// vanilla.py:328-343), std = exp() of the source row's scale BEFORE the reduction, n the recorded draw or Philox of (seed, source row, replica)
__device__ __forceinline__ float split_sample_coord(const EmdDensifyGather& g, int i, int rep, int j, int c, float v) {
    float n[3];
    if (g.samples) { const float* s = g.samples + ((size_t)rep * g.num_split + g.split_rank[j]) * 3; n[0] = s[0]; n[1] = s[1]; n[2] = s[2]; }
    else normal3(g.seed, (uint32_t)i, (uint32_t)rep, n);
    const float* sc = g.scaling + 3 * (size_t)i;
    const float* qq = g.rotation + 4 * (size_t)i;
    const float e0 = expf(sc[0]) * n[0], e1 = expf(sc[1]) * n[1], e2 = expf(sc[2]) * n[2];
    const float qn = sqrtf(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3]);
    const float r = qq[0] / qn, x = qq[1] / qn, y = qq[2] / qn, z = qq[3] / qn;
    float R0, R1, R2;
    if (c == 0) { R0 = 1.f - 2.f * (y * y + z * z); R1 = 2.f * (x * y - r * z); R2 = 2.f * (x * z + r * y); }
    else if (c == 1) { R0 = 2.f * (x * y + r * z); R1 = 1.f - 2.f * (x * x + z * z); R2 = 2.f * (y * z - r * x); }
    else { R0 = 2.f * (x * z - r * y); R1 = 2.f * (y * z + r * x); R2 = 1.f - 2.f * (x * x + y * y); }
    return ((R0 * e0 + R1 * e1) + R2 * e2) + v;
}

// One launch for all tensors: blockIdx.y = tensor, grid-stride over its output elements.  kind & 15: 0 a surviving source row, 1 its copy (clone /
// duplicate), 2 + r split sample of replica r.  A row's scale is reduced where kind carries + 16 (REFINE: the source was split -- original,
// samples and duplicate alike, vanilla.py:337-345) and, in the other two modes, on the samples (the split original is not an output row).
__global__ void __launch_bounds__(EMD_BLOCK) k_densify_gather(EmdDensifyGather g) {
    const EmdDensifyTensor t = g.tensors[blockIdx.y];
    const size_t total = (size_t)g.num_out * t.width;
    for (size_t idx = (size_t)blockIdx.x * EMD_BLOCK + threadIdx.x; idx < total; idx += (size_t)gridDim.x * EMD_BLOCK) {
        const int j = (int)(idx / t.width), c = (int)(idx % t.width);
        const int i = g.src[j], kd = g.kind[j], base = kd & 15;
        const bool fresh = base != 0, sample = base >= 2, reduced = (kd & 16) || (g.mode != EMD_DENSIFY_MODE_REFINE && sample);
        const auto source = [&] { return t.src[(size_t)i * t.width + c]; };
        float v = 0.f;
        switch (t.role) {          // the same for every thread of the block: a scalar branch, and a copied row's load does not depend on its kind
        case EMD_DENSIFY_ROLE_STATE: if (!fresh) v = source(); break;                                              // Adam moments of new rows: zero
        case EMD_DENSIFY_ROLE_ZERO: if (!fresh && g.mode != EMD_DENSIFY_MODE_DENSIFY) v = source(); break;         // statistics: also reset by a densification
        case EMD_DENSIFY_ROLE_SCALING: v = source(); if (reduced) v = logf(expf(v) / 1.6f); break;
        case EMD_DENSIFY_ROLE_XYZ: v = source(); if (sample) v = split_sample_coord(g, i, base - 2, j, c, v); break;
        default: v = source();                                                                                     // COPY
        }
        t.dst[idx] = v;
    }
}

// rank of every split output row among the split rows of its replica (needed only when the samples are supplied by the caller)
__global__ void __launch_bounds__(EMD_BLOCK) k_densify_split_rank(int num_out, int n_keep, int n_clone, int n_split, int32_t* __restrict__ rank) {
    const int j = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (j >= num_out) return;
    const int base = n_keep + n_clone;
    rank[j] = j < base ? 0 : (j - base) % (n_split > 0 ? n_split : 1);
}

// ---- OmniRe refinement (EmdRefineArgs in include/emd_raster.h restates the semantics) ------------------------------------------------------------
enum { RCODE_KEEP = 1, RCODE_DUP = 2, RCODE_SAMPLES = 4, RCODE_SPLIT = 8 };

__global__ void __launch_bounds__(EMD_BLOCK) k_refine_decide(EmdRefineArgs a, int32_t* __restrict__ code, int32_t* __restrict__ counts /*[4][nblocks]*/) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    bool keep = false, keep_samples = false, keep_dup = false, split = false;
    if (i < a.num_points) {
    const float l0 = a.scaling[3 * i], l1 = a.scaling[3 * i + 1], l2 = a.scaling[3 * i + 2];
    float smax = fmaxf(expf(l0), fmaxf(expf(l1), expf(l2)));
    const float m2d = a.max_2Dsize ? a.max_2Dsize[i] : 0.f;
    bool dup = false;
    float smax_new = smax;
    if (a.do_densify) {
        const bool high = a.grad_norm[i] / a.vis_counts[i] > a.grad_threshold;
        split = (smax > a.size_threshold || (a.use_split_screen && m2d > a.split_screen)) && high;
        if (split) {
            // the original takes log(exp(s) / 1.6) in place; what the later tests see is exp() of THAT (vanilla.py:344-345,302-309)
            smax_new = fmaxf(expf(logf(expf(l0) / 1.6f)), fmaxf(expf(logf(expf(l1) / 1.6f)), expf(logf(expf(l2) / 1.6f))));
            smax = smax_new;
        }
        dup = smax <= a.size_threshold && high;
    }
    keep = true; keep_samples = split; keep_dup = dup;
    if (a.do_cull) {
        const float op = 1.f / (1.f + expf(-a.opacity[i]));
        const bool faint = op < a.cull_alpha;
        const bool big = a.cull_big && smax > a.cull_size;                        // the same (possibly reduced) scale on the original, its samples, its duplicate
        const bool wide_old = a.cull_big && a.use_cull_screen && m2d > a.cull_screen;
        const bool wide_new = a.cull_big && a.use_cull_screen && 0.f > a.cull_screen;      // new rows carry max_2Dsize 0 (vanilla.py:266-269)
        keep = !(faint || big || wide_old);
        keep_samples = split && !(faint || big || wide_new);
        keep_dup = dup && !(faint || big || wide_new);
    }
    code[i] = (keep ? RCODE_KEEP : 0) | (keep_dup ? RCODE_DUP : 0) | (keep_samples ? RCODE_SAMPLES : 0) | (split ? RCODE_SPLIT : 0);
    }
    const bool f[4] = {keep, keep_dup, keep_samples, split};
    block_flag_counts<4>(f, counts, (int)gridDim.x);
}

__global__ void __launch_bounds__(EMD_BLOCK) k_refine_index(int n, int num_samples, const int32_t* __restrict__ code, const int32_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ totals, int32_t* __restrict__ src, int32_t* __restrict__ kind,
                                                            int32_t* __restrict__ split_rank) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    const int c = i < n ? code[i] : 0;
    const bool f[4] = {(c & RCODE_KEEP) != 0, (c & RCODE_DUP) != 0, (c & RCODE_SAMPLES) != 0, (c & RCODE_SPLIT) != 0};
    int pos[4];
    block_flag_positions<4>(f, offsets, (int)gridDim.x, pos);
    const int n_keep = totals[0], n_samp = totals[2];
    const int sp = (c & RCODE_SPLIT) ? 16 : 0;
    if (c & RCODE_KEEP) { const int j = pos[0]; src[j] = i; kind[j] = sp; if (split_rank) split_rank[j] = 0; }
    if (c & RCODE_SAMPLES) {
        for (int rep = 0; rep < num_samples; rep++) {
            const int j = n_keep + rep * n_samp + pos[2];
            src[j] = i; kind[j] = (2 + rep) | sp;
            if (split_rank) split_rank[j] = pos[3];          // rank among ALL split sources (the row of a caller-supplied draw)
        }
    }
    if (c & RCODE_DUP) { const int j = n_keep + num_samples * n_samp + pos[1]; src[j] = i; kind[j] = 1 | sp; if (split_rank) split_rank[j] = 0; }
}

// VanillaGaussians.after_train (vanilla.py:163-191) for one view, in place
__global__ void __launch_bounds__(EMD_BLOCK) k_after_train_stats(int n, const int32_t* __restrict__ radii, const float* __restrict__ g, int stride,
                                                                 float* __restrict__ grad_norm, float* __restrict__ vis, float* __restrict__ m2d, float last_size) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int r = radii[i];
    if (r <= 0) return;
    const float gx = g[(size_t)stride * i], gy = g[(size_t)stride * i + 1];
    if (grad_norm) grad_norm[i] += sqrtf(gx * gx + gy * gy);
    if (vis) vis[i] += 1.f;
    if (m2d) m2d[i] = fmaxf(m2d[i], (float)r / last_size);
}

}  // namespace

extern "C" int emd_refine_decide(const EmdRefineArgs* a, int32_t* code, int32_t* columns, void* hip_stream) {
    if (!a || !code || !columns) { emd_set_error("refine_decide: null argument"); return EMD_ERR_INVALID; }
    if (a->num_points < 0) { emd_set_error("refine_decide: bad size"); return EMD_ERR_INVALID; }
    if (a->num_points == 0) return EMD_OK;
    if (!a->scaling || (a->do_densify && (!a->grad_norm || !a->vis_counts)) || (a->do_cull && !a->opacity) ||
        (((a->do_densify && a->use_split_screen) || (a->do_cull && a->cull_big && a->use_cull_screen)) && !a->max_2Dsize)) {
        emd_set_error("refine_decide: null input"); return EMD_ERR_INVALID;
    }
    hipLaunchKernelGGL(k_refine_decide, dim3((a->num_points + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, (hipStream_t)hip_stream, *a, code, columns);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_refine_index(int32_t num_points, int32_t num_out, int32_t num_samples, const int32_t* code, const int32_t* block_offsets, const int32_t* totals,
                                int32_t* src, int32_t* kind, int32_t* split_rank, void* hip_stream) {
    if (num_points < 0 || num_out < 0 || num_samples < 1 || num_samples > 13 || (num_points > 0 && (!code || !block_offsets || !totals)) || (num_out > 0 && (!src || !kind))) {
        emd_set_error("refine_index: bad argument"); return EMD_ERR_INVALID;
    }
    if (num_points == 0) return EMD_OK;
    hipLaunchKernelGGL(k_refine_index, dim3((num_points + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, (hipStream_t)hip_stream, num_points, num_samples, code,
                       block_offsets, totals, src, kind, split_rank);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_after_train_stats(int32_t n, const int32_t* radii, const float* xys_grad, int32_t grad_stride, float* grad_norm, float* vis_counts,
                                     float* max_2Dsize, float last_size, void* hip_stream) {
    if (n < 0 || grad_stride < 2 || !(last_size > 0.f) || (n > 0 && (!radii || !xys_grad))) { emd_set_error("after_train_stats: bad argument"); return EMD_ERR_INVALID; }
    if (n == 0) return EMD_OK;
    hipLaunchKernelGGL(k_after_train_stats, dim3((n + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, (hipStream_t)hip_stream, n, radii, xys_grad, grad_stride, grad_norm,
                       vis_counts, max_2Dsize, last_size);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_densify_decide(const EmdDensifyArgs* a, int32_t* code, int32_t* columns, void* hip_stream) {
    if (!a || !code || !columns) { emd_set_error("densify_decide: null argument"); return EMD_ERR_INVALID; }
    if (a->num_points < 0 || (a->mode != EMD_DENSIFY_MODE_DENSIFY && a->mode != EMD_DENSIFY_MODE_PRUNE)) { emd_set_error("densify_decide: bad mode / size"); return EMD_ERR_INVALID; }
    if (a->num_points == 0) return EMD_OK;
    if (!a->scaling || (a->mode == EMD_DENSIFY_MODE_DENSIFY && (!a->grad_accum || !a->denom)) ||
        (a->mode == EMD_DENSIFY_MODE_PRUNE && (!a->opacity || (a->max_screen_size > 0.f && !a->max_radii2D)))) {
        emd_set_error("densify_decide: null input for mode %d", a->mode); return EMD_ERR_INVALID;
    }
    hipLaunchKernelGGL(k_densify_decide, dim3((a->num_points + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, (hipStream_t)hip_stream, *a, code, columns);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_densify_scan(int32_t num_points, int32_t num_columns, int32_t* block_counts, int32_t* totals, void* hip_stream) {
    if (num_points < 0 || num_columns < 1 || num_columns > 8 || !totals || (num_points > 0 && !block_counts)) { emd_set_error("densify_scan: bad argument"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    if (num_points == 0) return emd_zero_async(totals, sizeof(int32_t) * (size_t)num_columns, st);
    hipLaunchKernelGGL(k_densify_scan, dim3((unsigned)num_columns), dim3(1024), 0, st, (num_points + EMD_BLOCK - 1) / EMD_BLOCK, block_counts, totals);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_densify_index(int32_t num_points, int32_t num_out, const int32_t* code, const int32_t* block_offsets, const int32_t* totals, int32_t* src,
                                 int32_t* kind, void* hip_stream) {
    if (num_points < 0 || num_out < 0 || (num_points > 0 && (!code || !block_offsets || !totals)) || (num_out > 0 && (!src || !kind))) {
        emd_set_error("densify_index: bad argument"); return EMD_ERR_INVALID;
    }
    if (num_points == 0) return EMD_OK;
    hipLaunchKernelGGL(k_densify_index, dim3((num_points + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, (hipStream_t)hip_stream, num_points, code,
                       block_offsets, totals, src, kind);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_densify_gather(const EmdDensifyGather* g, void* hip_stream) {
    if (!g) { emd_set_error("densify_gather: null args"); return EMD_ERR_INVALID; }
    if (g->num_tensors < 0 || g->num_tensors > EMD_DENSIFY_MAX_TENSORS || g->num_out < 0) { emd_set_error("densify_gather: bad sizes"); return EMD_ERR_INVALID; }
    if (g->num_out == 0 || g->num_tensors == 0) return EMD_OK;
    if (!g->src || !g->kind) { emd_set_error("densify_gather: null index"); return EMD_ERR_INVALID; }
    bool has_xyz = false;
    size_t widest = 1;
    for (int k = 0; k < g->num_tensors; k++) {
        const EmdDensifyTensor& t = g->tensors[k];
        if (!t.src || !t.dst || t.width <= 0) { emd_set_error("densify_gather: tensor %d: null pointer / bad width", k); return EMD_ERR_INVALID; }
        if (t.role == EMD_DENSIFY_ROLE_XYZ) { has_xyz = true; if (t.width != 3) { emd_set_error("densify_gather: xyz width must be 3"); return EMD_ERR_INVALID; } }
        if ((size_t)t.width > widest) widest = (size_t)t.width;
    }
    if (has_xyz && g->mode != EMD_DENSIFY_MODE_PRUNE && (!g->scaling || !g->rotation)) { emd_set_error("densify_gather: split needs scaling and rotation"); return EMD_ERR_INVALID; }
    if (g->samples && !g->split_rank) { emd_set_error("densify_gather: caller-supplied samples need split_rank"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t total = (size_t)g->num_out * widest;
    unsigned blocks = (unsigned)((total + EMD_BLOCK - 1) / EMD_BLOCK);
    if (blocks > 16384u) blocks = 16384u;
    hipLaunchKernelGGL(k_densify_gather, dim3(blocks, (unsigned)g->num_tensors), dim3(EMD_BLOCK), 0, st, *g);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_densify_split_rank(int32_t num_out, int32_t n_keep, int32_t n_clone, int32_t n_split, int32_t* rank, void* hip_stream) {
    if (num_out < 0 || (num_out > 0 && !rank)) { emd_set_error("densify_split_rank: bad argument"); return EMD_ERR_INVALID; }
    if (num_out == 0) return EMD_OK;
    hipLaunchKernelGGL(k_densify_split_rank, dim3((num_out + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, (hipStream_t)hip_stream, num_out, n_keep,
                       n_clone, n_split, rank);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

// ---- Refinement of the OmniRe actor classes (EmdRefineNodesArgs in include/emd_raster.h restates the contract) -----------------------------------
// Columns of a row's code (bit c = column c): 0 original kept, 1 duplicate kept, 2 source is split, 3 + r sample of replica r kept,
// 3 + num_samples id outside [0, num_actors).  The column count is a run-time number here (5..17), so the flags of a thread travel as one mask.
namespace {

enum { NCOL_KEEP = 0, NCOL_DUP = 1, NCOL_SPLIT = 2, NCOL_SAMPLE0 = 3, NODES_MAX_COLS = 4 + 13 };

// per-block counts of every column; every thread of the block calls it (threads past the end with mask 0)
__device__ __forceinline__ void block_mask_counts(uint32_t m, int ncols, int32_t* __restrict__ counts, int nblocks) {
    __shared__ uint32_t s_cnt[NODES_MAX_COLS][EMD_BLOCK / EMD_WAVE];
    const int wave = threadIdx.x / EMD_WAVE, lane = threadIdx.x % EMD_WAVE;
    for (int c = 0; c < ncols; c++) {
        const unsigned long long b = __ballot((m >> c) & 1u);
        if (lane == 0) s_cnt[c][wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if ((int)threadIdx.x < ncols) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < EMD_BLOCK / EMD_WAVE; w++) t += s_cnt[threadIdx.x][w];
        counts[(size_t)threadIdx.x * nblocks + blockIdx.x] = (int32_t)t;
    }
}

__global__ void __launch_bounds__(EMD_BLOCK) k_refine_nodes_decide(EmdRefineNodesArgs a, int32_t* __restrict__ code, int32_t* __restrict__ counts) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    const int ns = a.num_samples;
    uint32_t m = 0;
    if (i < a.num_points) {
    const int id = a.ids[i];
    if (id < 0 || id >= a.num_actors) m = 1u << (NCOL_SAMPLE0 + ns);
    else {
    // ---- the expressions of k_refine_decide -------------------------------------------------------------------------------------------------
    const float l0 = a.scaling[3 * i], l1 = a.scaling[3 * i + 1], l2 = a.scaling[3 * i + 2];
    float smax = fmaxf(expf(l0), fmaxf(expf(l1), expf(l2)));
    const float m2d = a.max_2Dsize ? a.max_2Dsize[i] : 0.f;
    bool dup = false, split = false;
    float smax_new = smax;
    if (a.do_densify) {
        const bool high = a.grad_norm[i] / a.vis_counts[i] > a.grad_threshold;
        split = (smax > a.size_threshold || (a.use_split_screen && m2d > a.split_screen)) && high;
        if (split) {
            smax_new = fmaxf(expf(logf(expf(l0) / 1.6f)), fmaxf(expf(logf(expf(l1) / 1.6f)), expf(logf(expf(l2) / 1.6f))));
            smax = smax_new;
        }
        dup = smax <= a.size_threshold && high;
    }
    bool keep = true, keep_dup = dup, drop_new = false;
    const bool box = a.do_cull && a.cull_out_of_bound;
    if (a.do_cull) {
        const float op = 1.f / (1.f + expf(-a.opacity[i]));
        const bool faint = op < a.cull_alpha;
        const bool big = a.cull_big && smax > a.cull_size;
        const bool wide_old = a.cull_big && a.use_cull_screen && m2d > a.cull_screen;
        const bool wide_new = a.cull_big && a.use_cull_screen && 0.f > a.cull_screen;
        bool out = false;                                         // the row's own mean against its actor's box
        if (box) {
#pragma unroll 1
            for (int c = 0; c < 3; c++) out = out || fabsf(a.means[3 * (size_t)i + c]) > a.instances_size[3 * (size_t)id + c] / 2.f;
        }
        keep = !(faint || big || wide_old || out);
        drop_new = faint || big || wide_new;
        keep_dup = dup && !(drop_new || out);
    }
    m = (keep ? 1u << NCOL_KEEP : 0u) | (keep_dup ? 1u << NCOL_DUP : 0u) | (split ? 1u << NCOL_SPLIT : 0u);
    if (split && !drop_new) {
        if (!box) m |= ((1u << ns) - 1u) << NCOL_SAMPLE0;
        else {
            // the gather's own position function on the gather's own inputs: samples by SOURCE ROW (num_split = N, the rank is the row)
            EmdDensifyGather g;
            int32_t row = i;
            g.samples = a.samples; g.num_split = a.num_points; g.split_rank = &row;
            g.seed = a.seed; g.scaling = a.scaling; g.rotation = a.rotation;
            for (int r = 0; r < ns; r++) {
                bool out = false;
#pragma unroll 1
                for (int c = 0; c < 3; c++) {
                    const float p = split_sample_coord(g, i, r, 0, c, a.means[3 * (size_t)i + c]);
                    out = out || fabsf(p) > a.instances_size[3 * (size_t)id + c] / 2.f;
                }
                if (!out) m |= 1u << (NCOL_SAMPLE0 + r);
            }
        }
    }
    }
    code[i] = (int32_t)m;
    }
    block_mask_counts(m, 4 + ns, counts, (int)gridDim.x);
}

// Every output row of source i, in the reference's order (kept originals, kept samples of replica 0, 1, ..., kept duplicates, each in source order).
// Ungrouped: straight into the outputs.  Grouped: `ids_out` is the sort's key buffer and `order` its value buffer (the row's own position).
__global__ void __launch_bounds__(EMD_BLOCK) k_refine_nodes_index(int n, int ns, int num_out, const int32_t* __restrict__ code, const int32_t* __restrict__ ids,
                                                                  const int32_t* __restrict__ offsets, const int32_t* __restrict__ totals, int32_t* __restrict__ src,
                                                                  int32_t* __restrict__ kind, int32_t* __restrict__ ids_out, int32_t* __restrict__ split_rank,
                                                                  uint32_t* __restrict__ order) {
    __shared__ uint32_t s_cnt[NODES_MAX_COLS][EMD_BLOCK / EMD_WAVE];
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    const int wave = threadIdx.x / EMD_WAVE, lane = threadIdx.x % EMD_WAVE, nblocks = (int)gridDim.x, ncols = 3 + ns;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const uint32_t m = i < n ? (uint32_t)code[i] : 0u;
    for (int c = 0; c < ncols; c++) {
        const unsigned long long b = __ballot((m >> c) & 1u);
        if (lane == 0) s_cnt[c][wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    const int id = i < n ? ids[i] : 0;
    const int sp = (m >> NCOL_SPLIT) & 1u ? 16 : 0;
    int base = 0;                                                  // first output row of the column's section
    const auto emit = [&](int c, int kd, int rank) {
        const unsigned long long b = __ballot((m >> c) & 1u);      // (every lane of the wave gets here: `c` is uniform)
        if ((m >> c) & 1u) {
            int j = base + offsets[(size_t)c * nblocks + blockIdx.x] + __popcll(b & lt);
            for (int w = 0; w < wave; w++) j += (int)s_cnt[c][w];
            if (j < num_out) {
                src[j] = i; kind[j] = kd | sp; ids_out[j] = id;
                if (split_rank) split_rank[j] = rank;
                if (order) order[j] = (uint32_t)j;
            }
        }
    };
    emit(NCOL_KEEP, 0, 0);
    base = totals[NCOL_KEEP];
    for (int r = 0; r < ns; r++) { emit(NCOL_SAMPLE0 + r, 2 + r, i); base += totals[NCOL_SAMPLE0 + r]; }
    emit(NCOL_DUP, 1, 0);
}

// grouped: output row k takes the row the stable sort put there; segment_start[a] = first k with actor >= a
__global__ void __launch_bounds__(EMD_BLOCK) k_refine_nodes_group(int num_out, int num_actors, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                                                                  const int32_t* __restrict__ src_u, const int32_t* __restrict__ kind_u, int32_t* __restrict__ src,
                                                                  int32_t* __restrict__ kind, int32_t* __restrict__ ids_out, int32_t* __restrict__ split_rank,
                                                                  int32_t* __restrict__ segment_start) {
    const int k = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (k < num_out) {
        const uint32_t j = order[k];
        if (j < (uint32_t)num_out) {
            const int s = src_u[j], kd = kind_u[j];
            src[k] = s; kind[k] = kd; ids_out[k] = (int32_t)keys[k];
            if (split_rank) split_rank[k] = (kd & 15) >= 2 ? s : 0;
        }
    }
    if (k <= num_actors) {
        int lo = 0, hi = num_out;
        while (lo < hi) { const int mid = lo + (hi - lo) / 2; if (keys[mid] < (uint32_t)k) lo = mid + 1; else hi = mid; }
        segment_start[k] = lo;
    }
}

size_t nodes_ws_align(size_t words) { return (words + 63) / 64 * 64; }          // sections start on 256-byte boundaries

bool nodes_args_ok(const EmdRefineNodesArgs* a, const char* what) {
    if (a->num_points < 0) { emd_set_error("%s: negative size", what); return false; }
    if (a->num_actors < 1 || a->num_actors > 65536) { emd_set_error("%s: num_actors %d outside 1..65536", what, a->num_actors); return false; }
    if (a->num_samples < 1 || a->num_samples > 13) { emd_set_error("%s: num_samples %d outside 1..13", what, a->num_samples); return false; }
    if ((a->cull_out_of_bound | a->group_by_actor) & ~1) { emd_set_error("%s: cull_out_of_bound / group_by_actor must be 0 or 1", what); return false; }
    return true;
}

}  // namespace

extern "C" int emd_refine_nodes_decide(const EmdRefineNodesArgs* a, int32_t* code, int32_t* columns, void* hip_stream) {
    if (!a || !code || !columns) { emd_set_error("refine_nodes_decide: null argument"); return EMD_ERR_INVALID; }
    if (!nodes_args_ok(a, "refine_nodes_decide")) return EMD_ERR_INVALID;
    if (a->num_points == 0) return EMD_OK;
    if (!a->scaling || !a->ids || (a->do_densify && (!a->grad_norm || !a->vis_counts)) || (a->do_cull && !a->opacity) ||
        (((a->do_densify && a->use_split_screen) || (a->do_cull && a->cull_big && a->use_cull_screen)) && !a->max_2Dsize) ||
        (a->do_cull && a->cull_out_of_bound && (!a->means || !a->rotation || !a->instances_size))) {
        emd_set_error("refine_nodes_decide: null input"); return EMD_ERR_INVALID;
    }
    hipLaunchKernelGGL(k_refine_nodes_decide, dim3((a->num_points + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, (hipStream_t)hip_stream, *a, code, columns);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

// scratch of a grouped index over num_out rows: two key and two value buffers of the sort, the ungrouped src / kind, the sort's histograms
extern "C" size_t emd_refine_nodes_index_workspace(int32_t num_out) {
    if (num_out <= 0) return 0;
    const size_t m = nodes_ws_align((size_t)num_out), tiles = ((size_t)num_out + EMD_SORT_TILE - 1) / EMD_SORT_TILE;
    return sizeof(uint32_t) * (6 * m + nodes_ws_align(512 * tiles));
}

extern "C" int emd_refine_nodes_index(const EmdRefineNodesArgs* a, int32_t num_out, const int32_t* code, const int32_t* block_offsets, const int32_t* totals,
                                      int32_t* src, int32_t* kind, int32_t* ids_out, int32_t* segment_start, int32_t* split_rank, void* workspace,
                                      size_t workspace_bytes, void* hip_stream) {
    if (!a) { emd_set_error("refine_nodes_index: null argument"); return EMD_ERR_INVALID; }
    if (!nodes_args_ok(a, "refine_nodes_index")) return EMD_ERR_INVALID;
    const int n = a->num_points, ns = a->num_samples;
    const bool grouped = a->group_by_actor != 0;
    if (num_out < 0 || (grouped && !segment_start) || (n > 0 && (!code || !block_offsets || !totals || !a->ids)) || (num_out > 0 && (!src || !kind || !ids_out)) ||
        (n > 0 && grouped && num_out > 0 && (!workspace || workspace_bytes < emd_refine_nodes_index_workspace(num_out)))) {
        emd_set_error("refine_nodes_index: bad argument"); return EMD_ERR_INVALID;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (n == 0 || num_out == 0) return segment_start ? emd_zero_async(segment_start, sizeof(int32_t) * ((size_t)a->num_actors + 1), st) : EMD_OK;
    const dim3 grid((n + EMD_BLOCK - 1) / EMD_BLOCK), block(EMD_BLOCK);
    if (!grouped) {
        hipLaunchKernelGGL(k_refine_nodes_index, grid, block, 0, st, n, ns, num_out, code, a->ids, block_offsets, totals, src, kind, ids_out, split_rank, (uint32_t*)nullptr);
        EMD_LAUNCH_CHECK();
        return EMD_OK;
    }
    const size_t m = nodes_ws_align((size_t)num_out);
    uint32_t* w = (uint32_t*)workspace;
    RadixSortArgs r;
    r.keys[0] = w; r.keys[1] = w + m; r.vals[0] = w + 2 * m; r.vals[1] = w + 3 * m;
    int32_t *src_u = (int32_t*)(w + 4 * m), *kind_u = (int32_t*)(w + 5 * m);
    r.hist = w + 6 * m;
    r.n_cap = (size_t)num_out;
    int bits = 1;
    while (bits < 32 && ((uint32_t)(a->num_actors - 1) >> bits)) bits++;
    r.bits = 9;
    r.passes = (bits + 8) / 9;                                    // 1 up to 512 actors, 2 up to 65 536
    hipLaunchKernelGGL(k_refine_nodes_index, grid, block, 0, st, n, ns, num_out, code, a->ids, block_offsets, totals, src_u, kind_u, (int32_t*)r.keys[0], (int32_t*)nullptr,
                       r.vals[0]);
    EMD_LAUNCH_CHECK();
    const int buf = emd_launch_radix_sort(r, st);
    if (buf < 0) return buf;
    const int threads = num_out > a->num_actors + 1 ? num_out : a->num_actors + 1;
    hipLaunchKernelGGL(k_refine_nodes_group, dim3((threads + EMD_BLOCK - 1) / EMD_BLOCK), block, 0, st, num_out, a->num_actors, (const uint32_t*)r.keys[buf],
                       (const uint32_t*)r.vals[buf], (const int32_t*)src_u, (const int32_t*)kind_u, src, kind, ids_out, split_rank, segment_start);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}
