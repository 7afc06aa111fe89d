// knn.hip -- exact k nearest neighbours of 1 - 3 M points in 3-D, and the embedding regulariser over the neighbour table (ABI 28).
//
//   emd_knn                 distCUDA2 of create_from_pcd (k = 3, S3Gaussian/scene/gaussian_model.py:152-181) and the 20-neighbour table of the
//                           fine stage's regulariser (o3d_knn, train.py:326-337)
//   emd_knn_segments        the same contract inside segments (the instances of SMPLNodes: a pedestrian's neighbours are its own points): brute
//                           force per segment, k_knn_segments below; no workspace
//   emd_knn_reverse         the table's transposed adjacency (CSR), so that the regulariser's backward is a gather
//   emd_embed_reg_forward   weighted_l2_loss_v2(e[:, None], e[idx], w) = mean sqrt(w |e_n - e_m|^2 + 1e-20)
//   emd_embed_reg_backward  its gradient with respect to e, bit-identical from run to run
//
// Search.  Street scenes are very non-uniform (LiDAR sweeps, a ground plane, empty sky), so the space is cut by the data, not by a grid:
//   k_knn_bounds_*   bounding box of the finite points (two launches, no atomics)
//   k_knn_keys       30-bit Z-order key per point; a point with a non-finite coordinate gets the key 0xFFFFFFFF, which the first radix pass
//                    drops, and its output row (-1 / +inf) is written here
//   (radix_sort.hip) stable radix sort of (key, index): 4 passes of 8 bits; V = number of finite points stays on the device
//   k_knn_leaves     the points in sorted order as float4 (x, y, z, index bits); every 64 consecutive ones are a LEAF with its min / max corners
//   k_knn_groups     every 64 consecutive leaves are a GROUP with its corners
//   k_knn_search<K>  one wave per leaf; lane i owns query i of the leaf and keeps its K best (distance, index) pairs sorted in registers.
//                    The lists are seeded from the leaves L-2 .. L+2 (neighbours on the curve are mostly neighbours in space).  Then the wave
//                    tests 64 group boxes at a time -- one per lane -- against the LEAF's box and the largest k-th distance of its lanes, the
//                    64 leaf boxes of every group that passes in the same way, and for every leaf that passes each lane tests the box against
//                    its own query and k-th distance; if any lane still wants the leaf, all 64 points are scanned by every lane (the point
//                    address is uniform over the wave: scalar loads, no LDS staging needed).  A box is skipped only when its distance,
//                    evaluated with the SAME fp32 expression as a point distance, is not below the k-th distance: the expression is monotone
//                    in |dx|, |dy|, |dz|, so nothing that would have been inserted is skipped -- the result is exact.
// The traversal order is fixed, so the result is deterministic, equidistant candidates included (the earlier one in the order stays).
#include "common.h"
#include "device_utils.h"
#include "radix_sort.h"

#include <math.h>

namespace {

#define KNN_LEAF 64                  // points per leaf = queries per wave
#define KNN_GROUP 64                 // leaves per group
#define KNN_SEED 2                   // leaves either side of the wave's own that seed the candidate lists
#define KNN_BOUNDS_BLOCKS 1024
#define KNN_SORT_PASSES 4            // 30 key bits + the dropped all-ones key

__device__ __forceinline__ float knn_dist2(float dx, float dy, float dz) { return fmaf(dz, dz, fmaf(dy, dy, dx * dx)); }

__device__ __forceinline__ float wave_min_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// largest of the lanes' NON-NEGATIVE floats (+inf included): they order like their bit patterns
__device__ __forceinline__ float wave_max_nonneg(float v) {
    return __uint_as_float(readlane_u32(wave_scan_max_u32(__float_as_uint(v)), 63));
}

struct Box { float lo[3], hi[3]; };

__device__ __forceinline__ void box_reduce_block(Box& b, float (*s)[6]) {      // 256 threads -> thread 0
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; a++) { b.lo[a] = wave_min_f32(b.lo[a]); b.hi[a] = wave_max_f32(b.hi[a]); }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) { s[wave][a] = b.lo[a]; s[wave][3 + a] = b.hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            b.lo[a] = fminf(fminf(s[0][a], s[1][a]), fminf(s[2][a], s[3][a]));
            b.hi[a] = fmaxf(fmaxf(s[0][3 + a], s[1][3 + a]), fmaxf(s[2][3 + a], s[3][3 + a]));
        }
    }
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__global__ void __launch_bounds__(EMD_BLOCK) k_knn_bounds_partial(int N, const float* __restrict__ pts, float* __restrict__ partial /*[grid][6]*/) {
    __shared__ float s[4][6];
    Box b;
#pragma unroll
    for (int a = 0; a < 3; a++) { b.lo[a] = INFINITY; b.hi[a] = -INFINITY; }
    for (int n = blockIdx.x * EMD_BLOCK + threadIdx.x; n < N; n += gridDim.x * EMD_BLOCK) {
        const float x = pts[3 * (size_t)n], y = pts[3 * (size_t)n + 1], z = pts[3 * (size_t)n + 2];
        if (finite3(x, y, z)) {
            b.lo[0] = fminf(b.lo[0], x); b.lo[1] = fminf(b.lo[1], y); b.lo[2] = fminf(b.lo[2], z);
            b.hi[0] = fmaxf(b.hi[0], x); b.hi[1] = fmaxf(b.hi[1], y); b.hi[2] = fmaxf(b.hi[2], z);
        }
    }
    box_reduce_block(b, s);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) { partial[6 * blockIdx.x + a] = b.lo[a]; partial[6 * blockIdx.x + 3 + a] = b.hi[a]; }
    }
}

__global__ void __launch_bounds__(EMD_BLOCK) k_knn_bounds_final(int num_partial, const float* __restrict__ partial, float* __restrict__ aabb /*[6]*/) {
    __shared__ float s[4][6];
    Box b;
#pragma unroll
    for (int a = 0; a < 3; a++) { b.lo[a] = INFINITY; b.hi[a] = -INFINITY; }
    for (int i = threadIdx.x; i < num_partial; i += EMD_BLOCK) {
#pragma unroll
        for (int a = 0; a < 3; a++) { b.lo[a] = fminf(b.lo[a], partial[6 * i + a]); b.hi[a] = fmaxf(b.hi[a], partial[6 * i + 3 + a]); }
    }
    box_reduce_block(b, s);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) { aabb[a] = b.lo[a]; aabb[3 + a] = b.hi[a]; }
    }
}

__device__ __forceinline__ uint32_t knn_spread3(uint32_t v) {     // abcdefghij -> a00b00c00d00e00f00g00h00i00j
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    return (v | (v << 2)) & 0x09249249u;
}

__global__ void __launch_bounds__(EMD_BLOCK) k_knn_keys(int N, int k, const float* __restrict__ pts, const float* __restrict__ aabb, uint32_t* __restrict__ keys,
                                                        int32_t* __restrict__ idx, float* __restrict__ d2, float* __restrict__ mean_d2) {
    const int n = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (n >= N) return;
    const float p[3] = {pts[3 * (size_t)n], pts[3 * (size_t)n + 1], pts[3 * (size_t)n + 2]};
    if (!finite3(p[0], p[1], p[2])) {
        keys[n] = 0xFFFFFFFFu;
        for (int j = 0; j < k; j++) {
            if (idx) idx[(size_t)n * k + j] = -1;
            if (d2) d2[(size_t)n * k + j] = INFINITY;
        }
        if (mean_d2) mean_d2[n] = INFINITY;
        return;
    }
    uint32_t q[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        float u = (p[a] - aabb[a]) / (aabb[3 + a] - aabb[a]);         // (a flat axis: 0 / 0 = NaN -> 0, fmaxf returns the other operand)
        u = fminf(fmaxf(u, 0.f), 1.f);
        q[a] = (uint32_t)(u * 1023.f);
    }
    keys[n] = knn_spread3(q[0]) | (knn_spread3(q[1]) << 1) | (knn_spread3(q[2]) << 2);
}

// sorted points + leaf boxes.  One wave per leaf; the grid covers num_groups * 64 leaves, so the arrays hold no unwritten entry: a slot past the
// V sorted points is NaN (never nearer than anything), a leaf without points has the box (+inf, -inf) (never nearer than anything).
__global__ void __launch_bounds__(EMD_BLOCK) k_knn_leaves(const float* __restrict__ pts, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ count,
                                                          float4* __restrict__ sp, float4* __restrict__ leaf_box) {
    const uint32_t V = *count;
    const uint32_t i = blockIdx.x * EMD_BLOCK + threadIdx.x, leaf = i / KNN_LEAF;
    float4 v = make_float4(NAN, NAN, NAN, __int_as_float(-1));
    if (i < V) {
        const uint32_t n = perm[i];
        v = make_float4(pts[3 * (size_t)n], pts[3 * (size_t)n + 1], pts[3 * (size_t)n + 2], __int_as_float((int)n));
    }
    sp[i] = v;
    const bool in = i < V;
    const float lx = wave_min_f32(in ? v.x : INFINITY), ly = wave_min_f32(in ? v.y : INFINITY), lz = wave_min_f32(in ? v.z : INFINITY);
    const float hx = wave_max_f32(in ? v.x : -INFINITY), hy = wave_max_f32(in ? v.y : -INFINITY), hz = wave_max_f32(in ? v.z : -INFINITY);
    if ((threadIdx.x & 63) == 0) { leaf_box[2 * leaf] = make_float4(lx, ly, lz, 0.f); leaf_box[2 * leaf + 1] = make_float4(hx, hy, hz, 0.f); }
}

__global__ void __launch_bounds__(EMD_BLOCK) k_knn_groups(uint32_t num_groups, const float4* __restrict__ leaf_box, float4* __restrict__ group_box) {
    const uint32_t g = blockIdx.x * (EMD_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= num_groups) return;                      // (uniform over the wave)
    const float4 lo = leaf_box[2 * ((size_t)g * KNN_GROUP + lane)], hi = leaf_box[2 * ((size_t)g * KNN_GROUP + lane) + 1];
    const float lx = wave_min_f32(lo.x), ly = wave_min_f32(lo.y), lz = wave_min_f32(lo.z);
    const float hx = wave_max_f32(hi.x), hy = wave_max_f32(hi.y), hz = wave_max_f32(hi.z);
    if (lane == 0) { group_box[2 * g] = make_float4(lx, ly, lz, 0.f); group_box[2 * g + 1] = make_float4(hx, hy, hz, 0.f); }
}

// `d` is below the list's last distance: shift the farther entries up by one and drop (d, id) into the gap.  Fully unrolled, so the list stays in
// registers; an equidistant entry already in the list stays in front of the new one.
template <int K>
__device__ __forceinline__ void knn_insert(float (&dl)[K], int (&il)[K], float d, int id) {
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
        const bool up = d < dl[j - 1], here = d < dl[j];
        il[j] = up ? il[j - 1] : (here ? id : il[j]);
        dl[j] = up ? dl[j - 1] : (here ? d : dl[j]);
    }
    if (d < dl[0]) { dl[0] = d; il[0] = id; }
}

// every lane tests the 64 points of one leaf (`lp` is uniform over the wave) against its own query; `skip` = the lane's own slot in its own leaf
template <int K>
__device__ __forceinline__ void knn_scan_leaf(const float4* __restrict__ lp, float qx, float qy, float qz, int skip, float (&dl)[K], int (&il)[K]) {
#pragma unroll 8
    for (int j = 0; j < KNN_LEAF; j++) {
        const float4 p = lp[j];
        const float d = knn_dist2(qx - p.x, qy - p.y, qz - p.z);
        if (d < dl[K - 1] && j != skip) knn_insert<K>(dl, il, d, __float_as_int(p.w));
    }
}

// distance between two boxes / a point and a box along one axis (0 when they overlap; NaN operands give 0 or NaN, both harmless: see the callers)
__device__ __forceinline__ float knn_gap(float alo, float ahi, float blo, float bhi) { return fmaxf(fmaxf(blo - ahi, alo - bhi), 0.f); }

template <int K>
__global__ void __launch_bounds__(EMD_BLOCK) k_knn_search(int k, const uint32_t* __restrict__ count, const float4* __restrict__ sp,
                                                          const float4* __restrict__ leaf_box, const float4* __restrict__ group_box,
                                                          int32_t* __restrict__ idx, float* __restrict__ d2, float* __restrict__ mean_d2) {
    const uint32_t V = *count;
    const uint32_t num_leaves = (V + KNN_LEAF - 1) / KNN_LEAF, num_groups = (num_leaves + KNN_GROUP - 1) / KNN_GROUP;
    const uint32_t L = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (EMD_BLOCK / 64) + (threadIdx.x >> 6)));
    if (L >= num_leaves) return;                      // (uniform over the wave; the kernel has no workgroup barrier)
    const int lane = threadIdx.x & 63;
    const bool active = (size_t)L * KNN_LEAF + lane < V;
    const float4 me = sp[(size_t)L * KNN_LEAF + lane];                // (NaN past the end: such a lane never inserts anything)
    float dl[K];
    int il[K];
#pragma unroll
    for (int j = 0; j < K; j++) { dl[j] = active ? INFINITY : 0.f; il[j] = -1; }      // (0: an idle lane does not hold the wave's bound up)
    const uint32_t s0 = L > KNN_SEED ? L - KNN_SEED : 0u, s1 = min(L + KNN_SEED, num_leaves - 1);
    for (uint32_t l = s0; l <= s1; l++) knn_scan_leaf<K>(sp + (size_t)l * KNN_LEAF, me.x, me.y, me.z, l == L ? lane : -1, dl, il);
    const float4 qlo = leaf_box[2 * (size_t)L], qhi = leaf_box[2 * (size_t)L + 1];
    for (uint32_t gbase = 0; gbase < num_groups; gbase += 64) {
        const uint32_t g = gbase + lane;
        const bool gin = g < num_groups;
        const float4 glo = gin ? group_box[2 * (size_t)g] : make_float4(INFINITY, INFINITY, INFINITY, 0.f);
        const float4 ghi = gin ? group_box[2 * (size_t)g + 1] : make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
        float bound = wave_max_nonneg(dl[K - 1]);
        unsigned long long gm = __ballot(gin && knn_dist2(knn_gap(qlo.x, qhi.x, glo.x, ghi.x), knn_gap(qlo.y, qhi.y, glo.y, ghi.y),
                                                          knn_gap(qlo.z, qhi.z, glo.z, ghi.z)) < bound);
        while (gm) {
            const uint32_t grp = gbase + (uint32_t)__builtin_ctzll(gm);
            gm &= gm - 1;
            const uint32_t l = grp * KNN_GROUP + lane;                 // (the leaf-box array is written for every leaf of every group)
            const float4 llo = leaf_box[2 * (size_t)l], lhi = leaf_box[2 * (size_t)l + 1];
            bound = wave_max_nonneg(dl[K - 1]);
            unsigned long long lm = __ballot(!(l >= s0 && l <= s1) && knn_dist2(knn_gap(qlo.x, qhi.x, llo.x, lhi.x), knn_gap(qlo.y, qhi.y, llo.y, lhi.y),
                                                                                knn_gap(qlo.z, qhi.z, llo.z, lhi.z)) < bound);
            while (lm) {
                const int lj = __builtin_ctzll(lm);
                lm &= lm - 1;
                const float bx0 = readlane_f32(llo.x, lj), by0 = readlane_f32(llo.y, lj), bz0 = readlane_f32(llo.z, lj);
                const float bx1 = readlane_f32(lhi.x, lj), by1 = readlane_f32(lhi.y, lj), bz1 = readlane_f32(lhi.z, lj);
                const float bd = knn_dist2(knn_gap(me.x, me.x, bx0, bx1), knn_gap(me.y, me.y, by0, by1), knn_gap(me.z, me.z, bz0, bz1));
                if (__ballot(bd < dl[K - 1]))
                    knn_scan_leaf<K>(sp + ((size_t)grp * KNN_GROUP + lj) * KNN_LEAF, me.x, me.y, me.z, -1, dl, il);
            }
        }
    }
    if (!active) return;
    const size_t row = (size_t)__float_as_int(me.w) * k;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < K; j++) {
        if (j < k) {
            if (idx) idx[row + j] = il[j];
            if (d2) d2[row + j] = dl[j];
            sum += dl[j];
        }
    }
    if (mean_d2) mean_d2[__float_as_int(me.w)] = sum / (float)k;
}

// ---- search inside segments ----------------------------------------------------------------------------------------------------------------------
// emd_knn_segments: row n's candidates are the other rows of n's own segment [segment_start[s], segment_start[s+1]).  Segments are people (6 890
// points) or actors: small enough for brute force, so there is no sort and no workspace.  A wave owns 64 consecutive rows; each lane finds its own
// range by binary search in the table, the wave walks the union of its lanes' ranges in ascending row order at a wave-uniform address (scalar
// loads, as knn_scan_leaf), and a lane skips the candidates outside its own range and itself.  The ascending walk with knn_insert's strict `<`
// puts the lower row first among equidistant candidates.  A candidate with a non-finite coordinate gives d = NaN or +inf: never `<` anything.
template <int K>
__global__ void __launch_bounds__(EMD_BLOCK) k_knn_segments(int N, int S, int k, const float* __restrict__ pts, const int32_t* __restrict__ segment_start,
                                                            int32_t* __restrict__ idx, float* __restrict__ d2) {
    const int row0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (EMD_BLOCK / 64) + (threadIdx.x >> 6))) * 64;
    if (row0 >= N) return;                            // (uniform over the wave; the kernel has no workgroup barrier)
    const int n = row0 + (int)(threadIdx.x & 63);
    const bool in = n < N;
    int lo = 0, hi = 0;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (in) {
        // the last s in [0, S] whose clamped start is <= n (the table ascends); s == S or none: the row lies outside every segment
        int a = 0, b = S + 1;
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (min(max(segment_start[mid], 0), N) <= n) a = mid + 1; else b = mid;
        }
        const int s = a - 1;
        if (s >= 0 && s < S) { lo = min(max(segment_start[s], 0), N); hi = min(max(segment_start[s + 1], 0), N); }
        qx = pts[3 * (size_t)n]; qy = pts[3 * (size_t)n + 1]; qz = pts[3 * (size_t)n + 2];
        if (!finite3(qx, qy, qz)) lo = hi = 0;
    }
    const bool active = in && n >= lo && n < hi;
    float dl[K];
    int il[K];
#pragma unroll
    for (int j = 0; j < K; j++) { dl[j] = INFINITY; il[j] = -1; }
    int wlo = active ? lo : N, whi = active ? hi : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { wlo = min(wlo, __shfl_xor(wlo, o)); whi = max(whi, __shfl_xor(whi, o)); }
    wlo = __builtin_amdgcn_readfirstlane(wlo);
    whi = __builtin_amdgcn_readfirstlane(whi);
    const int mylo = active ? lo : 0, myhi = active ? hi : 0;
#pragma unroll 8
    for (int m = wlo; m < whi; m++) {
        const float px = pts[3 * (size_t)m], py = pts[3 * (size_t)m + 1], pz = pts[3 * (size_t)m + 2];
        const float d = knn_dist2(qx - px, qy - py, qz - pz);
        if (d < dl[K - 1] && m >= mylo && m < myhi && m != n) knn_insert<K>(dl, il, d, m);
    }
    if (!in) return;
    const size_t row = (size_t)n * k;
#pragma unroll
    for (int j = 0; j < K; j++) {
        if (j < k) {
            if (idx) idx[row + j] = il[j];
            if (d2) d2[row + j] = dl[j];
        }
    }
}

// ---- transposed adjacency -----------------------------------------------------------------------------------------------------------------------
// sorted targets (the kept entries of idx, ascending, stable) -> rev_start: thread i closes the rows between target[i-1] and target[i]
__global__ void __launch_bounds__(EMD_BLOCK) k_knn_rev_start(int N, uint32_t total, const uint32_t* __restrict__ targets, const uint32_t* __restrict__ count,
                                                             int32_t* __restrict__ rev_start) {
    const uint32_t cnt = *count;
    const uint32_t i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i > cnt || i > total) return;
    const int64_t prev = i ? (int64_t)min(targets[i - 1], (uint32_t)(N - 1)) : -1;
    const int64_t cur = i < cnt ? (int64_t)min(targets[i], (uint32_t)(N - 1)) : (int64_t)N;
    for (int64_t t = prev + 1; t <= cur; t++) rev_start[t] = (int32_t)i;
}

// ---- regulariser ----------------------------------------------------------------------------------------------------------------------------------
#define REG_THREADS 1024
#define REG_MAX_BLOCKS 512           // granules of one quantity in the scratch table (EMD_EMBED_REG_SCRATCH_WORDS = 2 quantities x 512 x 2 words)
#define REG_EPS 1e-20f

template <int E>
__device__ __forceinline__ void load_row(const float* __restrict__ e, uint32_t n, float (&v)[E]) {
#pragma unroll
    for (int q = 0; q < E / 4; q++) {
        const float4 t = reinterpret_cast<const float4*>(e)[(size_t)n * (E / 4) + q];
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
}

// One pair per thread and trip.  The sum and the pair count leave every workgroup as two 8-byte {value, tag} granules; workgroup 0 adds them in
// workgroup order (the scheme of k_l1_loss, standalone_ops.hip: nobody but workgroup 0 waits, so it cannot deadlock) and writes loss, 1 / pairs.
template <int E>
__global__ void __launch_bounds__(REG_THREADS) k_embed_reg_fwd(uint32_t N, uint32_t k, const float* __restrict__ e, const int32_t* __restrict__ idx,
                                                               const float* __restrict__ w, float* __restrict__ c, float* __restrict__ loss,
                                                               uint32_t* __restrict__ scratch) {
    __shared__ float s_sum[REG_THREADS / 64];
    __shared__ uint32_t s_cnt[REG_THREADS / 64];
    const uint32_t total = N * k, stride = gridDim.x * REG_THREADS;
    float acc = 0.f;
    uint32_t cnt = 0;
    for (uint32_t i = blockIdx.x * REG_THREADS + threadIdx.x; i < total; i += stride) {
        const int32_t m = idx[i];
        const float wv = w ? w[i] : 1.f;
        float cv = 0.f;
        if ((uint32_t)m < N) {
            float a[E], b[E];
            load_row<E>(e, i / k, a);
            load_row<E>(e, (uint32_t)m, b);
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < E; q++) { const float d = a[q] - b[q]; s = fmaf(d, d, s); }
            const float v = sqrtf(fmaf(wv, s, REG_EPS));
            acc += v;
            cnt++;
            cv = wv / v;
        }
        if (c) c[i] = cv;
    }
    acc = wave_reduce_to_lane63(acc);
    cnt = wave_scan_add_u32(cnt);
    if ((threadIdx.x & 63) == 63) { s_sum[threadIdx.x >> 6] = acc; s_cnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    unsigned long long* tab = reinterpret_cast<unsigned long long*>(scratch);
    if (threadIdx.x == 0) {
        float t = 0.f;
        uint32_t n = 0;
#pragma unroll
        for (int i = 0; i < REG_THREADS / 64; i++) { t += s_sum[i]; n += s_cnt[i]; }
        if (blockIdx.x != 0) {
            __hip_atomic_store(tab + blockIdx.x, ((unsigned long long)__float_as_uint(t) << 32) | 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(tab + REG_MAX_BLOCKS + blockIdx.x, ((unsigned long long)n << 32) | 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else { s_sum[0] = t; s_cnt[0] = n; }
    }
    if (blockIdx.x != 0) return;
    __syncthreads();
    float v = threadIdx.x == 0 ? s_sum[0] : 0.f;
    uint32_t n = threadIdx.x == 0 ? s_cnt[0] : 0u;
    if (threadIdx.x > 0 && threadIdx.x < gridDim.x) {          // one poller per other workgroup (gridDim.x <= REG_MAX_BLOCKS <= REG_THREADS)
        unsigned long long g0, g1;
        for (;;) {
            g0 = __hip_atomic_load(tab + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            g1 = __hip_atomic_load(tab + REG_MAX_BLOCKS + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((g0 & 1ull) && (g1 & 1ull)) break;
            __builtin_amdgcn_s_sleep(2);
        }
        v = __uint_as_float((uint32_t)(g0 >> 32));
        n = (uint32_t)(g1 >> 32);
        __hip_atomic_store(tab + threadIdx.x, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // the table is zero again for the next call
        __hip_atomic_store(tab + REG_MAX_BLOCKS + threadIdx.x, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();                                           // (thread 0 has read s_sum[0] / s_cnt[0])
    v = wave_reduce_to_lane63(v);                              // a fixed tree: the same sum for the same partials
    n = wave_scan_add_u32(n);
    if ((threadIdx.x & 63) == 63) { s_sum[threadIdx.x >> 6] = v; s_cnt[threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        uint32_t p = 0;
#pragma unroll
        for (int i = 0; i < REG_THREADS / 64; i++) { t += s_sum[i]; p += s_cnt[i]; }
        loss[0] = p ? t / (float)p : 0.f;
        loss[1] = p ? 1.f / (float)p : 0.f;
    }
}

// Eight lanes per row: lane g of the group takes the entries g, g + 8, ... of the row's own neighbours and then of its reverse list, the eight
// partial rows are added in a fixed butterfly.  Every term is c (e[n] - e[other]): a pair contributes to both of its ends with opposite signs.
#define REG_BWD_LANES 8
template <int E>
__global__ void __launch_bounds__(EMD_BLOCK) k_embed_reg_bwd(uint32_t N, uint32_t k, const float* __restrict__ e, const int32_t* __restrict__ idx,
                                                             const float* __restrict__ w, const float* __restrict__ c, const int32_t* __restrict__ rev_start,
                                                             const int32_t* __restrict__ rev_slot, const float* __restrict__ g,
                                                             const float* __restrict__ inv_pairs, float* __restrict__ grad_e, int accumulate) {
    const uint32_t row = blockIdx.x * (EMD_BLOCK / REG_BWD_LANES) + threadIdx.x / REG_BWD_LANES, sub = threadIdx.x % REG_BWD_LANES;
    const bool in = row < N;
    const uint32_t n = in ? row : 0u;
    float en[E], acc[E];
    load_row<E>(e, n, en);
#pragma unroll
    for (int q = 0; q < E; q++) acc[q] = 0.f;
    auto pair = [&](uint32_t other, uint32_t slot) {
        float eo[E], d[E];
        load_row<E>(e, other, eo);
        float cf;
        if (c) cf = c[slot];
        else {
            const float wv = w ? w[slot] : 1.f;
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < E; q++) { const float t = en[q] - eo[q]; s = fmaf(t, t, s); }
            cf = wv / sqrtf(fmaf(wv, s, REG_EPS));
        }
#pragma unroll
        for (int q = 0; q < E; q++) { d[q] = en[q] - eo[q]; acc[q] = fmaf(cf, d[q], acc[q]); }
    };
    if (in) {
        for (uint32_t j = sub; j < k; j += REG_BWD_LANES) {
            const int32_t m = idx[n * k + j];
            if ((uint32_t)m < N) pair((uint32_t)m, n * k + j);
        }
        const uint32_t r0 = (uint32_t)rev_start[n], r1 = (uint32_t)rev_start[n + 1];
        for (uint32_t t = r0 + sub; t < r1; t += REG_BWD_LANES) {
            const uint32_t slot = (uint32_t)rev_slot[t];
            if (slot < N * k) pair(slot / k, slot);
        }
    }
#pragma unroll
    for (int q = 0; q < E; q++) {
#pragma unroll
        for (int o = 1; o < REG_BWD_LANES; o <<= 1) acc[q] += __shfl_xor(acc[q], o);
    }
    if (!in) return;
    const float scale = g[0] * inv_pairs[0];
    // the group's lanes share the row's stores: lane `sub` writes the floats sub, sub + 8, ...
#pragma unroll
    for (int q = 0; q < E; q++) {
        if ((q % REG_BWD_LANES) == (int)sub) {
            const size_t o = (size_t)n * E + q;
            const float v = scale * acc[q];
            grad_e[o] = accumulate ? grad_e[o] + v : v;
        }
    }
}

struct KnnWs {
    float* partial; float* aabb; uint32_t* keys; uint32_t* kbuf[2]; uint32_t* vbuf[2]; uint32_t* hist; uint32_t* count;
    float4* sp; float4* leaf_box; float4* group_box;
    uint32_t num_groups_cap;
    size_t bytes;
};

void knn_carve(void* base, int N, KnnWs* w) {
    char* p = (char*)base;
    size_t off = 0;
    const size_t n = (size_t)(N > 0 ? N : 1);
    const size_t leaves = (n + KNN_LEAF - 1) / KNN_LEAF, groups = (leaves + KNN_GROUP - 1) / KNN_GROUP;
    w->num_groups_cap = (uint32_t)groups;
    auto take = [&](size_t bytes) { char* q = p + off; off = emd_align_up(off + bytes, 256); return q; };
    w->partial = (float*)take(KNN_BOUNDS_BLOCKS * 6 * sizeof(float));
    w->aabb = (float*)take(8 * sizeof(float));
    w->count = (uint32_t*)take(16);
    w->keys = (uint32_t*)take(n * 4);
    for (int i = 0; i < 2; i++) w->kbuf[i] = (uint32_t*)take(n * 4);
    for (int i = 0; i < 2; i++) w->vbuf[i] = (uint32_t*)take(n * 4);
    w->hist = (uint32_t*)take(((n + EMD_SORT_TILE - 1) / EMD_SORT_TILE) * EMD_RADIX_BINS * 4);
    w->sp = (float4*)take(groups * KNN_GROUP * KNN_LEAF * sizeof(float4));
    w->leaf_box = (float4*)take(groups * KNN_GROUP * 2 * sizeof(float4));
    w->group_box = (float4*)take(groups * 2 * sizeof(float4));
    w->bytes = off + 256;
}

struct RevWs { uint32_t* kbuf[2]; uint32_t* vbuf; uint32_t* hist; uint32_t* count; size_t bytes; };

void rev_carve(void* base, size_t total, RevWs* w) {
    char* p = (char*)base;
    size_t off = 0;
    const size_t n = total > 0 ? total : 1;
    auto take = [&](size_t bytes) { char* q = p + off; off = emd_align_up(off + bytes, 256); return q; };
    w->count = (uint32_t*)take(16);
    for (int i = 0; i < 2; i++) w->kbuf[i] = (uint32_t*)take(n * 4);
    w->vbuf = (uint32_t*)take(n * 4);
    w->hist = (uint32_t*)take(((n + EMD_SORT_TILE - 1) / EMD_SORT_TILE) * EMD_RADIX_BINS * 4);
    w->bytes = off + 256;
}

bool knn_sizes_ok(int32_t N, int32_t k) { return N >= 0 && k >= 1 && k <= EMD_KNN_MAX_K && (int64_t)N * k < ((int64_t)1 << 31) - EMD_SORT_TILE; }

}  // namespace

extern "C" size_t emd_knn_workspace(int32_t num_points, int32_t k) {
    if (!knn_sizes_ok(num_points, k)) return 0;
    KnnWs w;
    knn_carve(nullptr, num_points, &w);
    return w.bytes;
}

extern "C" int emd_knn(int32_t num_points, int32_t k, const float* pts, int32_t* idx, float* d2, float* mean_d2, void* workspace, size_t workspace_bytes,
                       void* hip_stream) {
    if (!knn_sizes_ok(num_points, k)) { emd_set_error("knn: bad sizes (num_points=%d, k=%d; 1 <= k <= %d)", num_points, k, EMD_KNN_MAX_K); return EMD_ERR_INVALID; }
    if (num_points == 0) return EMD_OK;
    if (!pts || (!idx && !d2 && !mean_d2)) { emd_set_error("knn: null points / no output"); return EMD_ERR_INVALID; }
    if (!workspace || workspace_bytes < emd_knn_workspace(num_points, k)) { emd_set_error("knn: workspace too small"); return EMD_ERR_WORKSPACE; }
    if ((uintptr_t)workspace & 15) { emd_set_error("knn: workspace must be 16-byte aligned"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    const int N = num_points;
    KnnWs w;
    knn_carve(workspace, N, &w);
    const unsigned nb = (unsigned)((N + EMD_BLOCK - 1) / EMD_BLOCK), pb = nb < KNN_BOUNDS_BLOCKS ? nb : KNN_BOUNDS_BLOCKS;
    hipLaunchKernelGGL(k_knn_bounds_partial, dim3(pb), dim3(EMD_BLOCK), 0, st, N, pts, w.partial);
    EMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_knn_bounds_final, dim3(1), dim3(EMD_BLOCK), 0, st, (int)pb, w.partial, w.aabb);
    EMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_knn_keys, dim3(nb), dim3(EMD_BLOCK), 0, st, N, k, pts, w.aabb, w.keys, idx, d2, mean_d2);
    EMD_LAUNCH_CHECK();
    RadixSortArgs zs;                                       // compacting: the keys of the non-finite points are all ones
    zs.keys_in = w.keys;
    for (int i = 0; i < 2; i++) { zs.keys[i] = w.kbuf[i]; zs.vals[i] = w.vbuf[i]; }
    zs.hist = w.hist;
    zs.n_cap = (size_t)N;
    zs.passes = KNN_SORT_PASSES;
    zs.count_out = w.count;
    const int zbuf = emd_launch_radix_sort(zs, st);
    if (zbuf < 0) return zbuf;
    const uint32_t* perm = w.vbuf[zbuf];
    const unsigned leaf_blocks = w.num_groups_cap * KNN_GROUP / (EMD_BLOCK / 64);      // one wave per leaf
    hipLaunchKernelGGL(k_knn_leaves, dim3(leaf_blocks), dim3(EMD_BLOCK), 0, st, pts, perm, w.count, w.sp, w.leaf_box);
    EMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_knn_groups, dim3((w.num_groups_cap + 3) / 4), dim3(EMD_BLOCK), 0, st, w.num_groups_cap, w.leaf_box, w.group_box);
    EMD_LAUNCH_CHECK();
#define KNN_SEARCH(KK) hipLaunchKernelGGL((k_knn_search<KK>), dim3(leaf_blocks), dim3(EMD_BLOCK), 0, st, (int)k, w.count, w.sp, w.leaf_box, w.group_box, idx, d2, mean_d2)
    if (k <= 3) KNN_SEARCH(3);
    else if (k <= 8) KNN_SEARCH(8);
    else if (k <= 20) KNN_SEARCH(20);
    else KNN_SEARCH(32);
#undef KNN_SEARCH
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_knn_segments(int32_t num_points, int32_t num_segments, int32_t k, const float* pts, const int32_t* segment_start, int32_t* idx,
                                float* d2, void* hip_stream) {
    if (!knn_sizes_ok(num_points, k)) { emd_set_error("knn_segments: bad sizes (num_points=%d, k=%d; 1 <= k <= %d)", num_points, k, EMD_KNN_MAX_K); return EMD_ERR_INVALID; }
    if (num_segments < 0 || num_segments >= INT32_MAX - 1) { emd_set_error("knn_segments: bad num_segments %d", num_segments); return EMD_ERR_INVALID; }
    if (num_points == 0) return EMD_OK;
    if (!pts || (!idx && !d2)) { emd_set_error("knn_segments: null points / no output"); return EMD_ERR_INVALID; }
    if (!segment_start) { emd_set_error("knn_segments: null segment_start (it holds num_segments + 1 entries)"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    const unsigned blocks = (unsigned)(((size_t)num_points + EMD_BLOCK - 1) / EMD_BLOCK);       // a wave per 64 consecutive rows
#define KNN_SEG(KK) hipLaunchKernelGGL((k_knn_segments<KK>), dim3(blocks), dim3(EMD_BLOCK), 0, st, (int)num_points, (int)num_segments, (int)k, pts, segment_start, idx, d2)
    if (k <= 3) KNN_SEG(3);
    else if (k <= 8) KNN_SEG(8);
    else if (k <= 20) KNN_SEG(20);
    else KNN_SEG(32);
#undef KNN_SEG
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" size_t emd_knn_reverse_workspace(int32_t num_points, int32_t k) {
    if (!knn_sizes_ok(num_points, k)) return 0;
    RevWs w;
    rev_carve(nullptr, (size_t)num_points * k, &w);
    return w.bytes;
}

extern "C" int emd_knn_reverse(int32_t num_points, int32_t k, const int32_t* idx, int32_t* rev_start, int32_t* rev_slot, void* workspace,
                               size_t workspace_bytes, void* hip_stream) {
    if (!knn_sizes_ok(num_points, k)) { emd_set_error("knn_reverse: bad sizes (num_points=%d, k=%d)", num_points, k); return EMD_ERR_INVALID; }
    if (!rev_start) { emd_set_error("knn_reverse: null rev_start"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    if (num_points == 0) return emd_zero_async(rev_start, sizeof(int32_t), st);
    if (!idx || !rev_slot) { emd_set_error("knn_reverse: null idx / rev_slot"); return EMD_ERR_INVALID; }
    if (!workspace || workspace_bytes < emd_knn_reverse_workspace(num_points, k)) { emd_set_error("knn_reverse: workspace too small"); return EMD_ERR_WORKSPACE; }
    const uint32_t total = (uint32_t)num_points * (uint32_t)k;
    RevWs w;
    rev_carve(workspace, total, &w);
    int bits = 1;
    while (((int64_t)1 << bits) < num_points) bits++;
    const int passes = (bits + 7) / 8;
    // the values of the last pass are the answer: lay the ping-pong out so that it writes them into rev_slot
    const int last = emd_radix_result_buf(true, passes);
    // a stable sort of (target, flat position) by target: positions ascend inside every target, entries < 0 (all ones) are dropped
    RadixSortArgs rs;
    rs.keys_in = (const uint32_t*)idx;
    for (int i = 0; i < 2; i++) { rs.keys[i] = w.kbuf[i]; rs.vals[i] = i == last ? (uint32_t*)rev_slot : w.vbuf; }
    rs.hist = w.hist;
    rs.n_cap = (size_t)total;
    rs.passes = passes;
    rs.count_out = w.count;
    const int rbuf = emd_launch_radix_sort(rs, st);          // (== last)
    if (rbuf < 0) return rbuf;
    hipLaunchKernelGGL(k_knn_rev_start, dim3((unsigned)(((size_t)total + 1 + EMD_BLOCK - 1) / EMD_BLOCK)), dim3(EMD_BLOCK), 0, st, (int)num_points, total,
                       w.kbuf[rbuf], w.count, rev_start);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

static int embed_reg_check(const char* who, int32_t N, int32_t k, int32_t E, const float* e, const int32_t* idx) {
    if (!knn_sizes_ok(N, k)) { emd_set_error("%s: bad sizes (num_points=%d, k=%d)", who, N, k); return EMD_ERR_INVALID; }
    if (E != 4 && E != 8 && E != 16 && E != 32) { emd_set_error("%s: embed_dim %d is not one of 4, 8, 16, 32", who, E); return EMD_ERR_INVALID; }
    if (N > 0 && (!e || !idx)) { emd_set_error("%s: null embedding / idx", who); return EMD_ERR_INVALID; }
    if ((uintptr_t)e & 15) { emd_set_error("%s: the embedding must be 16-byte aligned", who); return EMD_ERR_INVALID; }
    return EMD_OK;
}

extern "C" int emd_embed_reg_forward(int32_t num_points, int32_t k, int32_t embed_dim, const float* e, const int32_t* idx, const float* w, float* c,
                                     float* loss, uint32_t* scratch, void* hip_stream) {
    int rc = embed_reg_check("embed_reg_forward", num_points, k, embed_dim, e, idx);
    if (rc) return rc;
    if (!loss || !scratch) { emd_set_error("embed_reg_forward: null loss / scratch"); return EMD_ERR_INVALID; }
    if ((uintptr_t)scratch & 7) { emd_set_error("embed_reg_forward: scratch must be 8-byte aligned"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t total = (size_t)num_points * k;
    size_t blocks = (total + REG_THREADS - 1) / REG_THREADS;
    if (blocks < 1) blocks = 1;
    if (blocks > REG_MAX_BLOCKS) blocks = REG_MAX_BLOCKS;
#define REG_FWD(EE) hipLaunchKernelGGL((k_embed_reg_fwd<EE>), dim3((unsigned)blocks), dim3(REG_THREADS), 0, st, (uint32_t)num_points, (uint32_t)k, e, idx, w, c, loss, scratch)
    switch (embed_dim) { case 4: REG_FWD(4); break; case 8: REG_FWD(8); break; case 16: REG_FWD(16); break; default: REG_FWD(32); break; }
#undef REG_FWD
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_embed_reg_backward(int32_t num_points, int32_t k, int32_t embed_dim, const float* e, const int32_t* idx, const float* w, const float* c,
                                      const int32_t* rev_start, const int32_t* rev_slot, const float* g, const float* inv_pairs, float* grad_e,
                                      int32_t accumulate, void* hip_stream) {
    int rc = embed_reg_check("embed_reg_backward", num_points, k, embed_dim, e, idx);
    if (rc) return rc;
    if (num_points == 0) return EMD_OK;
    if (!rev_start || !rev_slot || !g || !inv_pairs || !grad_e) { emd_set_error("embed_reg_backward: null rev_start / rev_slot / g / inv_pairs / grad_e"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    const unsigned rows = EMD_BLOCK / REG_BWD_LANES, blocks = (unsigned)((num_points + rows - 1) / rows);
#define REG_BWD(EE) hipLaunchKernelGGL((k_embed_reg_bwd<EE>), dim3(blocks), dim3(EMD_BLOCK), 0, st, (uint32_t)num_points, (uint32_t)k, e, idx, w, c, rev_start, rev_slot, g, inv_pairs, grad_e, (int)(accumulate != 0))
    switch (embed_dim) { case 4: REG_BWD(4); break; case 8: REG_BWD(8); break; case 16: REG_BWD(16); break; default: REG_BWD(32); break; }
#undef REG_BWD
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}
