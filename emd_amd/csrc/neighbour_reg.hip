// neighbour_reg.hip -- the k-NN regulariser of SMPLNodes (reg.knn_reg of omnire.yaml, after GART): the mean standard deviation of up to eight
// attribute blocks over each point's neighbour group, v[nn].std(dim=1).mean() * w per block.  The contract is in include/emd_raster.h
// (EmdNeighbourStdArgs); DESIGN.md section 8.19 has the launch shape, the rounding count and the measurements.
//
//   k_neighbour_std_fwd   one launch: a lane owns one column of one point, neighbouring lanes the neighbouring columns of the same point, so
//                         every gathered row is read as one contiguous piece per block.  The lane forms the group's differences to its first
//                         member (the point itself), their mean and their standard deviation, and leaves (mu, 1 / ((g - 1) sigma)) in the stash.
//                         The sigmas leave every workgroup as one fp64 partial per block; the LAST workgroup to take a ticket (an integer
//                         counter: nobody waits for anybody) adds the partials in workgroup order and writes the terms.
//   k_neighbour_std_bwd   one launch, a gather: the groups that contain j are j's own and the owners of rev(j)'s slots, in that order; every
//                         gradient element is written once.
// No float atomics; the unit is built with -ffp-contract=off: the operation order of the contract is the order of the source.
#include "common.h"
#include "device_utils.h"

#include <math.h>

namespace {

#define NS_MAX_GRID 2048                       // workgroups of the forward = rows of the partial table
#define NS_HEAD_BYTES 256                      // the ticket counter's own region in front of the partials

// the lanes of a wave in one xor tree: every lane ends with the same bits (the tree of fixed_sum.h, whose includers are the units with a finalize
// kernel of their own; this unit's sums end in its forward kernel)
__device__ __forceinline__ double ns_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// the active blocks (weight != 0), compacted; first[] is padded with the column total so that a search over all entries needs no count
struct NsTab {
    const float* x[EMD_NSTD_MAX_BLOCKS];
    float* dx[EMD_NSTD_MAX_BLOCKS];
    int32_t first[EMD_NSTD_MAX_BLOCKS + 1], cols[EMD_NSTD_MAX_BLOCKS], act[EMD_NSTD_MAX_BLOCKS], orig[EMD_NSTD_MAX_BLOCKS];
    float weight[EMD_NSTD_MAX_BLOCKS];
    int32_t num_active, num_blocks, total_cols, reserved;
};

__device__ __forceinline__ float ns_act(float x, int a) {
    if (a == EMD_NSTD_ACT_EXP) return expf(x);
    if (a == EMD_NSTD_ACT_SIGMOID) return 1.f / (1.f + expf(-x));
    return x;
}
__device__ __forceinline__ float ns_act_grad(float v, int a) {          // da/dx from the activated value
    if (a == EMD_NSTD_ACT_EXP) return v;
    if (a == EMD_NSTD_ACT_SIGMOID) return v * (1.f - v);
    return 1.f;
}

// which (row of the pass, column) a thread owns: Tp = min(T, 256) columns per pass and chunk, 256 / Tp rows per pass
struct NsLane { int r, tl, Tp, rpp; bool on; };
__device__ __forceinline__ NsLane ns_lane(int T) {
    NsLane l;
    l.Tp = min(T, EMD_BLOCK);
    l.rpp = EMD_BLOCK / l.Tp;
    l.r = (int)threadIdx.x / l.Tp;
    l.tl = (int)threadIdx.x % l.Tp;
    l.on = l.r < l.rpp;
    return l;
}
__device__ __forceinline__ int ns_block_of(const NsTab& t, int col) {
    int p = 0;
#pragma unroll
    for (int i = 1; i < EMD_NSTD_MAX_BLOCKS; i++) p += col >= t.first[i] ? 1 : 0;      // (first[] never decreases)
    return p;
}

template <int KK>
__global__ void __launch_bounds__(EMD_BLOCK) k_neighbour_std_fwd(NsTab t, int N, int k, int rows_per_wg, const int32_t* __restrict__ idx,
                                                                 float2* __restrict__ stash, unsigned long long* __restrict__ partials,
                                                                 unsigned int* __restrict__ ticket, float* __restrict__ terms) {
    __shared__ double sm[EMD_BLOCK / EMD_WAVE][EMD_NSTD_MAX_BLOCKS];
    __shared__ unsigned int s_last;
    const int T = t.total_cols;
    const NsLane l = ns_lane(T);
    const int p0 = (int)min((long long)blockIdx.x * rows_per_wg, (long long)N), p1 = (int)min((long long)p0 + rows_per_wg, (long long)N);
    double total = 0.0;                           // thread b < num_active: the workgroup's sum of block b, chunk after chunk
    for (int c0 = 0; c0 < T; c0 += l.Tp) {
        const int col = c0 + l.tl;
        const bool on = l.on && col < T;
        const int b = ns_block_of(t, on ? col : 0);
        const int C = t.cols[b], c = (on ? col : 0) - t.first[b], a = t.act[b];
        const float* __restrict__ x = t.x[b];
        double acc = 0.0;
        if (on) {
            for (int n = p0 + l.r; n < p1; n += l.rpp) {
                int m[KK];
#pragma unroll
                for (int j = 0; j < KK; j++) m[j] = j < k ? idx[(size_t)n * k + j] : -1;
                const float vn = ns_act(x[(size_t)n * C + c], a);
                float d[KK];
                int g = 1;
#pragma unroll
                for (int j = 0; j < KK; j++) {
                    const bool has = (unsigned)m[j] < (unsigned)N;
                    d[j] = has ? ns_act(x[(size_t)m[j] * C + c], a) - vn : 0.f;
                    m[j] = has ? 1 : 0;
                    g += m[j];
                }
                float mu = 0.f, inv = 0.f;
                if (g >= 2) {
                    float s = 0.f;                   // (the point itself: d = 0)
#pragma unroll
                    for (int j = 0; j < KK; j++)
                        if (m[j]) s = s + d[j];
                    mu = s / (float)g;
                    float q = (0.f - mu) * (0.f - mu);
#pragma unroll
                    for (int j = 0; j < KK; j++)
                        if (m[j]) { const float e = d[j] - mu; q = q + e * e; }
                    const float sigma = sqrtf(q / (float)(g - 1));
                    acc += (double)sigma;
                    inv = sigma > 0.f ? 1.f / ((float)(g - 1) * sigma) : 0.f;
                }
                stash[(size_t)n * T + col] = make_float2(mu, inv);
            }
        }
        // the chunk's sums per block: lanes in a fixed tree, the four waves left to right, chunks in ascending order
#pragma unroll
        for (int q = 0; q < EMD_NSTD_MAX_BLOCKS; q++) {
            const double s = ns_wave_sum(on && b == q ? acc : 0.0);
            if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][q] = s;
        }
        __syncthreads();
        if (threadIdx.x < EMD_NSTD_MAX_BLOCKS) total += (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
        __syncthreads();
    }
    // publish (wave 0 alone): 8-byte write-through stores, drained by the wave that made them before its lane 0 takes the ticket -- no release
    // fence, which would write the stash rows back from the L2 as well; the last workgroup reads the partials with agent-scope loads
    if (threadIdx.x < EMD_WAVE) {
        if (threadIdx.x < EMD_NSTD_MAX_BLOCKS)
            __hip_atomic_store(partials + (size_t)blockIdx.x * EMD_NSTD_MAX_BLOCKS + threadIdx.x, (unsigned long long)__double_as_longlong(total),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#pragma unroll 1
    for (int q = 0; q < t.num_active; q++) {
        double s = 0.0;
        for (unsigned i = threadIdx.x; i < gridDim.x; i += EMD_BLOCK)
            s += __longlong_as_double((long long)__hip_atomic_load(partials + (size_t)i * EMD_NSTD_MAX_BLOCKS + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        s = ns_wave_sum(s);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][q] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < t.num_blocks) terms[threadIdx.x] = 0.f;         // (skipped blocks: value 0)
    __syncthreads();
    if ((int)threadIdx.x < t.num_active) {
        const double s = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
        terms[t.orig[threadIdx.x]] = (float)((double)t.weight[threadIdx.x] * s / ((double)N * (double)t.cols[threadIdx.x]));
    }
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // zero again for the next call
}

__global__ void __launch_bounds__(EMD_BLOCK) k_neighbour_std_bwd(NsTab t, int N, int k, const float2* __restrict__ stash, const int32_t* __restrict__ rev_start,
                                                                 const int32_t* __restrict__ rev_slot, const float* __restrict__ g_terms) {
    const int T = t.total_cols;
    const NsLane l = ns_lane(T);
    const long long jl = (long long)blockIdx.x * l.rpp + l.r;
    if (!l.on || jl >= N) return;
    const int j = (int)jl;
    const unsigned r0 = (unsigned)rev_start[j], r1 = (unsigned)rev_start[j + 1], slots = (unsigned)N * (unsigned)k;
    for (int c0 = 0; c0 < T; c0 += l.Tp) {
        const int col = c0 + l.tl;
        if (col >= T) break;
        const int b = ns_block_of(t, col);
        const int C = t.cols[b], c = col - t.first[b], a = t.act[b];
        const float* __restrict__ x = t.x[b];
        const float vj = ns_act(x[(size_t)j * C + c], a);
        const float2 own = stash[(size_t)j * T + col];
        float acc = (0.f - own.x) * own.y;                                  // j in its own group: d = 0
        for (unsigned s = r0; s < r1; s++) {
            const unsigned slot = (unsigned)rev_slot[s];
            if (slot >= slots) continue;
            const unsigned m = slot / (unsigned)k;
            const float2 st = stash[(size_t)m * T + col];
            const float d = vj - ns_act(x[(size_t)m * C + c], a);
            acc = acc + (d - st.x) * st.y;
        }
        const float scale = (float)((double)g_terms[t.orig[b]] * (double)t.weight[b] / ((double)N * (double)C));
        t.dx[b][(size_t)j * C + c] = ns_act_grad(vj, a) * (scale * acc);
    }
}

// Validates, compacts the active blocks.  Returns the number of active columns, or a negative code.
int ns_build(const EmdNeighbourStdArgs* a, bool backward, NsTab* t, const char* who) {
    if (!a) { emd_set_error("%s: null args", who); return EMD_ERR_INVALID; }
    if (a->num_points < 0 || a->k < 1 || a->k > EMD_KNN_MAX_K || (int64_t)a->num_points * a->k >= ((int64_t)1 << 31)) {
        emd_set_error("%s: bad sizes (num_points=%d, k=%d; 1 <= k <= %d)", who, a->num_points, a->k, EMD_KNN_MAX_K);
        return EMD_ERR_INVALID;
    }
    if (a->num_blocks < 1 || a->num_blocks > EMD_NSTD_MAX_BLOCKS) {
        emd_set_error("%s: num_blocks %d is outside 1 .. %d", who, a->num_blocks, EMD_NSTD_MAX_BLOCKS);
        return EMD_ERR_INVALID;
    }
    int n = 0, total = 0;
    for (int b = 0; b < a->num_blocks; b++) {
        if (a->cols[b] < 1 || a->cols[b] > EMD_NSTD_MAX_COLS) {
            emd_set_error("%s: block %d has %d columns, outside 1 .. %d", who, b, a->cols[b], EMD_NSTD_MAX_COLS);
            return EMD_ERR_INVALID;
        }
        if (a->act[b] != EMD_NSTD_ACT_IDENTITY && a->act[b] != EMD_NSTD_ACT_EXP && a->act[b] != EMD_NSTD_ACT_SIGMOID) {
            emd_set_error("%s: block %d has the unknown activation code %d", who, b, a->act[b]);
            return EMD_ERR_INVALID;
        }
        if (!(a->weight[b] == a->weight[b])) { emd_set_error("%s: the weight of block %d is NaN", who, b); return EMD_ERR_INVALID; }
        if (a->weight[b] == 0.f) continue;
        if (a->num_points > 0 && (!a->x[b] || (backward && !a->dx[b]))) {
            emd_set_error("%s: null %s of block %d", who, a->x[b] ? "gradient" : "values", b);
            return EMD_ERR_INVALID;
        }
        t->x[n] = a->x[b]; t->dx[n] = backward ? a->dx[b] : nullptr;
        t->first[n] = total; t->cols[n] = a->cols[b]; t->act[n] = a->act[b]; t->orig[n] = b; t->weight[n] = a->weight[b];
        total += a->cols[b];
        n++;
    }
    for (int i = n; i <= EMD_NSTD_MAX_BLOCKS; i++) t->first[i] = total;
    for (int i = n; i < EMD_NSTD_MAX_BLOCKS; i++) { t->x[i] = nullptr; t->dx[i] = nullptr; t->cols[i] = 1; t->act[i] = 0; t->orig[i] = 0; t->weight[i] = 0.f; }
    t->num_active = n; t->num_blocks = a->num_blocks; t->total_cols = total; t->reserved = 0;
    if (a->num_points > 0 && n > 0 && (!a->idx || !a->stash)) { emd_set_error("%s: null idx / stash", who); return EMD_ERR_INVALID; }
    if ((uintptr_t)a->stash & 7) { emd_set_error("%s: the stash must be 8-byte aligned", who); return EMD_ERR_INVALID; }
    return total;
}

}  // namespace

extern "C" size_t emd_neighbour_std_workspace_size(void) { return NS_HEAD_BYTES + (size_t)NS_MAX_GRID * EMD_NSTD_MAX_BLOCKS * sizeof(double); }

extern "C" int emd_neighbour_std_forward(const EmdNeighbourStdArgs* a, void* workspace, size_t workspace_bytes, void* hip_stream) {
    NsTab t;
    const int T = ns_build(a, false, &t, "neighbour_std_forward");
    if (T < 0) return T;
    if (!a->terms) { emd_set_error("neighbour_std_forward: null terms"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    if (a->num_points == 0 || T == 0) return emd_zero_async(a->terms, (size_t)a->num_blocks * sizeof(float), st);
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < emd_neighbour_std_workspace_size()) {
        emd_set_error("neighbour_std_forward: workspace missing, misaligned or smaller than emd_neighbour_std_workspace_size()");
        return EMD_ERR_WORKSPACE;
    }
    const int N = a->num_points, Tp = T < EMD_BLOCK ? T : EMD_BLOCK, rpp = EMD_BLOCK / Tp;
    int64_t grid = ((int64_t)N + rpp - 1) / rpp;
    if (grid > NS_MAX_GRID) grid = NS_MAX_GRID;
    const int rows_per_wg = (int)(((int64_t)N + grid - 1) / grid);
    grid = ((int64_t)N + rows_per_wg - 1) / rows_per_wg;                       // no workgroup without rows
    unsigned int* ticket = (unsigned int*)workspace;
    unsigned long long* partials = (unsigned long long*)((char*)workspace + NS_HEAD_BYTES);
#define NS_FWD(KK) hipLaunchKernelGGL((k_neighbour_std_fwd<KK>), dim3((unsigned)grid), dim3(EMD_BLOCK), 0, st, t, N, (int)a->k, rows_per_wg, a->idx, (float2*)a->stash, partials, ticket, a->terms)
    if (a->k <= 2) NS_FWD(2);
    else if (a->k <= 8) NS_FWD(8);
    else NS_FWD(32);
#undef NS_FWD
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_neighbour_std_backward(const EmdNeighbourStdArgs* a, void* hip_stream) {
    NsTab t;
    const int T = ns_build(a, true, &t, "neighbour_std_backward");
    if (T < 0) return T;
    if (a->num_points == 0 || T == 0) return EMD_OK;
    if (!a->rev_start || !a->rev_slot || !a->g_terms) { emd_set_error("neighbour_std_backward: null rev_start / rev_slot / g_terms"); return EMD_ERR_INVALID; }
    const int N = a->num_points, Tp = T < EMD_BLOCK ? T : EMD_BLOCK, rpp = EMD_BLOCK / Tp;
    const int64_t grid = ((int64_t)N + rpp - 1) / rpp;
    hipLaunchKernelGGL(k_neighbour_std_bwd, dim3((unsigned)grid), dim3(EMD_BLOCK), 0, (hipStream_t)hip_stream, t, N, (int)a->k, (const float2*)a->stash,
                       a->rev_start, a->rev_slot, a->g_terms);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}
