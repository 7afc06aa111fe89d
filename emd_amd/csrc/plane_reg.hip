// plane_reg.hip -- the HexPlane regularisers of the fine stage (compute_regulation, S3Gaussian/scene/gaussian_model.py:745-784): the second-difference
// smoothness of the spatial planes (plane TV) and of the time planes (time smoothness), and the L1 pull of the time planes towards 1.  The contract
// is in include/emd_raster.h (EmdPlaneRegArgs); DESIGN.md section 8.12 has the launch shape and the measurements.
//
// A plane is [H][W][C] floats, so the second difference along H couples elements R = W * C floats apart: the plane is an [H][R] matrix and the
// stencil runs down its columns.  One workgroup owns EMD_PLANE_REG_SEG rows x PR_CHUNK columns of ONE plane; a lane owns PR_COLS consecutive
// columns and walks down the rows with the window (x[h], x[h+1], d1[h], and backward d2[h-1], d2[h-2]) in registers, PR_BATCH rows requested
// before the first is used.  Every load is contiguous across the wave; 16-byte aligned planes with R % 4 == 0 take dwordx4 loads and stores, any
// other plane the same walk with dword accesses and a masked tail.
//   k_plane_reg_forward   all planes of all scales: every element read once (+ 2 halo rows per segment); per lane fp32 sums of at most
//                         EMD_PLANE_REG_SEG terms per accumulator, fp64 from there on; one (smooth, l1) pair of doubles per workgroup
//   k_plane_reg_finalize  one workgroup: a plane's pairs added in ascending workgroup order, the planes in ascending order, four floats out
//   k_plane_reg_backward  all planes: every element read once (+ 4 halo rows per segment), every gradient element written once
// No atomics anywhere: every output is a fixed function of the inputs.
#include "common.h"
#include "device_utils.h"
#include "fixed_sum.h"

namespace {

#define PR_MAX_PLANES (EMD_HEX_MAX_SCALES * 6)
#define PR_COLS 4                              // floats of a row per lane
#define PR_CHUNK (EMD_BLOCK * PR_COLS)         // columns per workgroup
#define PR_BATCH 8                             // rows in flight per lane
#define PR_FINAL_THREADS 1024
static_assert(EMD_PLANE_REG_SEG % PR_BATCH == 0, "a segment is whole batches");

// What the kernels read per plane; built on the host (pr_build), passed by value.  A plane's workgroups are first[p] .. first[p + 1] - 1, the column
// chunk running fastest; first[] is padded with the total so that a search over all PR_MAX_PLANES entries needs no count.
struct PlaneTab {
    const float* x[PR_MAX_PLANES];
    float* dx[PR_MAX_PLANES];
    int32_t H[PR_MAX_PLANES], R[PR_MAX_PLANES];
    int32_t first[PR_MAX_PLANES + 1];
    float w_smooth[PR_MAX_PLANES], w_l1[PR_MAX_PLANES];       // the term's weight (backward)
    int32_t num_planes, reserved;
};

struct F4 { float v[PR_COLS]; };

__device__ __forceinline__ bool pr_is_time(int p) { const int k = p % 6; return k == 2 || k == 4 || k == 5; }

// row h of the lane's columns j .. j + 3 (j < R).  A row outside the plane and the columns past R read as `fill` without touching memory.
template <bool VEC>
__device__ __forceinline__ F4 pr_row(const float* __restrict__ x, int h, int H, int R, int j, float fill) {
    F4 r;
    if (h < 0 || h >= H) {
#pragma unroll
        for (int c = 0; c < PR_COLS; c++) r.v[c] = fill;
        return r;
    }
    const float* __restrict__ row = x + (size_t)h * R + j;
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(row);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
#pragma unroll
        for (int c = 0; c < PR_COLS; c++) r.v[c] = j + c < R ? row[c] : fill;
    }
    return r;
}

template <bool VEC>
__device__ __forceinline__ void pr_store(float* __restrict__ dx, int h, int R, int j, const F4& o) {
    float* __restrict__ row = dx + (size_t)h * R + j;
    if (VEC) {
        *reinterpret_cast<float4*>(row) = make_float4(o.v[0], o.v[1], o.v[2], o.v[3]);
    } else {
#pragma unroll
        for (int c = 0; c < PR_COLS; c++)
            if (j + c < R) row[c] = o.v[c];
    }
}

// which plane, segment and column chunk a workgroup owns
struct PrTask { int p, H, R, h0, h1, j; };
__device__ __forceinline__ PrTask pr_task(const PlaneTab& t) {
    const int task = blockIdx.x;
    int p = 0;
#pragma unroll
    for (int i = 1; i < PR_MAX_PLANES; i++) p += task >= t.first[i] ? 1 : 0;      // (first[] never decreases)
    PrTask k;
    k.p = p; k.H = t.H[p]; k.R = t.R[p];
    const int chunks = (k.R + PR_CHUNK - 1) / PR_CHUNK, local = task - t.first[p];
    k.h0 = (local / chunks) * EMD_PLANE_REG_SEG;
    k.h1 = min(k.h0 + EMD_PLANE_REG_SEG, k.H);
    k.j = (local % chunks) * PR_CHUNK + threadIdx.x * PR_COLS;
    return k;
}
__device__ __forceinline__ bool pr_wide(const void* a, const void* b, int R) {
    return (R & 3) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

// rows [h0, h1) of the lane's columns: s2 += d2[h]^2 for the h with h + 2 < H, s1 += |1 - x[h]| (time planes).  Columns past R read as 1: both terms 0.
template <bool VEC, bool TIME>
__device__ __forceinline__ void pr_forward_rows(const float* __restrict__ x, const PrTask& k, F4& s2, F4& s1) {
    F4 xa = pr_row<VEC>(x, k.h0, k.H, k.R, k.j, 1.f), xb = pr_row<VEC>(x, k.h0 + 1, k.H, k.R, k.j, 1.f), d1;
#pragma unroll
    for (int c = 0; c < PR_COLS; c++) d1.v[c] = xb.v[c] - xa.v[c];
    for (int hb = k.h0; hb < k.h1; hb += PR_BATCH) {
        F4 xn[PR_BATCH];
#pragma unroll
        for (int i = 0; i < PR_BATCH; i++) xn[i] = pr_row<VEC>(x, hb + i < k.h1 ? hb + i + 2 : -1, k.H, k.R, k.j, 1.f);
#pragma unroll
        for (int i = 0; i < PR_BATCH; i++) {
            const int h = hb + i;
            if (h < k.h1) {
                const bool has_d2 = h + 2 < k.H;
#pragma unroll
                for (int c = 0; c < PR_COLS; c++) {
                    const float d1n = xn[i].v[c] - xb.v[c];
                    const float d2 = d1n - d1.v[c];                 // the difference of differences, never the expanded polynomial
                    if (has_d2) s2.v[c] += d2 * d2;
                    if (TIME) s1.v[c] += fabsf(1.f - xa.v[c]);
                    xa.v[c] = xb.v[c]; xb.v[c] = xn[i].v[c]; d1.v[c] = d1n;
                }
            }
        }
    }
}

__device__ __forceinline__ double pr_lane_sum(const F4& s) { return ((double)s.v[0] + (double)s.v[1]) + ((double)s.v[2] + (double)s.v[3]); }

__global__ void __launch_bounds__(EMD_BLOCK) k_plane_reg_forward(PlaneTab t, double* __restrict__ partials) {
    __shared__ double sm[EMD_BLOCK / EMD_WAVE][2];
    const PrTask k = pr_task(t);
    const float* __restrict__ x = t.x[k.p];
    F4 s2 = {{0.f, 0.f, 0.f, 0.f}}, s1 = {{0.f, 0.f, 0.f, 0.f}};
    if (k.j < k.R) {
        const bool wide = pr_wide(x, nullptr, k.R), time = pr_is_time(k.p);
        if (wide) { if (time) pr_forward_rows<true, true>(x, k, s2, s1); else pr_forward_rows<true, false>(x, k, s2, s1); }
        else { if (time) pr_forward_rows<false, true>(x, k, s2, s1); else pr_forward_rows<false, false>(x, k, s2, s1); }
    }
    // (the four waves meet as in fixed_block_store, fixed_sum.h, but thread 0 stores both sums: through the template the kernel came out with other
    //  instructions, profiles/shared_source_isa.txt)
    const double a = fixed_wave_sum(pr_lane_sum(s2)), b = fixed_wave_sum(pr_lane_sum(s1));
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = a; sm[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[2 * (size_t)blockIdx.x] = (sm[0][0] + sm[1][0]) + (sm[2][0] + sm[3][0]);
        partials[2 * (size_t)blockIdx.x + 1] = (sm[0][1] + sm[1][1]) + (sm[2][1] + sm[3][1]);
    }
}

// One workgroup.  Wave w takes the planes w, w + 16, ...: lane l adds the plane's pairs l, l + 64, ... in ascending order, then the fixed tree.
__global__ void __launch_bounds__(PR_FINAL_THREADS) k_plane_reg_finalize(PlaneTab t, const double* __restrict__ partials, float w_tv, float w_ts,
                                                                         float w_l1, float* __restrict__ out) {
    __shared__ double smooth[PR_MAX_PLANES], l1[PR_MAX_PLANES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int p = wave; p < t.num_planes; p += PR_FINAL_THREADS / EMD_WAVE) {
        double a = 0.0, b = 0.0;
        for (int i = t.first[p] + lane; i < t.first[p + 1]; i += EMD_WAVE) { a += partials[2 * (size_t)i]; b += partials[2 * (size_t)i + 1]; }
        a = fixed_wave_sum(a); b = fixed_wave_sum(b);
        if (lane == 0) {
            const double R = (double)t.R[p], H = (double)t.H[p];
            smooth[p] = a / (R * (H - 2.0));
            l1[p] = b / (R * H);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tv = 0.0, ts = 0.0, tl = 0.0;
        for (int p = 0; p < t.num_planes; p++) {
            if (pr_is_time(p)) { ts += smooth[p]; tl += l1[p]; }
            else tv += smooth[p];
        }
        out[0] = (float)((double)w_tv * tv + (double)w_ts * ts + (double)w_l1 * tl);
        out[1] = (float)tv; out[2] = (float)ts; out[3] = (float)tl;
    }
}

// rows [h0, h1) of the lane's columns: dx[h] = ks ((d2[h] - d2[h-1]) - (d2[h-1] - d2[h-2])) + kl sign(x[h] - 1), d2 = 0 outside [0, H-3]
template <bool VEC, bool TIME>
__device__ __forceinline__ void pr_backward_rows(const float* __restrict__ x, float* __restrict__ dx, const PrTask& k, float ks, float kl) {
    const int H = k.H, R = k.R, j = k.j, h0 = k.h0;
    F4 xc = pr_row<VEC>(x, h0, H, R, j, 0.f), xm = pr_row<VEC>(x, h0 + 1, H, R, j, 0.f), d1, e1, e2;
    {
        const F4 xp2 = pr_row<VEC>(x, h0 - 2, H, R, j, 0.f), xp1 = pr_row<VEC>(x, h0 - 1, H, R, j, 0.f);
        const bool v2 = h0 - 2 >= 0 && h0 < H, v1 = h0 - 1 >= 0 && h0 + 1 < H;      // d2[h0-2], d2[h0-1] exist
#pragma unroll
        for (int c = 0; c < PR_COLS; c++) {
            const float d1pp = xp1.v[c] - xp2.v[c], d1p = xc.v[c] - xp1.v[c];
            d1.v[c] = xm.v[c] - xc.v[c];
            e2.v[c] = v2 ? d1p - d1pp : 0.f;
            e1.v[c] = v1 ? d1.v[c] - d1p : 0.f;
        }
    }
    for (int hb = h0; hb < k.h1; hb += PR_BATCH) {
        F4 xn[PR_BATCH];
#pragma unroll
        for (int i = 0; i < PR_BATCH; i++) xn[i] = pr_row<VEC>(x, hb + i < k.h1 ? hb + i + 2 : -1, H, R, j, 0.f);
#pragma unroll
        for (int i = 0; i < PR_BATCH; i++) {
            const int h = hb + i;
            if (h < k.h1) {
                const bool has_d2 = h + 2 < H;
                F4 o;
#pragma unroll
                for (int c = 0; c < PR_COLS; c++) {
                    const float d1n = xn[i].v[c] - xm.v[c];
                    const float d2 = has_d2 ? d1n - d1.v[c] : 0.f;
                    const float st = (d2 - e1.v[c]) - (e1.v[c] - e2.v[c]);
                    float g = ks * st;
                    if (TIME) g += kl * (xc.v[c] > 1.f ? 1.f : (xc.v[c] < 1.f ? -1.f : 0.f));      // sign(0) = 0: time planes start at exactly 1
                    o.v[c] = g;
                    e2.v[c] = e1.v[c]; e1.v[c] = d2; xc.v[c] = xm.v[c]; xm.v[c] = xn[i].v[c]; d1.v[c] = d1n;
                }
                pr_store<VEC>(dx, h, R, j, o);
            }
        }
    }
}

__global__ void __launch_bounds__(EMD_BLOCK) k_plane_reg_backward(PlaneTab t, const float* __restrict__ g) {
    const PrTask k = pr_task(t);
    if (k.j >= k.R) return;
    const float* __restrict__ x = t.x[k.p];
    float* __restrict__ dx = t.dx[k.p];
    const double up = (double)g[0], R = (double)k.R, H = (double)k.H;
    const float ks = (float)(up * (double)t.w_smooth[k.p] * (2.0 / (R * (H - 2.0))));
    const float kl = (float)(up * (double)t.w_l1[k.p] / (R * H));
    const bool wide = pr_wide(x, dx, k.R), time = pr_is_time(k.p);
    if (wide) { if (time) pr_backward_rows<true, true>(x, dx, k, ks, kl); else pr_backward_rows<true, false>(x, dx, k, ks, kl); }
    else { if (time) pr_backward_rows<false, true>(x, dx, k, ks, kl); else pr_backward_rows<false, false>(x, dx, k, ks, kl); }
}

const int PR_PAIRS[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};

// Validates the shapes and (with `pointers`) the plane pointers, fills the table.  Returns the number of workgroups, or a negative code.
int64_t pr_build(const EmdPlaneRegArgs* a, bool pointers, bool backward, PlaneTab* t, const char* who) {
    if (!a) { emd_set_error("%s: null args", who); return EMD_ERR_INVALID; }
    if (a->channels < 1 || a->num_scales < 1 || a->num_scales > EMD_HEX_MAX_SCALES) {
        emd_set_error("%s: bad sizes (channels %d, num_scales %d)", who, a->channels, a->num_scales);
        return EMD_ERR_INVALID;
    }
    int64_t total = 0;
    int p = 0;
    for (int s = 0; s < a->num_scales; s++) {
        for (int k = 0; k < 4; k++)
            if (a->res[s][k] < 1) { emd_set_error("%s: bad resolution %d on scale %d", who, a->res[s][k], s); return EMD_ERR_INVALID; }
        for (int q = 0; q < 6; q++, p++) {
            const int64_t W = a->res[s][PR_PAIRS[q][0]], H = a->res[s][PR_PAIRS[q][1]], R = W * a->channels;
            if (H < 3) {
                emd_set_error("%s: plane %d of scale %d has H = %d < 3: the second difference along H needs three rows", who, q, s, (int)H);
                return EMD_ERR_INVALID;
            }
            if (R > (1 << 28) || R * H >= ((int64_t)1 << 40)) { emd_set_error("%s: plane %d of scale %d is too large", who, q, s); return EMD_ERR_INVALID; }
            t->H[p] = (int32_t)H; t->R[p] = (int32_t)R;
            t->first[p] = (int32_t)total;
            total += ((R + PR_CHUNK - 1) / PR_CHUNK) * ((H + EMD_PLANE_REG_SEG - 1) / EMD_PLANE_REG_SEG);
            if (total >= ((int64_t)1 << 30)) { emd_set_error("%s: too many workgroups", who); return EMD_ERR_INVALID; }
            const bool time = q == 2 || q == 4 || q == 5;
            t->w_smooth[p] = time ? a->time_smoothness_weight : a->plane_tv_weight;
            t->w_l1[p] = time ? a->l1_time_planes_weight : 0.f;
            t->x[p] = a->planes[s][q];
            t->dx[p] = backward ? a->dL_dplanes[s][q] : nullptr;
            if (pointers) {
                if (!t->x[p] || (backward && !t->dx[p])) { emd_set_error("%s: null plane %d of scale %d", who, q, s); return EMD_ERR_INVALID; }
                if (((uintptr_t)t->x[p] | (uintptr_t)t->dx[p]) & 3) { emd_set_error("%s: plane %d of scale %d is not 4-byte aligned", who, q, s); return EMD_ERR_INVALID; }
            }
        }
    }
    t->num_planes = p;
    t->reserved = 0;
    for (int i = p; i <= PR_MAX_PLANES; i++) t->first[i] = (int32_t)total;
    for (int i = p; i < PR_MAX_PLANES; i++) { t->x[i] = nullptr; t->dx[i] = nullptr; t->H[i] = 3; t->R[i] = 1; t->w_smooth[i] = 0.f; t->w_l1[i] = 0.f; }
    return total;
}

}  // namespace

extern "C" size_t emd_plane_reg_workspace_size(const EmdPlaneRegArgs* a) {
    PlaneTab t;
    const int64_t n = pr_build(a, false, false, &t, "plane_reg_workspace_size");
    return n > 0 ? (size_t)n * 2 * sizeof(double) : 0;
}

extern "C" int emd_plane_reg_forward(const EmdPlaneRegArgs* a, void* workspace, size_t workspace_bytes, void* hip_stream) {
    PlaneTab t;
    const int64_t n = pr_build(a, true, false, &t, "plane_reg_forward");
    if (n < 0) return (int)n;
    if (!a->out) { emd_set_error("plane_reg_forward: null out"); return EMD_ERR_INVALID; }
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < (size_t)n * 2 * sizeof(double)) {
        emd_set_error("plane_reg_forward: workspace missing, misaligned or smaller than emd_plane_reg_workspace_size()");
        return EMD_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_plane_reg_forward, dim3((unsigned)n), dim3(EMD_BLOCK), 0, st, t, (double*)workspace);
    EMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_plane_reg_finalize, dim3(1), dim3(PR_FINAL_THREADS), 0, st, t, (const double*)workspace, a->plane_tv_weight,
                       a->time_smoothness_weight, a->l1_time_planes_weight, a->out);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_plane_reg_backward(const EmdPlaneRegArgs* a, void* hip_stream) {
    PlaneTab t;
    const int64_t n = pr_build(a, true, true, &t, "plane_reg_backward");
    if (n < 0) return (int)n;
    if (!a->g) { emd_set_error("plane_reg_backward: null g"); return EMD_ERR_INVALID; }
    hipLaunchKernelGGL(k_plane_reg_backward, dim3((unsigned)n), dim3(EMD_BLOCK), 0, (hipStream_t)hip_stream, t, a->g);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}
