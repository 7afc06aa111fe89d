// vanilla.hip -- the two per-iteration pieces of OmniRe's VanillaGaussians (models/gaussians/vanilla.py) beside the rasterizer: the per-class
// dictionary of get_gaussians (:378-414) and the regularisers of compute_reg_loss.  The contracts are in include/emd_raster.h (EmdVanillaArgs,
// EmdVanillaRegArgs); DESIGN.md section 8.16 has the launch shapes and the measurements.  gfx950, one Gaussian per lane.
//
// Built with the flags of standalone_ops.hip (-ffp-contract=off -fno-slp-vectorize): the activations and the SH colour share gaussian_math.h with
// k_activations and k_sh_forward and must produce the same bits as they do.
//
//   k_vanilla_forward      one launch: sigmoid / exp / normalise, the view direction, the SH colour + 0.5 clamped to [0, 1] (or sigmoid(dc)), and one
//                          byte per Gaussian that says which colour channels the clamp lets a gradient through
//   k_vanilla_backward     one launch: every gradient element written once, the rows of dL/dfeatures_rest the degree does not use as +0
//   k_vanilla_reg_forward  one workgroup per EMD_VANILLA_REG_CHUNK Gaussians: four fp64 partial sums and the visible count of the chunk
//   k_vanilla_reg_finalize one workgroup: the chunks added in a fixed order, four weighted floats out, 1/N and 1/max(|V|, 1) kept for the backward
//   k_vanilla_reg_backward one launch: dL/dlog_scales and dL/dopacity_logits written once each
// No atomics anywhere: every output is a fixed function of the inputs.
//
// features_rest is the one wide stream ([N][M-1][3], 180 B per Gaussian at M = 16).  A lane that read its own record would touch it at a record
// stride (k_sh_forward does); here the block's run, which is contiguous, is loaded by all lanes together -- dwordx4 when the degree uses every row,
// the used floats of each record as dwords when it does not -- and passes through LDS, half of the block's records at a time (23 KB: more resident
// waves), at an ODD row stride: a lane then reads its own row dword by dword without bank conflicts.  The backward sends dL/dfeatures_rest out the
// same way.  Every global load of a kernel is issued before the arithmetic starts.
#include "common.h"
#include "device_utils.h"
#include "fixed_sum.h"
#include "gaussian_math.h"

#pragma clang fp contract(off)

namespace {

#define VG_HALF (EMD_BLOCK / 2)
#define VG_MAX_REST3 45                        // floats of a features_rest record at M = 16
#define VG_REG_FINAL_THREADS 256
#define VG_MAX_POINTS (INT32_MAX - EMD_BLOCK)  // the kernels index Gaussians as int: block * EMD_BLOCK + lane of the last block must not wrap

// floats f .. f + 3 of p (f a multiple of 4, p 16-byte aligned), the ones at or past `total` as 0 without touching memory
__device__ __forceinline__ float4 vg_load4(const float* __restrict__ p, size_t f, size_t total) {
    if (f + 4 <= total) return *reinterpret_cast<const float4*>(p + f);
    float4 r;
    r.x = f < total ? p[f] : 0.f; r.y = f + 1 < total ? p[f + 1] : 0.f; r.z = f + 2 < total ? p[f + 2] : 0.f; r.w = 0.f;
    return r;
}

// DEG: the active degree in sh mode, -1 in dc mode.  FULL: the degree uses every row of a record (3 (K - 1) == MR3), so a half block's run is
// contiguous and is loaded as float4; otherwise the first 3 (K - 1) floats of every record are loaded as dwords.
template <int DEG, bool FULL>
__global__ void __launch_bounds__(EMD_BLOCK) k_vanilla_forward(int n, int MR3, EmdVanillaArgs a) {
    constexpr int K = DEG > 0 ? (DEG + 1) * (DEG + 1) : 1;
    constexpr int KR3 = 3 * (K - 1);                       // floats of a record the degree uses: 0, 9, 24, 45
    constexpr int S = KR3 | 1;                             // LDS row stride
    constexpr int T4 = FULL ? (KR3 + 7) / 8 : 1;           // float4 per lane and half: 128 KR3 floats / 4 / 256 lanes, rounded up
    constexpr int T1 = FULL ? 1 : (KR3 + 1) / 2;           // dwords per lane and half
    __shared__ float s_rest[DEG > 0 ? VG_HALF * S : 1];
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    const int ic = min(i, n - 1);                          // the lanes past the end load the last Gaussian again and store nothing

    // ---- every load ----
    float4 v4[2][T4];
    float v1[2][T1];
    if constexpr (DEG > 0) {
        const size_t total = (size_t)n * MR3;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const size_t rec0 = (size_t)blockIdx.x * EMD_BLOCK + VG_HALF * h;
            if constexpr (FULL) {
#pragma unroll
                for (int t = 0; t < T4; t++) {
                    const int q = threadIdx.x + EMD_BLOCK * t;
                    v4[h][t] = q < VG_HALF * KR3 / 4 ? vg_load4(a.features_rest, rec0 * KR3 + 4 * (size_t)q, total) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            } else {
#pragma unroll
                for (int t = 0; t < T1; t++) {
                    const int idx = threadIdx.x + EMD_BLOCK * t;
                    // unconditional: a slot past the half or past the end reads the last record; it is not staged, or no live lane reads it
                    const size_t g = min(rec0 + idx / KR3, (size_t)n - 1);
                    v1[h][t] = a.features_rest[g * MR3 + idx % KR3];
                }
            }
        }
    }
    const float l0 = a.log_scales[3 * (size_t)ic], l1 = a.log_scales[3 * (size_t)ic + 1], l2 = a.log_scales[3 * (size_t)ic + 2];
    const float4 qt = *reinterpret_cast<const float4*>(a.quats + 4 * (size_t)ic);
    const float lo = a.opacity_logits[ic];
    const float dc[3] = {a.features_dc[3 * (size_t)ic], a.features_dc[3 * (size_t)ic + 1], a.features_dc[3 * (size_t)ic + 2]};
    float d[3] = {0.f, 0.f, 1.f};
    if (DEG > 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) d[k] = a.means[3 * (size_t)ic + k] - a.camera_center[k];
    }

    // ---- the activations, in k_activations' operation order ----
    const bool live = i < n;
    if (live) {
        a.scales[3 * (size_t)i] = expf(l0); a.scales[3 * (size_t)i + 1] = expf(l1); a.scales[3 * (size_t)i + 2] = expf(l2);
        float v[4] = {qt.x, qt.y, qt.z, qt.w};
        const float nn = fmaxf(quat_norm(v), 1e-12f);
        *reinterpret_cast<float4*>(a.quats_out + 4 * (size_t)i) = make_float4(v[0] / nn, v[1] / nn, v[2] / nn, v[3] / nn);
        a.opacities[i] = sigmoidf_(lo);
    }

    // ---- the colour ----
    if (DEG < 0) {
        if (live) {
            a.rgbs[3 * (size_t)i] = sigmoidf_(dc[0]); a.rgbs[3 * (size_t)i + 1] = sigmoidf_(dc[1]); a.rgbs[3 * (size_t)i + 2] = sigmoidf_(dc[2]);
            if (a.clamp_mask) a.clamp_mask[i] = 7;
        }
        return;
    }
    float bs[16];
    if (DEG > 0) {                                                    // k_sh_forward's normalisation and sum order
        const float nn = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        d[0] /= nn; d[1] /= nn; d[2] /= nn;
    }
    sh_basis(DEG > 0 ? DEG : 0, d, bs);
    float c[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) c[ch] += bs[0] * dc[ch];
    if constexpr (DEG > 0) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (h) __syncthreads();                                    // (the first half's rows have been read)
            if constexpr (FULL) {
#pragma unroll
                for (int t = 0; t < T4; t++) {
                    const int q = threadIdx.x + EMD_BLOCK * t;
                    if (q < VG_HALF * KR3 / 4) {
                        const float e[4] = {v4[h][t].x, v4[h][t].y, v4[h][t].z, v4[h][t].w};
#pragma unroll
                        for (int x = 0; x < 4; x++) { const int f = 4 * q + x; s_rest[(f / KR3) * S + f % KR3] = e[x]; }
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < T1; t++) {
                    const int idx = threadIdx.x + EMD_BLOCK * t;
                    if (idx < VG_HALF * KR3) s_rest[(idx / KR3) * S + idx % KR3] = v1[h][t];
                }
            }
            __syncthreads();
            if ((int)(threadIdx.x >> 7) == h) {
                const float* row = s_rest + (threadIdx.x & (VG_HALF - 1)) * S;
#pragma unroll
                for (int k = 1; k < K; k++) { c[0] += bs[k] * row[3 * k - 3]; c[1] += bs[k] * row[3 * k - 2]; c[2] += bs[k] * row[3 * k - 1]; }
            }
        }
    }
    if (live) {
        uint32_t mask = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float v = c[ch] + 0.5f;
            mask |= (v >= 0.f && v <= 1.f) ? 1u << ch : 0u;            // torch's clamp passes the gradient on the closed interval
            a.rgbs[3 * (size_t)i + ch] = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);      // (a NaN stays a NaN, as in torch.clamp)
        }
        if (a.clamp_mask) a.clamp_mask[i] = (uint8_t)mask;
    }
}

// DEG as above.  MR3 = 3 (M - 1) floats per record of dL/dfeatures_rest, all of them written (the rows past the degree as +0).
template <int DEG>
__global__ void __launch_bounds__(EMD_BLOCK) k_vanilla_backward(int n, int MR3, EmdVanillaArgs a) {
    constexpr int K = DEG > 0 ? (DEG + 1) * (DEG + 1) : 1;
    __shared__ float s_g[VG_HALF * VG_MAX_REST3];
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    const int ic = min(i, n - 1);
    const bool live = i < n;

    // ---- every load ----
    const float l0 = a.log_scales[3 * (size_t)ic], l1 = a.log_scales[3 * (size_t)ic + 1], l2 = a.log_scales[3 * (size_t)ic + 2];
    const float4 qt = *reinterpret_cast<const float4*>(a.quats + 4 * (size_t)ic);
    const float lo = a.opacity_logits[ic];
    float dc[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 1.f};
    if (DEG < 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) dc[k] = a.features_dc[3 * (size_t)ic + k];
    }
    if (DEG > 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) d[k] = a.means[3 * (size_t)ic + k] - a.camera_center[k];
    }
    const uint32_t mask = (DEG >= 0 && a.g_rgbs) ? a.clamp_mask[ic] : 7u;
    const float go = a.g_opacities ? a.g_opacities[ic] : 0.f;
    float gs[3] = {0.f, 0.f, 0.f}, gc[3] = {0.f, 0.f, 0.f};
    float4 gq = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.g_scales) { gs[0] = a.g_scales[3 * (size_t)ic]; gs[1] = a.g_scales[3 * (size_t)ic + 1]; gs[2] = a.g_scales[3 * (size_t)ic + 2]; }
    if (a.g_quats) gq = *reinterpret_cast<const float4*>(a.g_quats + 4 * (size_t)ic);
    if (a.g_rgbs) { gc[0] = a.g_rgbs[3 * (size_t)ic]; gc[1] = a.g_rgbs[3 * (size_t)ic + 1]; gc[2] = a.g_rgbs[3 * (size_t)ic + 2]; }

    // ---- the activations ----
    if (live) {
        if (a.dL_dopacity_logits) { const float o = sigmoidf_(lo); a.dL_dopacity_logits[i] = go * (o * (1.f - o)); }
        if (a.dL_dlog_scales) {
            a.dL_dlog_scales[3 * (size_t)i] = gs[0] * expf(l0); a.dL_dlog_scales[3 * (size_t)i + 1] = gs[1] * expf(l1); a.dL_dlog_scales[3 * (size_t)i + 2] = gs[2] * expf(l2);
        }
        if (a.dL_dquats) {
            float v[4] = {qt.x, qt.y, qt.z, qt.w};
            const float nn = fmaxf(quat_norm(v), 1e-12f);
            const float u[4] = {v[0] / nn, v[1] / nn, v[2] / nn, v[3] / nn};
            const float dot = (u[0] * gq.x + u[1] * gq.y) + (u[2] * gq.z + u[3] * gq.w);
            *reinterpret_cast<float4*>(a.dL_dquats + 4 * (size_t)i) =
                make_float4((gq.x - u[0] * dot) / nn, (gq.y - u[1] * dot) / nn, (gq.z - u[2] * dot) / nn, (gq.w - u[3] * dot) / nn);
        }
    }

    // ---- the colour ----
    float bs[16];
    float gt[3];                                                      // the colour gradient behind the clamp (sh mode) or behind the sigmoid (dc mode)
    if (DEG < 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) { const float s = sigmoidf_(dc[ch]); gt[ch] = gc[ch] * (s * (1.f - s)); }
        bs[0] = 1.f;
    } else {
        if (DEG > 0) {
            const float nn = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            d[0] /= nn; d[1] /= nn; d[2] /= nn;
        }
        sh_basis(DEG > 0 ? DEG : 0, d, bs);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) gt[ch] = (mask >> ch & 1u) ? gc[ch] : 0.f;
    }
    if (live && a.dL_dfeatures_dc) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) a.dL_dfeatures_dc[3 * (size_t)i + ch] = bs[0] * gt[ch];
    }
    if (!a.dL_dfeatures_rest || MR3 <= 0) return;                     // (uniform: the barriers below are reached by every lane or by none)
    const int S = MR3 | 1;
    const size_t total = (size_t)n * MR3;
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
        if (h) __syncthreads();                                        // (the first half's rows have been stored)
        if ((int)(threadIdx.x >> 7) == h) {
            float* row = s_g + (threadIdx.x & (VG_HALF - 1)) * S;
#pragma unroll
            for (int k = 1; k < K; k++) { row[3 * k - 3] = bs[k] * gt[0]; row[3 * k - 2] = bs[k] * gt[1]; row[3 * k - 1] = bs[k] * gt[2]; }
            for (int j = 3 * (K - 1); j < MR3; j++) row[j] = 0.f;      // a row the degree does not use is +0, not 0 * g
        }
        __syncthreads();
        const size_t run = ((size_t)blockIdx.x * EMD_BLOCK + VG_HALF * h) * MR3;      // a multiple of 128 floats: float4 stores are aligned
        for (int q = threadIdx.x; q < VG_HALF * MR3 / 4; q += EMD_BLOCK) {
            const int f = 4 * q;
            int rec = f / MR3, j = f - rec * MR3;
            float e[4];
#pragma unroll
            for (int x = 0; x < 4; x++) {
                e[x] = s_g[rec * S + j];
                if (++j == MR3) { j = 0; rec++; }
            }
            const size_t o = run + f;
            if (o + 4 <= total) *reinterpret_cast<float4*>(a.dL_dfeatures_rest + o) = make_float4(e[0], e[1], e[2], e[3]);
            else {
#pragma unroll
                for (int x = 0; x < 4; x++)
                    if (o + x < total) a.dL_dfeatures_rest[o + x] = e[x];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The regularisers.  A lane owns EMD_VANILLA_REG_CHUNK / EMD_BLOCK Gaussians of its chunk, a block apart (contiguous across the wave).
// ---------------------------------------------------------------------------------------------------------------------------------------------
#define VR_PER_LANE (EMD_VANILLA_REG_CHUNK / EMD_BLOCK)
static_assert(EMD_VANILLA_REG_CHUNK % EMD_BLOCK == 0, "a chunk is whole blocks");

struct VrScales { float s[3], smax, smin; };
__device__ __forceinline__ VrScales vr_scales(float l0, float l1, float l2) {
    VrScales r;
    r.s[0] = expf(l0); r.s[1] = expf(l1); r.s[2] = expf(l2);
    r.smax = fmaxf(fmaxf(r.s[0], r.s[1]), r.s[2]);
    r.smin = fminf(fminf(r.s[0], r.s[1]), r.s[2]);
    return r;
}
// The smaller of o = sigmoid(a) and 1 - o, formed without the cancellation of 1 - o: w = 1 / (1 + exp(|a|)).  The entropy is even in a, and
// o (1 - o) = w (1 - w).  The clip of o to [1e-6, 1 - 1e-6] is the clip of w to [1e-6, 1/2] from below; inside it means w >= 1e-6.
__device__ __forceinline__ float vr_small_side(float a) { return 1.f / (1.f + expf(fabsf(a))); }
#define VR_CLIP 1e-6f

// partials [chunks][4] doubles: the sums over the chunk of max(ratio, R) - R, min(smin, 30), the entropy over V, smax^2; counts [chunks]: |V| of the chunk
__global__ void __launch_bounds__(EMD_BLOCK) k_vanilla_reg_forward(int n, const float* __restrict__ ls, const float* __restrict__ logits,
                                                                   const int32_t* __restrict__ radii, float R, int scale_terms, int sparse,
                                                                   double* __restrict__ partials, int32_t* __restrict__ counts) {
    __shared__ double sm[EMD_BLOCK / EMD_WAVE][4];
    __shared__ int32_t sc[EMD_BLOCK / EMD_WAVE];
    float l[VR_PER_LANE][3], av[VR_PER_LANE];
    int32_t rv[VR_PER_LANE];
#pragma unroll
    for (int j = 0; j < VR_PER_LANE; j++) {
        const size_t i = (size_t)blockIdx.x * EMD_VANILLA_REG_CHUNK + j * EMD_BLOCK + threadIdx.x;
        const size_t c = i < (size_t)n ? i : (size_t)n - 1;
        l[j][0] = l[j][1] = l[j][2] = 0.f; av[j] = 0.f; rv[j] = 0;
        if (scale_terms) { l[j][0] = ls[3 * c]; l[j][1] = ls[3 * c + 1]; l[j][2] = ls[3 * c + 2]; }
        if (sparse) { av[j] = logits[c]; rv[j] = radii[c]; }
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int32_t vis = 0;
#pragma unroll
    for (int j = 0; j < VR_PER_LANE; j++) {
        const size_t i = (size_t)blockIdx.x * EMD_VANILLA_REG_CHUNK + j * EMD_BLOCK + threadIdx.x;
        if (i >= (size_t)n) continue;
        if (scale_terms) {
            const VrScales v = vr_scales(l[j][0], l[j][1], l[j][2]);
            acc[0] += (double)(fmaxf(v.smax / v.smin, R) - R);
            acc[1] += (double)fminf(v.smin, 30.f);                     // |clamp(smin, 0, 30)| of a positive smin
            acc[3] += (double)(v.smax * v.smax);
        }
        if (sparse && rv[j] > 0) {
            const float w = fmaxf(vr_small_side(av[j]), VR_CLIP);
            acc[2] += (double)(-((1.f - w) * log1pf(-w) + w * logf(w)));
            vis++;
        }
    }
    // (the four waves meet as in fixed_block_store, fixed_sum.h, with the integer count beside the doubles behind the same barrier: through the
    //  template the kernel came out with other instructions, profiles/shared_source_isa.txt)
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] = fixed_wave_sum(acc[k]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) vis += __shfl_xor(vis, m);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) sm[threadIdx.x >> 6][k] = acc[k];
        sc[threadIdx.x >> 6] = vis;
    }
    __syncthreads();
    if (threadIdx.x < 4) partials[4 * (size_t)blockIdx.x + threadIdx.x] = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
    if (threadIdx.x == 4) counts[blockIdx.x] = (sc[0] + sc[1]) + (sc[2] + sc[3]);
}

// One workgroup.  Lane t adds the chunks t, t + 256, ... in ascending order, then the fixed tree.  head[0] = 1 / N, head[1] = 1 / max(|V|, 1).
__global__ void __launch_bounds__(VG_REG_FINAL_THREADS) k_vanilla_reg_finalize(int n, int chunks, const double* __restrict__ partials,
                                                                               const int32_t* __restrict__ counts, float w_sharp, float w_flatten,
                                                                               float w_sparse, float w_msq, double* __restrict__ head,
                                                                               float* __restrict__ terms) {
    __shared__ double sm[VG_REG_FINAL_THREADS / EMD_WAVE][4];
    __shared__ long long sc[VG_REG_FINAL_THREADS / EMD_WAVE];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    long long vis = 0;
    for (int c = threadIdx.x; c < chunks; c += VG_REG_FINAL_THREADS) {
#pragma unroll
        for (int k = 0; k < 4; k++) acc[k] += partials[4 * (size_t)c + k];
        vis += counts[c];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] = fixed_wave_sum(acc[k]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) vis += __shfl_xor(vis, m);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) sm[threadIdx.x >> 6][k] = acc[k];
        sc[threadIdx.x >> 6] = vis;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4];
#pragma unroll
        for (int k = 0; k < 4; k++) t[k] = (sm[0][k] + sm[1][k]) + (sm[2][k] + sm[3][k]);
        const long long v = (sc[0] + sc[1]) + (sc[2] + sc[3]);
        const double inv_n = 1.0 / (double)n, inv_v = 1.0 / (double)(v > 0 ? v : 1);
        head[0] = inv_n; head[1] = inv_v;
        terms[0] = (float)((double)w_sharp * t[0] * inv_n);
        terms[1] = (float)((double)w_flatten * t[1] * inv_n);
        terms[2] = (float)((double)w_sparse * t[2] * inv_v);
        terms[3] = (float)((double)w_msq * t[3] * inv_n);
    }
}

__global__ void __launch_bounds__(EMD_BLOCK) k_vanilla_reg_backward(int n, const float* __restrict__ ls, const float* __restrict__ logits,
                                                                    const int32_t* __restrict__ radii, float R, float w_sharp, float w_flatten,
                                                                    float w_sparse, float w_msq, int sparse, const double* __restrict__ head,
                                                                    const float* __restrict__ g, float* __restrict__ d_ls, float* __restrict__ d_logits) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float l0 = ls[3 * (size_t)i], l1 = ls[3 * (size_t)i + 1], l2 = ls[3 * (size_t)i + 2];
    const float av = sparse ? logits[i] : 0.f;
    const int32_t rv = sparse ? radii[i] : 0;
    const double inv_n = head[0], inv_v = head[1];
    // (a skipped term has weight 0 here: its upstream scalar is not read into the product as NaN * 0)
    const float k_sharp = w_sharp != 0.f ? (float)((double)g[0] * (double)w_sharp * inv_n) : 0.f;
    const float k_flat = w_flatten != 0.f ? (float)((double)g[1] * (double)w_flatten * inv_n) : 0.f;
    const float k_sparse = sparse ? (float)((double)g[2] * (double)w_sparse * inv_v) : 0.f;
    const float k_msq = w_msq != 0.f ? (float)((double)g[3] * (double)w_msq * inv_n) : 0.f;

    const VrScales v = vr_scales(l0, l1, l2);
    int nmax = 0, nmin = 0, first_max = -1, first_min = -1;
#pragma unroll
    for (int k = 2; k >= 0; k--) {
        if (v.s[k] == v.smax) { nmax++; first_max = k; }
        if (v.s[k] == v.smin) { nmin++; first_min = k; }
    }
    const float ratio = v.smax / v.smin;
    const float up = (w_sharp != 0.f && ratio > R) ? k_sharp * ratio : 0.f;          // amax / amin share the gradient evenly among equal columns
    const float flat = (w_flatten != 0.f && v.smin < 30.f) ? k_flat * v.smin : 0.f;  // min / max (with indices) give it to the lowest of equal columns
    const float msq = w_msq != 0.f ? k_msq * (2.f * (v.smax * v.smax)) : 0.f;
    float out[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float o = 0.f;
        if (v.s[k] == v.smax) o += up / (float)nmax;
        if (v.s[k] == v.smin) o -= up / (float)nmin;
        if (k == first_min) o += flat;
        if (k == first_max) o += msq;
        out[k] = o;
    }
    d_ls[3 * (size_t)i] = out[0]; d_ls[3 * (size_t)i + 1] = out[1]; d_ls[3 * (size_t)i + 2] = out[2];
    if (d_logits) {
        float o = 0.f;
        if (sparse && rv > 0) {
            const float w = vr_small_side(av);
            if (w >= VR_CLIP) o = k_sparse * (-av * (w * (1.f - w)));  // ln((1 - o~) / o~) = -a inside the clip
        }
        d_logits[i] = o;
    }
}

bool vg_misaligned(const void* p, uintptr_t m) { return ((uintptr_t)p & m) != 0; }

// 0 when the arguments can be launched, else EMD_ERR_INVALID with the message set.  `backward`: the upstream gradients and the outputs of the backward.
int vg_check(const EmdVanillaArgs* a, bool backward, const char* who) {
    if (!a) { emd_set_error("%s: null args", who); return EMD_ERR_INVALID; }
    if (a->num_points < 0) { emd_set_error("%s: negative num_points (%d)", who, a->num_points); return EMD_ERR_INVALID; }
    if (a->num_points > VG_MAX_POINTS) { emd_set_error("%s: num_points %d above %d", who, a->num_points, VG_MAX_POINTS); return EMD_ERR_INVALID; }
    if (a->sh_coeffs < 1 || a->sh_coeffs > 16) { emd_set_error("%s: sh_coeffs %d outside 1 .. 16", who, a->sh_coeffs); return EMD_ERR_INVALID; }
    if (a->degree < 0 || a->degree > 3) { emd_set_error("%s: degree %d out of range (0 .. 3)", who, a->degree); return EMD_ERR_INVALID; }
    if (a->sh_mode != 0 && a->sh_mode != 1) { emd_set_error("%s: sh_mode %d is neither 0 (dc) nor 1 (sh)", who, a->sh_mode); return EMD_ERR_INVALID; }
    if ((a->degree + 1) * (a->degree + 1) > a->sh_coeffs) {
        emd_set_error("%s: degree %d needs %d coefficient rows, sh_coeffs is %d", who, a->degree, (a->degree + 1) * (a->degree + 1), a->sh_coeffs);
        return EMD_ERR_INVALID;
    }
    const bool dirs = a->sh_mode && a->degree > 0;
    if (!a->means || !a->log_scales || !a->quats || !a->opacity_logits || !a->features_dc || (a->sh_mode && !a->camera_center) ||
        (dirs && !a->features_rest)) {
        emd_set_error("%s: null input (means, log_scales, quats, opacity_logits, features_dc; camera_center in sh mode; features_rest at degree > 0)", who);
        return EMD_ERR_INVALID;
    }
    if (!backward && (!a->opacities || !a->scales || !a->quats_out || !a->rgbs)) { emd_set_error("%s: null output", who); return EMD_ERR_INVALID; }
    if (backward && a->sh_mode && a->g_rgbs && !a->clamp_mask) {
        emd_set_error("%s: null clamp_mask (the forward's, needed for the gradient of the clamped colour)", who);
        return EMD_ERR_INVALID;
    }
    const void* wide[] = {a->means, a->log_scales, a->quats, a->opacity_logits, a->features_dc, a->features_rest, a->opacities, a->scales, a->quats_out,
                          a->rgbs, a->g_quats, a->dL_dopacity_logits, a->dL_dlog_scales, a->dL_dquats, a->dL_dfeatures_dc, a->dL_dfeatures_rest};
    for (const void* p : wide)
        if (vg_misaligned(p, 15)) { emd_set_error("%s: a tensor is not 16-byte aligned", who); return EMD_ERR_INVALID; }
    // g_opacities, g_scales and g_rgbs are read dword by dword: autograd hands a consumer's torch.cat or slice back as a view at any row offset
    const void* narrow[] = {a->camera_center, a->g_opacities, a->g_scales, a->g_rgbs};
    for (const void* p : narrow)
        if (vg_misaligned(p, 3)) { emd_set_error("%s: camera_center or an upstream gradient is not 4-byte aligned", who); return EMD_ERR_INVALID; }
    return EMD_OK;
}

struct VrPlan { int64_t chunks; size_t partials_off, counts_off, bytes; bool scale_terms, sparse; };

int vr_plan(const EmdVanillaRegArgs* a, bool pointers, VrPlan* p, const char* who) {
    if (!a) { emd_set_error("%s: null args", who); return EMD_ERR_INVALID; }
    if (a->num_points < 1) { emd_set_error("%s: num_points %d < 1 (a mean over no Gaussian)", who, a->num_points); return EMD_ERR_INVALID; }
    if (a->num_points > VG_MAX_POINTS) { emd_set_error("%s: num_points %d above %d", who, a->num_points, VG_MAX_POINTS); return EMD_ERR_INVALID; }
    p->chunks = ((int64_t)a->num_points + EMD_VANILLA_REG_CHUNK - 1) / EMD_VANILLA_REG_CHUNK;
    p->partials_off = 2 * sizeof(double);
    p->counts_off = p->partials_off + (size_t)p->chunks * 4 * sizeof(double);
    p->bytes = emd_align_up(p->counts_off + (size_t)p->chunks * sizeof(int32_t), 8);
    p->scale_terms = a->w_sharp != 0.f || a->w_flatten != 0.f || a->w_max_s_square != 0.f;
    p->sparse = a->w_sparse != 0.f && a->opacity_logits && a->radii;
    if (pointers) {
        if (!a->log_scales) { emd_set_error("%s: null log_scales", who); return EMD_ERR_INVALID; }
        if (vg_misaligned(a->log_scales, 3) || vg_misaligned(a->opacity_logits, 3) || vg_misaligned(a->radii, 3)) {
            emd_set_error("%s: a tensor is not 4-byte aligned", who);
            return EMD_ERR_INVALID;
        }
        if (!(a->max_gauss_ratio > 0.f)) { emd_set_error("%s: max_gauss_ratio must be positive", who); return EMD_ERR_INVALID; }
    }
    return EMD_OK;
}

}  // namespace

extern "C" int emd_vanilla_forward(const EmdVanillaArgs* a, void* hip_stream) {
    const int rc = vg_check(a, false, "vanilla_forward");
    if (rc) return rc;
    const int n = a->num_points, MR3 = 3 * (a->sh_coeffs - 1);
    if (n == 0) return EMD_OK;
    const dim3 grid((n + EMD_BLOCK - 1) / EMD_BLOCK), block(EMD_BLOCK);
    hipStream_t st = (hipStream_t)hip_stream;
    const int deg = a->sh_mode ? a->degree : -1;
    const bool full = deg > 0 && 3 * ((deg + 1) * (deg + 1) - 1) == MR3;
    switch (deg) {
    case -1: hipLaunchKernelGGL((k_vanilla_forward<-1, true>), grid, block, 0, st, n, MR3, *a); break;
    case 0: hipLaunchKernelGGL((k_vanilla_forward<0, true>), grid, block, 0, st, n, MR3, *a); break;
    case 1:
        if (full) hipLaunchKernelGGL((k_vanilla_forward<1, true>), grid, block, 0, st, n, MR3, *a);
        else hipLaunchKernelGGL((k_vanilla_forward<1, false>), grid, block, 0, st, n, MR3, *a);
        break;
    case 2:
        if (full) hipLaunchKernelGGL((k_vanilla_forward<2, true>), grid, block, 0, st, n, MR3, *a);
        else hipLaunchKernelGGL((k_vanilla_forward<2, false>), grid, block, 0, st, n, MR3, *a);
        break;
    default: hipLaunchKernelGGL((k_vanilla_forward<3, true>), grid, block, 0, st, n, MR3, *a); break;      // (degree 3 needs all 16 rows)
    }
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_vanilla_backward(const EmdVanillaArgs* a, void* hip_stream) {
    const int rc = vg_check(a, true, "vanilla_backward");
    if (rc) return rc;
    const int n = a->num_points, MR3 = 3 * (a->sh_coeffs - 1);
    if (n == 0) return EMD_OK;
    const dim3 grid((n + EMD_BLOCK - 1) / EMD_BLOCK), block(EMD_BLOCK);
    hipStream_t st = (hipStream_t)hip_stream;
    switch (a->sh_mode ? a->degree : -1) {
    case -1: hipLaunchKernelGGL((k_vanilla_backward<-1>), grid, block, 0, st, n, MR3, *a); break;
    case 0: hipLaunchKernelGGL((k_vanilla_backward<0>), grid, block, 0, st, n, MR3, *a); break;
    case 1: hipLaunchKernelGGL((k_vanilla_backward<1>), grid, block, 0, st, n, MR3, *a); break;
    case 2: hipLaunchKernelGGL((k_vanilla_backward<2>), grid, block, 0, st, n, MR3, *a); break;
    default: hipLaunchKernelGGL((k_vanilla_backward<3>), grid, block, 0, st, n, MR3, *a); break;
    }
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" size_t emd_vanilla_reg_workspace_size(int32_t num_points) {
    EmdVanillaRegArgs a = {};
    a.num_points = num_points;
    VrPlan p;
    return vr_plan(&a, false, &p, "vanilla_reg_workspace_size") ? 0 : p.bytes;
}

extern "C" int emd_vanilla_reg_forward(const EmdVanillaRegArgs* a, void* workspace, size_t workspace_bytes, void* hip_stream) {
    VrPlan p;
    const int rc = vr_plan(a, true, &p, "vanilla_reg_forward");
    if (rc) return rc;
    if (!a->terms) { emd_set_error("vanilla_reg_forward: null terms"); return EMD_ERR_INVALID; }
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < p.bytes) {
        emd_set_error("vanilla_reg_forward: workspace missing, misaligned or smaller than emd_vanilla_reg_workspace_size()");
        return EMD_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    double* partials = (double*)((char*)workspace + p.partials_off);
    int32_t* counts = (int32_t*)((char*)workspace + p.counts_off);
    hipLaunchKernelGGL(k_vanilla_reg_forward, dim3((unsigned)p.chunks), dim3(EMD_BLOCK), 0, st, a->num_points, a->log_scales, a->opacity_logits, a->radii,
                       a->max_gauss_ratio, p.scale_terms ? 1 : 0, p.sparse ? 1 : 0, partials, counts);
    EMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vanilla_reg_finalize, dim3(1), dim3(VG_REG_FINAL_THREADS), 0, st, a->num_points, (int)p.chunks, (const double*)partials,
                       (const int32_t*)counts, a->w_sharp, a->w_flatten, p.sparse ? a->w_sparse : 0.f, a->w_max_s_square, (double*)workspace, a->terms);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_vanilla_reg_backward(const EmdVanillaRegArgs* a, const void* workspace, size_t workspace_bytes, void* hip_stream) {
    VrPlan p;
    const int rc = vr_plan(a, true, &p, "vanilla_reg_backward");
    if (rc) return rc;
    if (!a->g || !a->dL_dlog_scales) { emd_set_error("vanilla_reg_backward: null g or dL_dlog_scales"); return EMD_ERR_INVALID; }
    if (vg_misaligned(a->dL_dlog_scales, 3) || vg_misaligned(a->dL_dopacity_logits, 3) || vg_misaligned(a->g, 3)) {
        emd_set_error("vanilla_reg_backward: a tensor is not 4-byte aligned");
        return EMD_ERR_INVALID;
    }
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < p.bytes) {
        emd_set_error("vanilla_reg_backward: workspace missing, misaligned or smaller than emd_vanilla_reg_workspace_size() (it is the forward's)");
        return EMD_ERR_WORKSPACE;
    }
    const int n = a->num_points;
    hipLaunchKernelGGL(k_vanilla_reg_backward, dim3((n + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, (hipStream_t)hip_stream, n, a->log_scales,
                       a->opacity_logits, a->radii, a->max_gauss_ratio, a->w_sharp, a->w_flatten, a->w_sparse, a->w_max_s_square, p.sparse ? 1 : 0,
                       (const double*)workspace, a->g, a->dL_dlog_scales, a->dL_dopacity_logits);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}
