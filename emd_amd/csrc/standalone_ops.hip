// standalone_ops.hip -- the entry points beside the rasterizer's own pipeline, one small kernel each: explicit motion and SH colour as
// stand-alone forward / backward, the dense SH gradient from per-view factors, the activations, the per-frame actor pose table, the
// densification statistics, and the L1 losses with their backward passes.  gfx950, one element per lane.
//
// Built with the flags of preprocess.hip (-ffp-contract=off -fno-slp-vectorize): the motion and SH kernels share gaussian_math.h with K1 / K8
// and must produce the same bits as they do.  The actor pose row is shared with embed.hip's one-launch actor chain the same way, through
// quat_math.h (no contraction there whatever the unit's flags).
//
// Reference behaviour this replaces (file:line):
//   activations                           S3Gaussian/gaussian_renderer/__init__.py:99-101
//   SH colour                             S3Gaussian/utils/sh_utils.py:57-112, gaussian_renderer/__init__.py:19-25
//   rigid actor motion + residual         OmniRe/models/nodes/rigid.py:478-568, deformable.py:57-69
//   densification statistics              S3Gaussian/scene/gaussian_model.py:728-730, train.py:403-406
//   L1 loss                               S3Gaussian/utils/loss_utils.py:21-22, train.py:226
#include "common.h"
#include "device_utils.h"
#include "gaussian_math.h"

#pragma clang fp contract(off)

namespace {

__global__ void __launch_bounds__(EMD_BLOCK) k_motion_forward(int n, const float* means, const float* quats,
                                                              const float* opac, EmdMotion mo, float* wm, float* wq,
                                                              float* wo) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i >= n) return;
    float m[3], q[4] = {1.f, 0.f, 0.f, 0.f}, o = 0.f;
    motion_point(i, means, quats, opac, mo, m, q, &o);
    if (wm) { wm[3 * i] = m[0]; wm[3 * i + 1] = m[1]; wm[3 * i + 2] = m[2]; }
    if (wq && quats) *(float4*)(wq + 4 * i) = make_float4(q[0], q[1], q[2], q[3]);
    if (wo && opac) wo[i] = o;
}

__global__ void __launch_bounds__(EMD_BLOCK) k_sh_forward(int n, int deg, int M, const float* dirs,
                                                          const float* coeffs, float* rgb) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i >= n) return;
    float d[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
    float nn = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    d[0] /= nn; d[1] /= nn; d[2] /= nn;
    float bs[16];
    sh_basis(deg, d, bs);
    const int K = (deg + 1) * (deg + 1);
    const float* sh = coeffs + (size_t)i * M * 3;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    for (int k = 0; k < K; k++) { c0 += bs[k] * sh[3 * k]; c1 += bs[k] * sh[3 * k + 1]; c2 += bs[k] * sh[3 * k + 2]; }
    rgb[3 * i] = c0; rgb[3 * i + 1] = c1; rgb[3 * i + 2] = c2;
}

__global__ void __launch_bounds__(EMD_BLOCK) k_motion_backward(int n, const float* means, const float* quats,
                                                               const float* opac, EmdMotion mo, const float* g_wm,
                                                               const float* g_wq, const float* g_wo, float* d_means,
                                                               float* d_quats, float* d_opac, float* d_pose,
                                                               float* d_rdx, float* d_rdq) {
#include "motion_point_bwd_body.inc"
    if (d_pose) reduce_pose_grad(a_id, pose_g, d_pose);
}

// The deterministic form (emd_motion_backward_det), k_motion_backward up to its last statement: the per-point half of both is
// one text, motion_point_bwd_body.inc (k_motion_backward kept its instructions: profiles/shared_source_isa.txt).  A bound point stores its twelve floats as row i of pose_rows, as K8 does
// under EMD_FLAG_DETERMINISTIC (preprocess.hip), and its actor as the row's destination; the sort drops the static points (0xFFFFFFFF) and the
// segmented row sum adds every actor's rows in ascending point index (api.hip).  No atomics.  pose_rows == NULL: no pose gradient is asked for.
__global__ void __launch_bounds__(EMD_BLOCK) k_motion_backward_det(int n, const float* means, const float* quats,
                                                                   const float* opac, EmdMotion mo, const float* g_wm,
                                                                   const float* g_wq, const float* g_wo, float* d_means,
                                                                   float* d_quats, float* d_opac, float* d_rdx, float* d_rdq,
                                                                   float* __restrict__ pose_rows, uint32_t* __restrict__ keys_in) {
#include "motion_point_bwd_body.inc"
    if (!pose_rows || i >= n) return;
    if (a_id >= 0) {
        float4* pr = reinterpret_cast<float4*>(pose_rows + (size_t)i * EMD_ACTOR_STRIDE);
        pr[0] = make_float4(pose_g[0], pose_g[1], pose_g[2], pose_g[3]);
        pr[1] = make_float4(pose_g[4], pose_g[5], pose_g[6], pose_g[7]);
        pr[2] = make_float4(pose_g[8], pose_g[9], pose_g[10], pose_g[11]);
    }
    keys_in[i] = a_id >= 0 ? (uint32_t)a_id : 0xFFFFFFFFu;
}

__global__ void __launch_bounds__(EMD_BLOCK) k_sh_backward(int n, int deg, int M, const float* dirs,
                                                           const float* coeffs, const float* g_rgb, float* d_coeffs,
                                                           float* d_dirs) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i >= n) return;
    float d0[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
    float nn = sqrtf((d0[0] * d0[0] + d0[1] * d0[1]) + d0[2] * d0[2]);
    float d[3] = {d0[0] / nn, d0[1] / nn, d0[2] / nn};
    const float gc[3] = {g_rgb[3 * i], g_rgb[3 * i + 1], g_rgb[3 * i + 2]};
    const int K = (deg + 1) * (deg + 1);
    if (d_coeffs) {
        float bs[16];
        sh_basis(deg, d, bs);
        float* o = d_coeffs + (size_t)i * M * 3;
        for (int k = 0; k < M; k++) {
            // a row the degree does not use is +0, not 0 * g (that is -0 for g < 0 and NaN for a non-finite g)
            if (k < K) { o[3 * k] = bs[k] * gc[0]; o[3 * k + 1] = bs[k] * gc[1]; o[3 * k + 2] = bs[k] * gc[2]; }
            else { o[3 * k] = 0.f; o[3 * k + 1] = 0.f; o[3 * k + 2] = 0.f; }
        }
    }
    if (d_dirs) {
        float gd[3];
        sh_dir_backward(deg, d, coeffs + (size_t)i * M * 3, gc, gd);
        float dot = (d[0] * gd[0] + d[1] * gd[1]) + d[2] * gd[2];
        d_dirs[3 * i] = (gd[0] - d[0] * dot) / nn;
        d_dirs[3 * i + 1] = (gd[1] - d[1] * dot) / nn;
        d_dirs[3 * i + 2] = (gd[2] - d[2] * dot) / nn;
    }
}

// Dense, view-averaged SH gradient from the per-view rank-one factors (emd_sh_grad_from_factors): one Gaussian per lane,
// rows leave through LDS as coalesced dwordx4 stores like K8's (preprocess.hip).
__global__ void __launch_bounds__(EMD_BLOCK) k_sh_grad_from_factors(int n, int V, int deg, const float* __restrict__ means,
                                                                    EmdMotion mo, int pose_per_view, const float* __restrict__ campos,
                                                                    const float* __restrict__ gc, float scale,
                                                                    float* __restrict__ d_shs) {
    __shared__ float4 s_sh[(EMD_BLOCK / 2) * SH_ROW4];    // half of the block's rows at a time (26 KB: more resident waves)
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    float acc[48];
#pragma unroll
    for (int k = 0; k < 48; k++) acc[k] = 0.f;
    if (i < n) {
        float m[3], qd[4], od;
        if (mo.actor_id || mo.residual_dx) motion_point(i, means, nullptr, nullptr, mo, m, qd, &od, false);
        else { m[0] = means[3 * i]; m[1] = means[3 * i + 1]; m[2] = means[3 * i + 2]; }
        const int K = (deg + 1) * (deg + 1);
        // views of different timestamps (6 cameras on 8 ranks): an actor's Gaussians sit at a different world position in every
        // view, so the pose table is per view ([V][A][12]); static Gaussians keep the position computed above
        const bool moving = pose_per_view && mo.actor_id && mo.actor_id[i] >= 0;
        for (int v = 0; v < V; v++) {
            const float* g = gc + ((size_t)v * n + i) * 3;
            const float g0 = g[0], g1 = g[1], g2 = g[2];
            if (g0 == 0.f && g1 == 0.f && g2 == 0.f) continue;          // not visible in view v
            if (moving && v > 0) {
                EmdMotion mv = mo;
                mv.actor_pose = mo.actor_pose + (size_t)v * mo.num_actors * EMD_ACTOR_STRIDE;
                motion_point(i, means, nullptr, nullptr, mv, m, qd, &od, false);
            }
            float d[3] = {m[0] - campos[3 * v], m[1] - campos[3 * v + 1], m[2] - campos[3 * v + 2]};
            const float nn = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            d[0] /= nn; d[1] /= nn; d[2] /= nn;
            float bs[16];
            sh_basis(deg, d, bs);
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if (k < K) { acc[3 * k] += bs[k] * g0; acc[3 * k + 1] += bs[k] * g1; acc[3 * k + 2] += bs[k] * g2; }
            }
        }
    }
    const size_t lim4 = (size_t)n * 12;
    float4* out = (float4*)d_shs;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if ((int)(threadIdx.x >> 7) == h) {
#pragma unroll
            for (int j = 0; j < 12; j++)
                s_sh[(threadIdx.x & 127) * SH_ROW4 + j] = make_float4(acc[4 * j] * scale, acc[4 * j + 1] * scale, acc[4 * j + 2] * scale, acc[4 * j + 3] * scale);
        }
        __syncthreads();
        const size_t base4 = ((size_t)blockIdx.x * EMD_BLOCK + 128 * h) * 12;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const uint32_t idx = threadIdx.x + EMD_BLOCK * j;
            if (base4 + idx < lim4) out[base4 + idx] = s_sh[(idx / 12) * SH_ROW4 + (idx % 12)];
        }
        __syncthreads();
    }
}

// Densification statistics of one view, in place and without the boolean-mask indexing (= a device-to-host sync) of the
// reference: for every visible Gaussian  accum += |dL/dmean2D.xy|, denom += 1, max_radii = max(max_radii, radius)
// (S3Gaussian/scene/gaussian_model.py:728-730, train.py:403-406).
__global__ void __launch_bounds__(EMD_BLOCK) k_densification_stats(int n, const int32_t* __restrict__ radii,
                                                                   const float* __restrict__ g2d /*[N,3]*/,
                                                                   float* __restrict__ accum, float* __restrict__ denom,
                                                                   float* __restrict__ max_radii) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int r = radii[i];
    if (r <= 0) return;
    const float gx = g2d[3 * i], gy = g2d[3 * i + 1];
    if (accum) accum[i] += sqrtf(gx * gx + gy * gy);
    if (denom) denom[i] += 1.f;
    if (max_radii) max_radii[i] = fmaxf(max_radii[i], (float)r);
}

__global__ void __launch_bounds__(EMD_BLOCK) k_activations(int n, const float* ls, float* sc, const float* rq, float* q,
                                                           const float* lo, float* o) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (ls && sc) { sc[3 * i] = expf(ls[3 * i]); sc[3 * i + 1] = expf(ls[3 * i + 1]); sc[3 * i + 2] = expf(ls[3 * i + 2]); }
    if (rq && q) {
        const float4 t = *(const float4*)(rq + 4 * i);
        float v[4] = {t.x, t.y, t.z, t.w};
        const float nn = fmaxf(quat_norm(v), 1e-12f);
        *(float4*)(q + 4 * i) = make_float4(v[0] / nn, v[1] / nn, v[2] / nn, v[3] / nn);
    }
    if (lo && o) o[i] = sigmoidf_(lo[i]);
}

// ---------------------------------------------------------------------------------------------------
// Per-frame actor pose table (training branch of rigid.py:478-568): one lane per actor.
//   q_mean = normalize(q_f)                       rotation applied to local means          (rigid.py:499-503)
//   trans  = t_f + dt      (dt skipped when NaN)                                            (rigid.py:519-532)
//   q_rot  = normalize(q_f (x) dq)  (dq skipped when NaN) composed onto local quaternions   (rigid.py:547-566)
// Replaces ~25 launch-bound torch kernels (normalize / cat / index and their backward) per step.  The row's arithmetic is
// pose_row_forward / pose_row_backward (quat_math.h), which k_tracked_pose (embed.hip) calls too: the kernels here load and store.
// ---------------------------------------------------------------------------------------------------
__global__ void k_actor_pose_forward(int A, const float* __restrict__ q_f, const float* __restrict__ t_f,
                                     const uint8_t* __restrict__ valid, const float* __restrict__ dt,
                                     const float* __restrict__ dq, float* __restrict__ pose, const int32_t* __restrict__ frame_dev) {
    if (frame_dev) {        // q_f / t_f / valid are the whole [F, A, .] tables and the frame index lives on the device (hipGraph replay)
        const size_t f = (size_t)frame_dev[0];
        q_f += f * A * 4; t_f += f * A * 3;
        if (valid) valid += f * A;
    }
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= A) return;
    const float q[4] = {q_f[4 * a], q_f[4 * a + 1], q_f[4 * a + 2], q_f[4 * a + 3]}, t[3] = {t_f[3 * a], t_f[3 * a + 1], t_f[3 * a + 2]};
    float dtv[3] = {0.f, 0.f, 0.f}, dqv[4] = {1.f, 0.f, 0.f, 0.f}, row[12];
    if (dt) for (int k = 0; k < 3; k++) dtv[k] = dt[3 * a + k];
    if (dq) for (int k = 0; k < 4; k++) dqv[k] = dq[4 * a + k];
    pose_row_forward(q, t, dt != nullptr, dtv, dq != nullptr, dqv, valid ? (valid[a] ? 1.f : 0.f) : 1.f, row);
    float* P = pose + (size_t)a * EMD_ACTOR_STRIDE;
    for (int k = 0; k < 12; k++) P[k] = row[k];
}

__global__ void k_actor_pose_backward(int A, const float* __restrict__ q_f, const float* __restrict__ dt,
                                      const float* __restrict__ dq, const float* __restrict__ g_pose,
                                      float* __restrict__ d_q_f, float* __restrict__ d_t_f, float* __restrict__ d_dt,
                                      float* __restrict__ d_dq, const int32_t* __restrict__ frame_dev) {
    if (frame_dev) { const size_t f = (size_t)frame_dev[0]; q_f += f * A * 4; d_q_f += f * A * 4; d_t_f += f * A * 3; }
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= A) return;
    const float q[4] = {q_f[4 * a], q_f[4 * a + 1], q_f[4 * a + 2], q_f[4 * a + 3]};
    float dtv[3] = {0.f, 0.f, 0.f}, dqv[4] = {1.f, 0.f, 0.f, 0.f}, G[12], dqf[4], ddt[3], dr[4];
    if (dt) for (int k = 0; k < 3; k++) dtv[k] = dt[3 * a + k];
    if (dq) for (int k = 0; k < 4; k++) dqv[k] = dq[4 * a + k];
    for (int k = 0; k < 12; k++) G[k] = g_pose[(size_t)a * EMD_ACTOR_STRIDE + k];
    pose_row_backward(q, dt != nullptr, dtv, dq != nullptr, dqv, G, dqf, ddt, dr);
    for (int k = 0; k < 4; k++) d_q_f[4 * a + k] = dqf[k];
    for (int k = 0; k < 3; k++) d_t_f[3 * a + k] = G[4 + k];
    if (d_dt) for (int k = 0; k < 3; k++) d_dt[3 * a + k] = ddt[k];
    if (d_dq) for (int k = 0; k < 4; k++) d_dq[4 * a + k] = dr[k];
}

// ---------------------------------------------------------------------------------------------------
// L1 photometric loss (S3Gaussian/utils/loss_utils.py:21-22, train.py:226): mean |a - b| and its gradient
// sign(a - b) / n in one pass (the reference spends ~9 element-wise launches on it per step).
// ---------------------------------------------------------------------------------------------------
#define L1_THREADS 1024      // (the block count is capped by the same-address atomics below: wide blocks keep enough bytes in flight)
// TICKET (round 5): `loss` needs no zero fill in front of the kernel -- that fill was a launch of its own (4.6 us for 4 bytes in the replayed
// step).  Every workgroup publishes its partial sum as ONE aligned 8-byte {value, tag = 1} granule (a single device-scope store: no fence, no
// wait -- MI355X_MICROARCH.md, "R2's granule needs no ordering at all") in a caller-kept scratch table that is zero between calls; workgroup 0
// polls the table with device-scope loads, adds the partials in workgroup order (a deterministic sum, unlike the float atomics it replaces),
// writes the loss and clears the tags for the next call.  Nobody but workgroup 0 waits for anything, so the scheme cannot deadlock however
// few workgroups are resident.  (First built with a returning atomic add + a ticket per workgroup: two serialised memory round trips at the
// end of EVERY workgroup made the kernel 5.8 us longer than the 4.6 us fill it replaced.)
template <bool TICKET>
__global__ void __launch_bounds__(L1_THREADS) k_l1_loss(size_t n, const float* __restrict__ a, const float* __restrict__ b,
                                                        float inv_n, float* __restrict__ loss, float* __restrict__ grad, uint32_t* __restrict__ scratch) {
    __shared__ float s_part[L1_THREADS / 64];
    float acc = 0.f;
    const size_t n4 = n / 4, stride = (size_t)gridDim.x * L1_THREADS;
    for (size_t i = (size_t)blockIdx.x * L1_THREADS + threadIdx.x; i < n4; i += stride) {
        const float4 x = ((const float4*)a)[i], y = b ? ((const float4*)b)[i] : make_float4(0.f, 0.f, 0.f, 0.f);   // b == NULL: mean |a|
        const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
        acc += (fabsf(d0) + fabsf(d1)) + (fabsf(d2) + fabsf(d3));
        if (grad) {
            auto sg = [inv_n](float d) { return d > 0.f ? inv_n : (d < 0.f ? -inv_n : 0.f); };
            ((float4*)grad)[i] = make_float4(sg(d0), sg(d1), sg(d2), sg(d3));
        }
    }
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * L1_THREADS + threadIdx.x; i < n; i += stride) {
        const float d = a[i] - (b ? b[i] : 0.f);
        acc += fabsf(d);
        if (grad) grad[i] = d > 0.f ? inv_n : (d < 0.f ? -inv_n : 0.f);
    }
    acc = wave_reduce_to_lane63(acc);
    if ((threadIdx.x & 63) == 63) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < L1_THREADS / 64; w++) t += s_part[w];
        if (!TICKET) { atomicAdd(loss, t * inv_n); return; }
        unsigned long long* tab = reinterpret_cast<unsigned long long*>(scratch);
        const unsigned long long mine = ((unsigned long long)__float_as_uint(t * inv_n) << 32) | 1ull;
        if (blockIdx.x != 0) __hip_atomic_store(tab + blockIdx.x, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else s_part[0] = t * inv_n;
    }
    if (TICKET && blockIdx.x == 0) {
        __syncthreads();
        // one poller per other workgroup (gridDim.x <= 512 <= L1_THREADS): spin on ITS granule, hand the value to thread 0 through LDS
        unsigned long long* tab = reinterpret_cast<unsigned long long*>(scratch);
        float v = threadIdx.x == 0 ? s_part[0] : 0.f;
        if (threadIdx.x > 0 && threadIdx.x < gridDim.x) {
            unsigned long long g = 0ull;
            for (;;) {
                g = __hip_atomic_load(tab + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (g & 1ull) break;
                __builtin_amdgcn_s_sleep(2);
            }
            v = __uint_as_float((uint32_t)(g >> 32));
            __hip_atomic_store(tab + threadIdx.x, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the table is zero again for the next call
        }
        __syncthreads();                                      // (thread 0 has read s_part[0])
        v = wave_reduce_to_lane63(v);                         // a fixed tree: the same sum for the same partials
        if ((threadIdx.x & 63) == 63) s_part[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < L1_THREADS / 64; w++) tot += s_part[w];
            loss[0] = tot;
        }
    }
}

__global__ void __launch_bounds__(EMD_BLOCK) k_abs_mean_backward(size_t n, const float* __restrict__ x, const float* __restrict__ g, float inv_n,
                                                                 float* __restrict__ out) {
    const float s = g[0] * inv_n;
    const size_t n4 = n / 4, stride = (size_t)gridDim.x * EMD_BLOCK;
    auto sg = [s](float d) { return d > 0.f ? s : (d < 0.f ? -s : 0.f); };
    for (size_t i = (size_t)blockIdx.x * EMD_BLOCK + threadIdx.x; i < n4; i += stride) {
        const float4 v = ((const float4*)x)[i];
        ((float4*)out)[i] = make_float4(sg(v.x), sg(v.y), sg(v.z), sg(v.w));
    }
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * EMD_BLOCK + threadIdx.x; i < n; i += stride) out[i] = sg(x[i]);
}

// The same for a PAIR of residuals that also carry an upstream gradient (the fine stage's dshs_coarse / dshs_fine: both receive the
// rasterizer's dL/dshs -- usually the very same tensor -- plus the gradient of their L1 regulariser):
//   out_a[i] = up_a[i] + sign(x_a[i]) g_a[0] / n,   out_b[i] = up_b[i] + sign(x_b[i]) g_b[0] / n
// in one pass that reads the shared upstream gradient once (instead of two sign passes and two adds over [N,16,3]).
__global__ void __launch_bounds__(EMD_BLOCK) k_residual_l1_backward(size_t n, const float* __restrict__ up_a, const float* __restrict__ up_b,
                                                                    const float* __restrict__ x_a, const float* __restrict__ x_b,
                                                                    const float* __restrict__ g_a, const float* __restrict__ g_b, float inv_n,
                                                                    float* __restrict__ out_a, float* __restrict__ out_b) {
    const float sa = g_a ? g_a[0] * inv_n : 0.f, sb = g_b ? g_b[0] * inv_n : 0.f;
    const size_t n4 = n / 4, stride = (size_t)gridDim.x * EMD_BLOCK;
    auto sg = [](float d, float s) { return d > 0.f ? s : (d < 0.f ? -s : 0.f); };
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (size_t i = (size_t)blockIdx.x * EMD_BLOCK + threadIdx.x; i < n4; i += stride) {
        const float4 ua = up_a ? ((const float4*)up_a)[i] : z;
        const float4 ub = (up_b == up_a) ? ua : (up_b ? ((const float4*)up_b)[i] : z);
        const float4 a = ((const float4*)x_a)[i], b = ((const float4*)x_b)[i];
        ((float4*)out_a)[i] = make_float4(ua.x + sg(a.x, sa), ua.y + sg(a.y, sa), ua.z + sg(a.z, sa), ua.w + sg(a.w, sa));
        ((float4*)out_b)[i] = make_float4(ub.x + sg(b.x, sb), ub.y + sg(b.y, sb), ub.z + sg(b.z, sb), ub.w + sg(b.w, sb));
    }
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * EMD_BLOCK + threadIdx.x; i < n; i += stride) {
        out_a[i] = (up_a ? up_a[i] : 0.f) + sg(x_a[i], sa);
        out_b[i] = (up_b ? up_b[i] : 0.f) + sg(x_b[i], sb);
    }
}

}  // namespace

int emd_launch_residual_l1_backward(size_t n, const float* up_a, const float* up_b, const float* x_a, const float* x_b, const float* g_a,
                                    const float* g_b, float* out_a, float* out_b, hipStream_t st) {
    if (n == 0) return EMD_OK;
    size_t blocks = (n / 4 + EMD_BLOCK - 1) / EMD_BLOCK;
    if (blocks < 1) blocks = 1;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_residual_l1_backward, dim3((unsigned)blocks), dim3(EMD_BLOCK), 0, st, n, up_a, up_b, x_a, x_b, g_a, g_b, 1.f / (float)n,
                       out_a, out_b);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_abs_mean_backward(size_t n, const float* x, const float* g, float* out, hipStream_t st) {
    if (n == 0) return EMD_OK;
    size_t blocks = (n / 4 + EMD_BLOCK - 1) / EMD_BLOCK;
    if (blocks < 1) blocks = 1;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_abs_mean_backward, dim3((unsigned)blocks), dim3(EMD_BLOCK), 0, st, n, x, g, 1.f / (float)n, out);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_motion_forward(int n, const float* means, const float* quats, const float* opac, const EmdMotion& mo,
                              float* wm, float* wq, float* wo, hipStream_t st) {
    if (n <= 0) return EMD_OK;
    hipLaunchKernelGGL(k_motion_forward, dim3((n + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, st, n, means, quats,
                       opac, mo, wm, wq, wo);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_sh_forward(int n, int deg, int M, const float* dirs, const float* coeffs, float* rgb, hipStream_t st) {
    if (n <= 0) return EMD_OK;
    hipLaunchKernelGGL(k_sh_forward, dim3((n + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, st, n, deg, M, dirs,
                       coeffs, rgb);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_motion_backward(int n, const float* means, const float* quats, const float* opac, const EmdMotion& mo,
                               const float* g_wm, const float* g_wq, const float* g_wo, float* d_means, float* d_quats,
                               float* d_opac, float* d_pose, float* d_rdx, float* d_rdq, hipStream_t st) {
    if (n <= 0) return EMD_OK;
    hipLaunchKernelGGL(k_motion_backward, dim3((n + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, st, n, means, quats,
                       opac, mo, g_wm, g_wq, g_wo, d_means, d_quats, d_opac, d_pose, d_rdx, d_rdq);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_motion_backward_det(int n, const float* means, const float* quats, const float* opac, const EmdMotion& mo,
                                   const float* g_wm, const float* g_wq, const float* g_wo, float* d_means, float* d_quats,
                                   float* d_opac, float* d_rdx, float* d_rdq, float* pose_rows, uint32_t* keys_in, hipStream_t st) {
    if (n <= 0) return EMD_OK;
    hipLaunchKernelGGL(k_motion_backward_det, dim3((n + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, st, n, means, quats,
                       opac, mo, g_wm, g_wq, g_wo, d_means, d_quats, d_opac, d_rdx, d_rdq, pose_rows, keys_in);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_sh_backward(int n, int deg, int M, const float* dirs, const float* coeffs, const float* g_rgb,
                           float* d_coeffs, float* d_dirs, hipStream_t st) {
    if (n <= 0) return EMD_OK;
    hipLaunchKernelGGL(k_sh_backward, dim3((n + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, st, n, deg, M, dirs,
                       coeffs, g_rgb, d_coeffs, d_dirs);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_sh_grad_from_factors(int n, int V, int deg, int M, const float* means, const EmdMotion& mo, int pose_per_view,
                                    const float* campos, const float* gc, float scale, float* d_shs, hipStream_t st) {
    if (n <= 0) return EMD_OK;
    if (M != 16) { emd_set_error("sh_grad_from_factors: the staged row store needs sh_coeffs == 16"); return EMD_ERR_INVALID; }
    hipLaunchKernelGGL(k_sh_grad_from_factors, dim3((n + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, st, n, V, deg, means, mo, pose_per_view, campos,
                       gc, scale, d_shs);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_densification_stats(int n, const int32_t* radii, const float* g2d, float* accum, float* denom, float* max_radii,
                                   hipStream_t st) {
    if (n <= 0) return EMD_OK;
    hipLaunchKernelGGL(k_densification_stats, dim3((n + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, st, n, radii, g2d, accum, denom,
                       max_radii);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_activations(int n, const float* ls, float* sc, const float* rq, float* q, const float* lo, float* o, hipStream_t st) {
    if (n <= 0) return EMD_OK;
    hipLaunchKernelGGL(k_activations, dim3((n + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, st, n, ls, sc, rq, q, lo, o);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_actor_pose_forward(int A, const float* q, const float* t, const uint8_t* valid, const float* dt, const float* dq,
                                  float* pose, const int32_t* frame_dev, hipStream_t st) {
    if (A <= 0) return EMD_OK;
    hipLaunchKernelGGL(k_actor_pose_forward, dim3((A + 63) / 64), dim3(64), 0, st, A, q, t, valid, dt, dq, pose, frame_dev);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_actor_pose_backward(int A, const float* q, const float* dt, const float* dq, const float* g_pose, float* d_q,
                                   float* d_t, float* d_dt, float* d_dq, const int32_t* frame_dev, hipStream_t st) {
    if (A <= 0) return EMD_OK;
    hipLaunchKernelGGL(k_actor_pose_backward, dim3((A + 63) / 64), dim3(64), 0, st, A, q, dt, dq, g_pose, d_q, d_t, d_dt, d_dq, frame_dev);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_l1_loss(size_t n, const float* a, const float* b, float* loss, float* grad, uint32_t* scratch, hipStream_t st) {
    if (!scratch || n == 0) { int zrc = emd_zero_async(loss, sizeof(float), st); if (zrc) return zrc; }
    if (n == 0) return EMD_OK;
    size_t blocks = (n / 4 + L1_THREADS - 1) / L1_THREADS;
    if (blocks > 512) blocks = 512;     // one same-address float atomic per block: 2048 of them serialised for ~20 us
    if (blocks == 0) blocks = 1;
    if (scratch) hipLaunchKernelGGL((k_l1_loss<true>), dim3((unsigned)blocks), dim3(L1_THREADS), 0, st, n, a, b, 1.0f / (float)n, loss, grad, scratch);
    else hipLaunchKernelGGL((k_l1_loss<false>), dim3((unsigned)blocks), dim3(L1_THREADS), 0, st, n, a, b, 1.0f / (float)n, loss, grad, scratch);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}
