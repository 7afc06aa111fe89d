// gaussian_math.h -- per-Gaussian device math shared by the projection kernels (preprocess.hip) and the stand-alone entry points
// (standalone_ops.hip): quaternions, the explicit-motion model and its backward, the SH basis and its direction derivative, cov3D.
// Two things here are not math but are needed on both sides: SH_ROW4, the padded LDS row of the SH staging (K1, K8, k_sh_grad_from_factors),
// and reduce_pose_grad, the wave-level reduction + atomic add of the actor-pose gradient (K8, k_motion_backward).
//
// EVERY includer is built with -ffp-contract=off (csrc/Makefile): this arithmetic is a bit-exact contract with oracle/raster_oracle.c --
// the view depth (sort key), radius and tile rectangle derive from it --, so every operation here is an individually rounded fp32 op in
// the documented order ("pinned evaluation order").  The pragma below says the same to a compiler that was not given the flag.
// quat_mul / quat_norm / dnormalize4 / any_nan and the actor pose row live in quat_math.h, which embed.hip includes too.
#pragma once
#include "common.h"
#include "device_utils.h"
#include "quat_math.h"

#pragma clang fp contract(off)

namespace {

__device__ const float SH_C0 = 0.28209479177387814f;
__device__ const float SH_C1 = 0.4886025119029199f;
__device__ const float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                   -1.0925484305920792f, 0.5462742152960396f};
__device__ const float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                   0.3731763325901154f,  -0.4570457994644658f, 1.445305721320277f,
                                   -0.5900435899266435f};

__device__ __forceinline__ void quat_to_R(const float q[4], float R[9]) {
    float r = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.f - 2.f * (y * y + z * z);
    R[1] = 2.f * (x * y - r * z);
    R[2] = 2.f * (x * z + r * y);
    R[3] = 2.f * (x * y + r * z);
    R[4] = 1.f - 2.f * (x * x + z * z);
    R[5] = 2.f * (y * z - r * x);
    R[6] = 2.f * (x * z - r * y);
    R[7] = 2.f * (y * z + r * x);
    R[8] = 1.f - 2.f * (x * x + y * y);
}

// World-space mean / quaternion / opacity of Gaussian i under the explicit-motion model.
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// raw = EMD_FLAG_RAW_PARAMS: opacities are logits (sigmoid here), static quaternions are un-normalised (normalised
// here, F.normalize eps 1e-12) -- the activations of S3Gaussian/gaussian_renderer/__init__.py:99-101 fused in.
// The arithmetic of motion_point on values already in registers (round 5: K8 issues every load of a Gaussian together before any of them is used):
// m = local mean (residual_dx applied), a = actor id or -1, q = the stored quaternion, dq_res = OmniRe's quaternion residual (dynamic points),
// op_in = the stored opacity, p0 / p1 / p2 = the actor's pose rows (read when a >= 0 only).
__device__ __forceinline__ void motion_apply(const float m[3], int a, bool has_q, float4 q, bool has_dq, float4 dq_res, bool has_op, float op_in, float4 p0,
                                             float4 p1, float4 p2, bool raw, float wm[3], float wq[4], float* wo) {
    if (a < 0) {
        wm[0] = m[0]; wm[1] = m[1]; wm[2] = m[2];
        if (has_q) {
            wq[0] = q.x; wq[1] = q.y; wq[2] = q.z; wq[3] = q.w;
            if (raw) { const float n = fmaxf(quat_norm(wq), 1e-12f); wq[0] /= n; wq[1] /= n; wq[2] /= n; wq[3] /= n; }
        }
        if (has_op) *wo = raw ? sigmoidf_(op_in) : op_in;
        return;
    }
    const float qm[4] = {p0.x, p0.y, p0.z, p0.w};
    float R[9];
    quat_to_R(qm, R);
    wm[0] = ((R[0] * m[0] + R[1] * m[1]) + R[2] * m[2]) + p1.x;
    wm[1] = ((R[3] * m[0] + R[4] * m[1]) + R[5] * m[2]) + p1.y;
    wm[2] = ((R[6] * m[0] + R[7] * m[1]) + R[8] * m[2]) + p1.z;
    if (has_q) {
        float ql[4] = {q.x, q.y, q.z, q.w};
        if (has_dq) { ql[0] += dq_res.x; ql[1] += dq_res.y; ql[2] += dq_res.z; ql[3] += dq_res.w; }
        float n = fmaxf(quat_norm(ql), 1e-12f);
        float qn[4] = {ql[0] / n, ql[1] / n, ql[2] / n, ql[3] / n};
        const float qr[4] = {p2.x, p2.y, p2.z, p2.w};
        float p[4];
        quat_mul(qr, qn, p);
        float n2 = fmaxf(quat_norm(p), 1e-12f);
        wq[0] = p[0] / n2; wq[1] = p[1] / n2; wq[2] = p[2] / n2; wq[3] = p[3] / n2;
    }
    if (has_op) *wo = (raw ? sigmoidf_(op_in) : op_in) * p1.w;
}

__device__ __forceinline__ void motion_point(int i, const float* __restrict__ means, const float* __restrict__ quats,
                                             const float* __restrict__ opac, const EmdMotion& mo, float wm[3],
                                             float wq[4], float* wo, bool raw = false) {
    float m[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    if (mo.residual_dx) {
        m[0] += mo.residual_dx[3 * i]; m[1] += mo.residual_dx[3 * i + 1]; m[2] += mo.residual_dx[3 * i + 2];
    }
    int a = mo.actor_id ? mo.actor_id[i] : -1;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 q = z4, dqr = z4, p0 = z4, p1 = z4, p2 = z4;
    if (quats) q = *(const float4*)(quats + 4 * i);
    if (a >= 0) {
        const float4* Pp = (const float4*)(mo.actor_pose + (size_t)a * EMD_ACTOR_STRIDE);
        p0 = Pp[0]; p1 = Pp[1]; p2 = Pp[2];
        if (quats && mo.residual_dq) dqr = *(const float4*)(mo.residual_dq + 4 * i);
    }
    motion_apply(m, a, quats != nullptr, q, mo.residual_dq != nullptr, dqr, opac != nullptr, opac ? opac[i] : 0.f, p0, p1, p2, raw, wm, wq, wo);
}

__device__ __forceinline__ void sh_basis(int deg, const float d[3], float b[16]) {
    float x = d[0], y = d[1], z = d[2];
    b[0] = SH_C0;
    if (deg > 0) {
        b[1] = -SH_C1 * y; b[2] = SH_C1 * z; b[3] = -SH_C1 * x;
        if (deg > 1) {
            float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            b[4] = SH_C2[0] * xy; b[5] = SH_C2[1] * yz; b[6] = SH_C2[2] * (2.f * zz - xx - yy);
            b[7] = SH_C2[3] * xz; b[8] = SH_C2[4] * (xx - yy);
            if (deg > 2) {
                b[9] = SH_C3[0] * y * (3.f * xx - yy);
                b[10] = SH_C3[1] * xy * z;
                b[11] = SH_C3[2] * y * (4.f * zz - xx - yy);
                b[12] = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy);
                b[13] = SH_C3[4] * x * (4.f * zz - xx - yy);
                b[14] = SH_C3[5] * z * (xx - yy);
                b[15] = SH_C3[6] * x * (xx - 3.f * yy);
            }
        }
    }
}

__device__ __forceinline__ void cov3d_from_sr(const float s[3], float mod, const float q[4], float c[6]) {
    float R[9], L[9];
    quat_to_R(q, R);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) L[3 * r + k] = R[3 * r + k] * (mod * s[k]);
    c[0] = (L[0] * L[0] + L[1] * L[1]) + L[2] * L[2];
    c[1] = (L[0] * L[3] + L[1] * L[4]) + L[2] * L[5];
    c[2] = (L[0] * L[6] + L[1] * L[7]) + L[2] * L[8];
    c[3] = (L[3] * L[3] + L[4] * L[4]) + L[5] * L[5];
    c[4] = (L[3] * L[6] + L[4] * L[7]) + L[5] * L[8];
    c[5] = (L[6] * L[6] + L[7] * L[7]) + L[8] * L[8];
}

// d colour / d (unit) direction contracted with the colour gradient gc: gd = sum_k d basis_k/d dir * (sh[k] . gc)
__device__ __forceinline__ void sh_dir_backward(int deg, const float d[3], const float* __restrict__ sh,
                                                const float gc[3], float gd[3]) {
    const float x = d[0], y = d[1], z = d[2];
    gd[0] = gd[1] = gd[2] = 0.f;
#define SDOT(k) ((sh[3 * (k)] * gc[0] + sh[3 * (k) + 1] * gc[1]) + sh[3 * (k) + 2] * gc[2])
    if (deg > 0) {
        gd[1] += -SH_C1 * SDOT(1); gd[2] += SH_C1 * SDOT(2); gd[0] += -SH_C1 * SDOT(3);
        if (deg > 1) {
            float xx = x * x, yy = y * y, zz = z * z;
            float s4 = SDOT(4), s5 = SDOT(5), s6 = SDOT(6), s7 = SDOT(7), s8 = SDOT(8);
            gd[0] += SH_C2[0] * y * s4 + SH_C2[2] * -2.f * x * s6 + SH_C2[3] * z * s7 + SH_C2[4] * 2.f * x * s8;
            gd[1] += SH_C2[0] * x * s4 + SH_C2[1] * z * s5 + SH_C2[2] * -2.f * y * s6 + SH_C2[4] * -2.f * y * s8;
            gd[2] += SH_C2[1] * y * s5 + SH_C2[2] * 4.f * z * s6 + SH_C2[3] * x * s7;
            if (deg > 2) {
                float s9 = SDOT(9), s10 = SDOT(10), s11 = SDOT(11), s12 = SDOT(12), s13 = SDOT(13),
                      s14 = SDOT(14), s15 = SDOT(15);
                gd[0] += SH_C3[0] * 6.f * x * y * s9 + SH_C3[1] * y * z * s10 + SH_C3[2] * -2.f * x * y * s11 +
                         SH_C3[3] * -6.f * x * z * s12 + SH_C3[4] * (4.f * zz - 3.f * xx - yy) * s13 +
                         SH_C3[5] * 2.f * x * z * s14 + SH_C3[6] * (3.f * xx - 3.f * yy) * s15;
                gd[1] += SH_C3[0] * (3.f * xx - 3.f * yy) * s9 + SH_C3[1] * x * z * s10 +
                         SH_C3[2] * (4.f * zz - xx - 3.f * yy) * s11 + SH_C3[3] * -6.f * y * z * s12 +
                         SH_C3[4] * -2.f * x * y * s13 + SH_C3[5] * -2.f * y * z * s14 +
                         SH_C3[6] * -6.f * x * y * s15;
                gd[2] += SH_C3[1] * x * y * s10 + SH_C3[2] * 8.f * y * z * s11 +
                         SH_C3[3] * (6.f * zz - 3.f * xx - 3.f * yy) * s12 + SH_C3[4] * 8.f * x * z * s13 +
                         SH_C3[5] * (xx - yy) * s14;
            }
        }
    }
#undef SDOT
}

// d colour_c / d (unit direction) for the three channels: J[3 c + axis] = sum_k d basis_k / d axis * sh[k][c].
// K1 stores it (36 B) so that K8 gets d L / d dir = J^T gc without touching the SH coefficients again.
__device__ __forceinline__ void sh_dir_jacobian(int deg, const float d[3], const float* __restrict__ sh, float J[9]) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float gc[3] = {0.f, 0.f, 0.f};
        gc[c] = 1.f;
        sh_dir_backward(deg, d, sh, gc, J + 3 * c);
    }
}

// A 192-byte SH row ([16][3] floats) staged in LDS is padded to 13 float4 (52 dwords): 52 t mod 64 takes 16 distinct multiples of 4, so a
// ds_read_b128 lane group is conflict-free (the staging itself: "SH rows through LDS", preprocess.hip).
#define SH_ROW4 13

__device__ __forceinline__ void dR_to_dq(const float q[4], const float dR[9], float dq[4]) {
    float r = q[0], x = q[1], y = q[2], z = q[3];
    dq[0] = 2.f * (-z * dR[1] + y * dR[2] + z * dR[3] - x * dR[5] - y * dR[6] + x * dR[7]);
    dq[1] = 2.f * (y * dR[1] + z * dR[2] + y * dR[3] - 2.f * x * dR[4] - r * dR[5] + z * dR[6] + r * dR[7] - 2.f * x * dR[8]);
    dq[2] = 2.f * (-2.f * y * dR[0] + x * dR[1] + r * dR[2] + x * dR[3] + z * dR[5] - r * dR[6] + z * dR[7] - 2.f * y * dR[8]);
    dq[3] = 2.f * (-2.f * z * dR[0] - r * dR[1] + x * dR[2] + r * dR[3] - 2.f * z * dR[4] + y * dR[5] + x * dR[6] + y * dR[7]);
}

// Backward of motion_point for an actor point (a_id >= 0): world-space gradients (dm, dq, dop) -> local-space
// gradients (dl, dql, dopl) and this point's contribution to its actor's pose row (pose_g[12]).
// (the arithmetic on values in registers; motion_point_backward below loads them)
__device__ __forceinline__ void motion_backward_apply(const float ml[3], bool has_q, float4 qq, bool has_dq, float4 dq_res, bool has_op, float op_in,
                                                      float4 p0, float4 p1, float4 p2, const float dm[3], const float dq[4], float dop, float dl[3],
                                                      float dql[4], float* dopl, float pose_g[12], bool raw) {
    const float qm[4] = {p0.x, p0.y, p0.z, p0.w};
    float R[9];
    quat_to_R(qm, R);
#pragma unroll
    for (int k = 0; k < 3; k++) dl[k] = (R[k] * dm[0] + R[3 + k] * dm[1]) + R[6 + k] * dm[2];
    float dRm[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) dRm[3 * r + k] = dm[r] * ml[k];
    float dqm[4];
    dR_to_dq(qm, dRm, dqm);
    pose_g[0] = dqm[0]; pose_g[1] = dqm[1]; pose_g[2] = dqm[2]; pose_g[3] = dqm[3];
    pose_g[4] = dm[0]; pose_g[5] = dm[1]; pose_g[6] = dm[2];
    pose_g[7] = has_op ? dop * (raw ? sigmoidf_(op_in) : op_in) : 0.f;
    pose_g[8] = pose_g[9] = pose_g[10] = pose_g[11] = 0.f;
    dql[0] = dql[1] = dql[2] = dql[3] = 0.f;
    if (has_q) {
        float ql[4] = {qq.x, qq.y, qq.z, qq.w};
        if (has_dq) { ql[0] += dq_res.x; ql[1] += dq_res.y; ql[2] += dq_res.z; ql[3] += dq_res.w; }
        float n = fmaxf(quat_norm(ql), 1e-12f);
        float qn[4] = {ql[0] / n, ql[1] / n, ql[2] / n, ql[3] / n};
        const float qr[4] = {p2.x, p2.y, p2.z, p2.w};
        float pp[4];
        quat_mul(qr, qn, pp);
        float n2 = fmaxf(quat_norm(pp), 1e-12f);
        float pu[4] = {pp[0] / n2, pp[1] / n2, pp[2] / n2, pp[3] / n2};
        float dp[4];
        dnormalize4(pu, n2, dq, dp);
        // p = a (x) b : dL/da = g (x) conj(b), dL/db = conj(a) (x) g
        const float bc[4] = {qn[0], -qn[1], -qn[2], -qn[3]}, ac[4] = {qr[0], -qr[1], -qr[2], -qr[3]};
        float dqa[4], dqb[4];
        quat_mul(dp, bc, dqa);
        quat_mul(ac, dp, dqb);
        pose_g[8] = dqa[0]; pose_g[9] = dqa[1]; pose_g[10] = dqa[2]; pose_g[11] = dqa[3];
        dnormalize4(qn, n, dqb, dql);
    }
    *dopl = dop * p1.w;
}

__device__ __forceinline__ void motion_point_backward(int i, int a_id, const float* __restrict__ means,
                                                      const float* __restrict__ quats, const float* __restrict__ opac,
                                                      const EmdMotion& mo, const float dm[3], const float dq[4],
                                                      float dop, float dl[3], float dql[4], float* dopl,
                                                      float pose_g[12], bool raw = false) {
    const float4* Pp = (const float4*)(mo.actor_pose + (size_t)a_id * EMD_ACTOR_STRIDE);
    const float4 p0 = Pp[0], p1 = Pp[1], p2 = Pp[2];
    float ml[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    if (mo.residual_dx) { ml[0] += mo.residual_dx[3 * i]; ml[1] += mo.residual_dx[3 * i + 1]; ml[2] += mo.residual_dx[3 * i + 2]; }
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 qq = z4, dqr = z4;
    if (quats) {
        qq = *(const float4*)(quats + 4 * i);
        if (mo.residual_dq) dqr = *(const float4*)(mo.residual_dq + 4 * i);
    }
    motion_backward_apply(ml, quats != nullptr, qq, mo.residual_dq != nullptr, dqr, opac != nullptr, opac ? opac[i] : 0.f, p0, p1, p2, dm, dq, dop, dl, dql,
                          dopl, pose_g, raw);
}

// Segmented reduction of per-point pose gradients into dL_dactor_pose.  Actor points are stored contiguously
// per instance (rigid.py:53-145), so most waves hold one actor id: DPP wave sum, one atomic row per wave -- as ONE
// wave-instruction with twelve lanes.  Float atomics execute at the memory side, one 64-byte request per wave-instruction, and
// all of an actor's adds land on the same line or two: twelve one-lane adds per wave (30 000 requests onto 12 lines in the
// headline step) held K8 at 0.19 ms, 0.15 without any (profiles/r07_preprocess_ab.txt).  A wave holding several ids adds lane by lane.
// (the sums reach lanes 0..11 through readlane: the same thing through LDS costs K8 six spilled registers)
__device__ __forceinline__ void reduce_pose_grad(int a_id, const float pose_g[12], float* __restrict__ dL_dpose) {
    const unsigned long long has = __ballot(a_id >= 0);
    if (!has) return;
    const int first = __ffsll((long long)has) - 1;
    const int a0 = __builtin_amdgcn_readlane(a_id, first);
    const bool uniform = __ballot(a_id >= 0 && a_id != a0) == 0ull;
    if (uniform) {
        const int lane = threadIdx.x & 63;
        float mine = 0.f;                   // lane k < 12: component k of the wave's sum
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const float v = wave_reduce_to_lane63(a_id >= 0 ? pose_g[k] : 0.f);
            const float t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
            mine = lane == k ? t : mine;
        }
        if (lane < 12) atomicAdd(dL_dpose + (size_t)a0 * EMD_ACTOR_STRIDE + lane, mine);
    } else if (a_id >= 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) atomicAdd(dL_dpose + (size_t)a_id * EMD_ACTOR_STRIDE + k, pose_g[k]);
    }
}

}  // namespace
