// quat_math.h -- quaternion arithmetic and the per-actor pose row, shared by the includers of gaussian_math.h (which includes this header) and by
// embed.hip.  embed.hip is built with the default contraction and cannot take gaussian_math.h's file-scope pragma (the track heads' bits would
// change), so there is NO file-scope pragma here: every function with a multiply-add in it carries `#pragma clang fp contract(off)` itself and
// gives the same individually rounded fp32 operations in every unit, whatever the unit's flags.
#pragma once

namespace {

__device__ __forceinline__ void quat_mul(const float a[4], const float b[4], float o[4]) {
#pragma clang fp contract(off)
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

__device__ __forceinline__ float quat_norm(const float q[4]) {
#pragma clang fp contract(off)
    return sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
}

__device__ __forceinline__ void dnormalize4(const float vu[4], float n, const float g[4], float out[4]) {
#pragma clang fp contract(off)
    float dot = ((vu[0] * g[0] + vu[1] * g[1]) + vu[2] * g[2]) + vu[3] * g[3];
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = (g[k] - vu[k] * dot) / n;
}

__device__ __forceinline__ bool any_nan(const float* v, int n) {
    bool b = false;
    for (int k = 0; k < n; k++) b |= !(v[k] == v[k]);
    return b;
}

// ---------------------------------------------------------------------------------------------------
// One row of the per-frame actor pose table (training branch of rigid.py:478-568), on values in registers; the callers load and store
// (k_actor_pose_forward / _backward in standalone_ops.hip: one lane per actor; k_tracked_pose in embed.hip: one workgroup per actor).
//   row[0..3]  = normalize(q)                   rotation applied to local means          (rigid.py:499-503)
//   row[4..6]  = t + dt                                                                   (rigid.py:519-532)
//   row[7]     = valid
//   row[8..11] = normalize(q (x) dq)            composed onto local quaternions           (rigid.py:547-566)
// dt / dq are the learned offsets: absent (has_dt / has_dq false: no offsets) or with a NaN component means skipped (rigid.py:528,559 `continue`).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pose_compose(const float q[4], bool has_dq, const float dq[4], float p[4]) {      // -> whether dq was applied
    const bool use_r = has_dq && !any_nan(dq, 4);
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = q[k];
    if (use_r) quat_mul(q, dq, p);
    return use_r;
}

__device__ __forceinline__ void pose_row_forward(const float q[4], const float t[3], bool has_dt, const float dt[3], bool has_dq, const float dq[4], float valid,
                                                 float row[12]) {
#pragma clang fp contract(off)
    const float n = fmaxf(quat_norm(q), 1e-12f);
    const bool ok_t = has_dt && !any_nan(dt, 3);
    float p[4];
    pose_compose(q, has_dq, dq, p);
    const float n2 = fmaxf(quat_norm(p), 1e-12f);
#pragma unroll
    for (int k = 0; k < 4; k++) { row[k] = q[k] / n; row[8 + k] = p[k] / n2; }
#pragma unroll
    for (int k = 0; k < 3; k++) row[4 + k] = ok_t ? t[k] + dt[k] : t[k];
    row[7] = valid;
}

// G = d L / d row.  -> dqf = d L / d q, ddt = d L / d dt (zero where dt is skipped; d L / d t is G[4..6] as it stands), dr = d L / d dq
__device__ __forceinline__ void pose_row_backward(const float q[4], bool has_dt, const float dt[3], bool has_dq, const float dq[4], const float G[12], float dqf[4],
                                                  float ddt[3], float dr[4]) {
#pragma clang fp contract(off)
    const float n = fmaxf(quat_norm(q), 1e-12f);
    const float qu[4] = {q[0] / n, q[1] / n, q[2] / n, q[3] / n};
    dnormalize4(qu, n, G, dqf);
    float p[4], dp[4];
    const bool use_r = pose_compose(q, has_dq, dq, p);
    const float n2 = fmaxf(quat_norm(p), 1e-12f);
    const float pu[4] = {p[0] / n2, p[1] / n2, p[2] / n2, p[3] / n2};
    dnormalize4(pu, n2, G + 8, dp);
    dr[0] = dr[1] = dr[2] = dr[3] = 0.f;
    if (use_r) {   // p = q (x) r : dL/dq = dp (x) conj(r), dL/dr = conj(q) (x) dp
        const float rc[4] = {dq[0], -dq[1], -dq[2], -dq[3]}, qc[4] = {q[0], -q[1], -q[2], -q[3]};
        float t1[4];
        quat_mul(dp, rc, t1);
        quat_mul(qc, dp, dr);
#pragma unroll
        for (int k = 0; k < 4; k++) dqf[k] += t1[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) dqf[k] += dp[k];
    }
    const bool ok_t = has_dt && !any_nan(dt, 3);
#pragma unroll
    for (int k = 0; k < 3; k++) ddt[k] = ok_t ? G[4 + k] : 0.f;
}

}  // namespace
