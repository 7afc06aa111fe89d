// camera_grad.hip -- dL/d(viewmatrix, projmatrix, campos) of one rasterizer call: the opt-in kernel between the two halves of the backward
// (K7 has filled the per-Gaussian accumulator rows, K8 has not consumed them yet).  gfx950, one Gaussian per lane.
//
// Every entry of EmdSettings.viewmatrix / projmatrix / campos that K1 reads is a free variable; the 35 outputs are laid out as the settings
// block is (V[16], P[16], campos[3]); the entries K1 never reads (V[3], V[7], V[11], V[15], the z column of P) get an exact 0.f.  The chain
// rule from these numbers to a camera pose stays with the caller (4x4 tensors).  The per-Gaussian arithmetic is K8's (preprocess.hip),
// term for term and in K8's order, so that both read the same fp32 intermediates; the accumulator rows are READ only (K8 consumes and
// clears them afterwards).  DESIGN.md, "Camera gradients", lists the terms.
//
// Reduction, deterministic (two replicas of a data-parallel step get the same bits): no float atomics, no fences, no look-back.
//   lane: 27 live terms in fp32 -> wave: DPP sum (wave_reduce_to_lane63) -> workgroup: the four waves' sums meet in LDS (plain stores, a
//   barrier, plain reads; added in wave order) -> one row of 36 floats per workgroup in a caller-owned buffer (nine 16-byte stores) ->
//   k_camera_reduce, ONE workgroup: the rows added in a fixed order in fp64, 35 fp32 results.
// Nothing depends on the order in which the grid's workgroups run.
//
// Built like preprocess.hip (-ffp-contract=off: gaussian_math.h's contract; K8's intermediates bit for bit).
#include "common.h"
#include "device_utils.h"
#include "gaussian_math.h"

#pragma clang fp contract(off)

namespace {

// project_cov2d of preprocess.hip restated (that file's instruction schedule is pinned, so nothing is moved out of it): everything up to
// cov2D of one visible Gaussian, the same operations in the same order.
struct CamProj {
    float tx, ty, tz, cx, cy;
    bool clx, cly;
    float J00, J02, J11, J12;
    float T0[3], T1[3];
    float a, b, c, det;
};

__device__ __forceinline__ void cam_project_cov2d(const EmdSettings& S, const float c3[6], float fx, float fy, CamProj& p) {
    const float* V = S.viewmatrix;
    float limx = 1.3f * S.tanfovx, limy = 1.3f * S.tanfovy;
    float txtz = p.tx / p.tz, tytz = p.ty / p.tz;
    p.clx = (txtz < -limx) || (txtz > limx);
    p.cly = (tytz < -limy) || (tytz > limy);
    p.cx = fminf(limx, fmaxf(-limx, txtz)) * p.tz;
    p.cy = fminf(limy, fmaxf(-limy, tytz)) * p.tz;
    p.J00 = fx / p.tz; p.J02 = -(fx * p.cx) / (p.tz * p.tz); p.J11 = fy / p.tz; p.J12 = -(fy * p.cy) / (p.tz * p.tz);
    float M0[3], M1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        M0[k] = p.J00 * V[4 * k + 0] + p.J02 * V[4 * k + 2];
        M1[k] = p.J11 * V[4 * k + 1] + p.J12 * V[4 * k + 2];
    }
    const float Sg[9] = {c3[0], c3[1], c3[2], c3[1], c3[3], c3[4], c3[2], c3[4], c3[5]};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        p.T0[k] = (M0[0] * Sg[k] + M0[1] * Sg[3 + k]) + M0[2] * Sg[6 + k];
        p.T1[k] = (M1[0] * Sg[k] + M1[1] * Sg[3 + k]) + M1[2] * Sg[6 + k];
    }
    p.a = ((p.T0[0] * M0[0] + p.T0[1] * M0[1]) + p.T0[2] * M0[2]) + 0.3f;
    p.b = (p.T0[0] * M1[0] + p.T0[1] * M1[1]) + p.T0[2] * M1[2];
    p.c = ((p.T1[0] * M1[0] + p.T1[1] * M1[1]) + p.T1[2] * M1[2]) + 0.3f;
    p.det = p.a * p.c - p.b * p.b;
}

#define CAM_BLOCK 256
#define CAM_WAVES (CAM_BLOCK / 64)
#define CAM_OUT 35            // V[16] | P[16] | campos[3]
#define CAM_ROW 36            // a workgroup's row: the 35 outputs + one pad float = nine float4
#define CAM_LIVE 27           // entries K1 reads: V[4k+r] r < 3 (slots 0..11), P[4k+j] j != 2 (12..23), campos (24..26)

// slot of output entry e among the live terms, or -1 for an entry K1 never reads (and the pad)
__device__ __forceinline__ int cam_slot(int e) {
    if (e < 16) return (e & 3) < 3 ? 3 * (e >> 2) + (e & 3) : -1;
    if (e < 32) { const int j = (e - 16) & 3, k = (e - 16) >> 2; return j == 2 ? -1 : 12 + 3 * k + (j == 3 ? 2 : j); }
    return e < CAM_OUT ? 24 + (e - 32) : -1;
}

__global__ void __launch_bounds__(CAM_BLOCK) k_camera_backward(PreBwdArgs a, float* __restrict__ partials) {
    EmdSettings S = a.s;
    emd_settings_from_device(S, a.sdev, a.flags);
    __shared__ float s_part[CAM_WAVES][CAM_LIVE + 1];
    const int i = blockIdx.x * CAM_BLOCK + threadIdx.x;
    const bool vis = i < a.N && emd_bwd_visible_words(a.flags, a.radii, a.g)[i] > 0;     // (K8's set: a Gaussian K7 never added to has an all-zero row)
    float acc[CAM_LIVE];
#pragma unroll
    for (int k = 0; k < CAM_LIVE; k++) acc[k] = 0.f;
    float* dV = acc;              // dV[3 k + r] = dL/dV[4 k + r]
    float* dP = acc + 12;         // dP[3 k + (0, 1, 2)] = dL/dP[4 k + (0, 1, 3)]
    float* dC = acc + 24;
    if (vis) {
        const float* V = S.viewmatrix;
        const float* P = S.projmatrix;
        const int W = S.image_width, H = S.image_height;
        const float fx = (float)W / (2.f * S.tanfovx), fy = (float)H / (2.f * S.tanfovy);
        const bool raw = (a.flags & EMD_FLAG_RAW_PARAMS) != 0;
        // as K8 part 1: every load whose address depends on the index alone is issued here, back to back, before any is used (an absent
        // array is read through the Gaussian's own accumulator row -- 48 readable, 16-byte aligned bytes -- and selected where it is used),
        // then the actor's pose rows, the one dependent address
        const bool motion = (a.flags & EMD_FLAG_MOTION) != 0;
        const bool has_ids = motion && a.motion.actor_id != nullptr, has_rot = a.rotations != nullptr;
        const bool has_rdx = motion && a.motion.residual_dx != nullptr, has_rdq = motion && has_rot && a.motion.residual_dq != nullptr;
        const float4 z4c = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4* gr = (const float4*)(a.grad_rec + (size_t)i * a.bwd_stride);
        const float* safe = (const float*)gr;
        const int aid_raw = *(has_ids ? a.motion.actor_id + i : a.radii + i);
        const float* mp = a.means3D + 3 * (size_t)i;
        const float* xp = has_rdx ? a.motion.residual_dx + 3 * (size_t)i : safe;
        const float* sp = a.cov3D_precomp ? safe : a.scales + 3 * (size_t)i;
        const float* cp = a.cov3D_precomp ? a.cov3D_precomp + 6 * (size_t)i : safe;
        const float4* jr = a.colors_precomp ? gr : a.g.shjac + (size_t)i * 3;
        const float m0 = mp[0], m1 = mp[1], m2 = mp[2];
        const float x0 = xp[0], x1 = xp[1], x2 = xp[2];
        const float4 qq = *(const float4*)(has_rot ? a.rotations + 4 * (size_t)i : safe);
        const float4 dqq = *(const float4*)(has_rdq ? a.motion.residual_dq + 4 * (size_t)i : safe);
        const float s0 = sp[0], s1 = sp[1], s2 = sp[2];
        const float c0 = cp[0], c1 = cp[1], c2 = cp[2], c3_ = cp[3], c4 = cp[4], c5 = cp[5];
        const float4 g0 = gr[0], g1 = gr[1], g2 = gr[2];
        const float4 j0 = jr[0], j1 = jr[1], j2 = jr[2];
        const int a_id = has_ids ? aid_raw : -1;
        float4 pr0 = z4c, pr1 = z4c, pr2 = z4c;
        if (a_id >= 0) {
            const float4* Pp = (const float4*)(a.motion.actor_pose + (size_t)a_id * EMD_ACTOR_STRIDE);
            pr0 = Pp[0]; pr1 = Pp[1]; pr2 = Pp[2];
        }
        // ---- the Gaussian's world pose, as K8 forms it (the opacity does not depend on the camera: not formed)
        float m[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, op_unused = 0.f;
        const float mloc[3] = {has_rdx ? m0 + x0 : m0, has_rdx ? m1 + x1 : m1, has_rdx ? m2 + x2 : m2};
        if (motion) motion_apply(mloc, a_id, has_rot, qq, has_rdq, dqq, false, 0.f, pr0, pr1, pr2, raw, m, q, &op_unused);
        else {
            m[0] = m0; m[1] = m1; m[2] = m2;
            if (has_rot) { q[0] = qq.x; q[1] = qq.y; q[2] = qq.z; q[3] = qq.w; }
        }
        if (raw && a_id < 0 && has_rot) {   // static point: the raw quaternion, normalised (F.normalize eps 1e-12)
            const float qr[4] = {qq.x, qq.y, qq.z, qq.w};
            const float q_norm = fmaxf(quat_norm(qr), 1e-12f);
            q[0] = qr[0] / q_norm; q[1] = qr[1] / q_norm; q[2] = qr[2] / q_norm; q[3] = qr[3] / q_norm;
        }
        const float g_depth = g0.z, gA = g1.x, gB = g1.y, gC = g1.z;
        const float gcol[3] = {g1.w, g2.x, g2.y};
        CamProj p;
        p.tx = ((V[0] * m[0] + V[4] * m[1]) + V[8] * m[2]) + V[12];
        p.ty = ((V[1] * m[0] + V[5] * m[1]) + V[9] * m[2]) + V[13];
        p.tz = ((V[2] * m[0] + V[6] * m[1]) + V[10] * m[2]) + V[14];
        // ---- SH colour: d colour / d campos = -d colour / d mean
        if (!a.colors_precomp) {
            float d0[3] = {m[0] - S.campos[0], m[1] - S.campos[1], m[2] - S.campos[2]};
            float n = sqrtf((d0[0] * d0[0] + d0[1] * d0[1]) + d0[2] * d0[2]);
            float d[3] = {d0[0] / n, d0[1] / n, d0[2] / n};
            const uint32_t bits = __float_as_uint(j0.w);        // (the clamp bits K1 left in the row's spare word)
            float gc[3];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) gc[ch] = ((bits >> ch) & 1u) ? 0.f : gcol[ch];
            float gd[3];
            gd[0] = (j0.x * gc[0] + j1.x * gc[1]) + j2.x * gc[2];
            gd[1] = (j0.y * gc[0] + j1.y * gc[1]) + j2.y * gc[2];
            gd[2] = (j0.z * gc[0] + j1.z * gc[1]) + j2.z * gc[2];
            float dot = (d[0] * gd[0] + d[1] * gd[1]) + d[2] * gd[2];
#pragma unroll
            for (int k = 0; k < 3; k++) dC[k] = -((gd[k] - d[k] * dot) / n);
        }
        // ---- covariance: conic -> cov2D -> M = J W (rows M0, M1), and J's own dependence on t
        float c3[6];
        if (a.cov3D_precomp) {
            c3[0] = c0; c3[1] = c1; c3[2] = c2; c3[3] = c3_; c3[4] = c4; c3[5] = c5;
        } else {
            float sc[3] = {s0, s1, s2};
            if (raw) { sc[0] = expf(sc[0]); sc[1] = expf(sc[1]); sc[2] = expf(sc[2]); }
            cov3d_from_sr(sc, S.scale_modifier, q, c3);
        }
        cam_project_cov2d(S, c3, fx, fy, p);
        float da = 0.f, db = 0.f, dc = 0.f;
        if (p.det != 0.f) {
            float i2 = 1.f / (p.det * p.det);
            da = (-p.c * p.c * gA + p.b * p.c * gB - p.b * p.b * gC) * i2;
            db = (2.f * p.b * p.c * gA - (p.a * p.c + p.b * p.b) * gB + 2.f * p.a * p.b * gC) * i2;
            dc = (-p.b * p.b * gA + p.a * p.b * gB - p.a * p.a * gC) * i2;
        }
        float dJ00 = 0.f, dJ02 = 0.f, dJ11 = 0.f, dJ12 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            float dM0 = 2.f * da * p.T0[k] + db * p.T1[k];
            float dM1 = 2.f * dc * p.T1[k] + db * p.T0[k];
            dJ00 += dM0 * V[4 * k + 0]; dJ02 += dM0 * V[4 * k + 2];
            dJ11 += dM1 * V[4 * k + 1]; dJ12 += dM1 * V[4 * k + 2];
            dV[3 * k + 0] = p.J00 * dM0;
            dV[3 * k + 1] = p.J11 * dM1;
            dV[3 * k + 2] = p.J02 * dM0 + p.J12 * dM1;
        }
        // ---- camera-space mean t = (m, 1) V: through J (a clamped x/z, y/z is a constant) and the depth image
        float tz2 = 1.f / (p.tz * p.tz), tz3 = tz2 / p.tz;
        float dt[3];
        dt[0] = p.clx ? 0.f : -fx * tz2 * dJ02;
        dt[1] = p.cly ? 0.f : -fy * tz2 * dJ12;
        dt[2] = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + 2.f * fx * p.cx * tz3 * dJ02 + 2.f * fy * p.cy * tz3 * dJ12;
        dt[2] += g_depth;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int k = 0; k < 3; k++) dV[3 * k + r] += m[k] * dt[r];
            dV[9 + r] = dt[r];
        }
        // ---- pixel mean: (hx, hy, hw) = (m, 1) P, ndc = (hx, hy) / (hw + 1e-7)
        float gxn = 0.5f * (float)W * g0.x, gyn = 0.5f * (float)H * g0.y;
        float hx = ((P[0] * m[0] + P[4] * m[1]) + P[8] * m[2]) + P[12];
        float hy = ((P[1] * m[0] + P[5] * m[1]) + P[9] * m[2]) + P[13];
        float hw = ((P[3] * m[0] + P[7] * m[1]) + P[11] * m[2]) + P[15];
        float pw = 1.f / (hw + 0.0000001f);
        float mul1 = hx * pw * pw, mul2 = hy * pw * pw;
        const float dh[3] = {pw * gxn, pw * gyn, -(mul1 * gxn + mul2 * gyn)};
#pragma unroll
        for (int j = 0; j < 3; j++) {
#pragma unroll
            for (int k = 0; k < 3; k++) dP[3 * k + j] = m[k] * dh[j];
            dP[9 + j] = dh[j];
        }
    }
    // wave sums (valid in lane 63), then the four waves through LDS
    const uint32_t wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < CAM_LIVE; k++) {
        const float v = wave_reduce_to_lane63(acc[k]);
        if ((threadIdx.x & 63) == 63) s_part[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < CAM_ROW / 4) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int slot = cam_slot(4 * (int)threadIdx.x + j);
            float v = 0.f;
            if (slot >= 0) {
                v = s_part[0][slot];
#pragma unroll
                for (int w = 1; w < CAM_WAVES; w++) v = v + s_part[w][slot];
            }
            o[j] = v;
        }
        reinterpret_cast<float4*>(partials + (size_t)blockIdx.x * CAM_ROW)[threadIdx.x] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// One workgroup.  The rows are contiguous, so thread t of the first 28 * 36 walks element t % 36 of the rows t / 36, t / 36 + 28, ... in
// ascending order (coalesced: the whole workgroup reads 1008 consecutive floats per step) and adds them in fp64; the 28 partial sums of an
// output then meet in LDS and are added in ascending order.  The order is a function of the row count alone.
#define CAMR_GROUPS 28
#define CAMR_THREADS (CAMR_GROUPS * CAM_ROW)
__global__ void __launch_bounds__(1024) k_camera_reduce(const float* __restrict__ partials, int rows, float* __restrict__ out) {
    __shared__ double s_sum[CAMR_THREADS];
    const int t = threadIdx.x;
    const size_t total = (size_t)rows * CAM_ROW;
    if (t < CAMR_THREADS) {
        double s = 0.0;
        for (size_t k = (size_t)t; k < total; k += CAMR_THREADS) s += (double)partials[k];
        s_sum[t] = s;
    }
    __syncthreads();
    if (t < CAM_OUT) {
        double s = s_sum[t];
        for (int g = 1; g < CAMR_GROUPS; g++) s += s_sum[g * CAM_ROW + t];
        out[t] = (float)s;
    }
}

}  // namespace

size_t emd_camera_grad_rows(int N) { return N > 0 ? ((size_t)N + CAM_BLOCK - 1) / CAM_BLOCK : 0; }
size_t emd_camera_grad_bytes(int N) {
    const size_t rows = emd_camera_grad_rows(N);
    return (rows > 0 ? rows : 1) * CAM_ROW * sizeof(float);
}

int emd_launch_camera_backward(const PreBwdArgs& a, float* partials, float* dL_dcamera, hipStream_t st) {
    const int rows = (int)emd_camera_grad_rows(a.N);
    if (rows > 0) {
        hipLaunchKernelGGL(k_camera_backward, dim3(rows), dim3(CAM_BLOCK), 0, st, a, partials);
        EMD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_camera_reduce, dim3(1), dim3(1024), 0, st, partials, rows, dL_dcamera);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}
