// camera_grad.hip -- dL/d(viewmatrix, projmatrix, campos) of one rasterizer call: the opt-in kernel between the two halves of the backward
// (K7 has filled the per-Gaussian accumulator rows, K8 has not consumed them yet).  gfx950, one Gaussian per lane.
//
// Every entry of EmdSettings.viewmatrix / projmatrix / campos that K1 reads is a free variable; the 35 outputs are laid out as the settings
// block is (V[16], P[16], campos[3]); the entries K1 never reads (V[3], V[7], V[11], V[15], the z column of P) get an exact 0.f.  The chain
// rule from these numbers to a camera pose stays with the caller (4x4 tensors).  The per-Gaussian arithmetic is K8's (preprocess.hip),
// term for term and in K8's order, so that both read the same fp32 intermediates: both kernels compile the same source, the functions of
// projection_math.h and the *_body.inc texts it names.  The accumulator rows are READ only (K8 consumes and clears them afterwards).  DESIGN.md, "Camera gradients", lists the terms.
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
#include "projection_math.h"

#pragma clang fp contract(off)

namespace {

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
        // K8's part 1, its text: the loads and the world pose.  The accumulator row is read only and the opacity does not depend on the camera:
        // consume_row = false.  (The three lines of flags are K8's, restated: as a function they moved K8's machine code.)
        const bool motion = (a.flags & EMD_FLAG_MOTION) != 0;
        const bool has_ids = motion && a.motion.actor_id != nullptr, has_rot = a.rotations != nullptr;
        const bool has_rdx = motion && a.motion.residual_dx != nullptr, has_rdq = motion && has_rot && a.motion.residual_dq != nullptr;
        const float4 z4c = make_float4(0.f, 0.f, 0.f, 0.f);
        int a_id;
        float m[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, op = 0.f, q_norm, mloc[3], op_raw;
        float4 q_raw, rdq, pr0 = z4c, pr1 = z4c, pr2 = z4c;
        constexpr bool consume_row = false;
#include "gaussian_pose_body.inc"
        const float* cp = a.cov3D_precomp ? a.cov3D_precomp + 6 * (size_t)i : safe;
        const float c0 = cp[0], c1 = cp[1], c2 = cp[2], c3_ = cp[3], c4 = cp[4], c5 = cp[5];
        const float g_depth = g0.z, gA = g1.x, gB = g1.y, gC = g1.z;
        const float gcol[3] = {g1.w, g2.x, g2.y};
        Proj p;
        view_transform(V, m, p.tx, p.ty, p.tz);
        // ---- SH colour: d colour / d campos = -d colour / d mean
        if (!a.colors_precomp) {
#include "sh_dir_grad_body.inc"
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
        const ProjJac J = project_cov2d(S, c3, fx, fy, p);
#include "conic_bwd_body.inc"
#include "cov2d_bwd_body.inc"
        // ---- camera-space mean t = (m, 1) V
#pragma unroll
        for (int k = 0; k < 3; k++) {
            dV[3 * k + 0] = J.J00 * dM0[k];
            dV[3 * k + 1] = J.J11 * dM1[k];
            dV[3 * k + 2] = J.J02 * dM0[k] + J.J12 * dM1[k];
        }
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int k = 0; k < 3; k++) dV[3 * k + r] += m[k] * dt[r];
            dV[9 + r] = dt[r];
        }
        // ---- pixel mean: (hx, hy, hw) = (m, 1) P, ndc = (hx, hy) / (hw + 1e-7)
        float gxn = 0.5f * (float)W * g0.x, gyn = 0.5f * (float)H * g0.y;
        const Clip h = clip_transform(P, m);
        float mul1 = h.hx * h.pw * h.pw, mul2 = h.hy * h.pw * h.pw;
        const float dh[3] = {h.pw * gxn, h.pw * gyn, -(mul1 * gxn + mul2 * gyn)};
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
