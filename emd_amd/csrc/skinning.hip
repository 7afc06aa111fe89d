// skinning.hip -- linear-blend skinning of SMPL pedestrian nodes: the 24-joint kinematic chain and the per-point
// blend / transform / quaternion composition, forward and backward, two launches each way.  gfx950.
//
// Built with the flags of standalone_ops.hip (-ffp-contract=off -fno-slp-vectorize): it shares gaussian_math.h, and every sum here is an
// individually rounded fp32 operation in the order written, so the gradients are a fixed function of the call's inputs.  No kernel of this unit
// uses an atomic: the per-instance sums dL/dA and dL/dtrans leave k_skin_backward as one partial slab per chunk of at most 256 points, added
// in ascending point order, and k_joint_chain_backward adds an instance's slabs in ascending chunk order.
//
// Reference behaviour this replaces (file:line, restated as formulas in include/emd_raster.h and tests/skinning_ref.py):
//   joint chain      OmniRe/models/human_body.py:158-181   (SMPLTemplate.forward: a Python loop over 24 joints of 4x4 products)
//   skinning         OmniRe/models/nodes/smpl.py:438-532   (transform_means_and_quats: [N,24] x [N,24,16] blend, bmm, matrix_to_quaternion,
//                                                           quat_mult, quat_act)
#include "common.h"
#include "device_utils.h"
#include "gaussian_math.h"

#pragma clang fp contract(off)

#define SKIN_J EMD_SKIN_JOINTS
#define SKIN_TAB (SKIN_J * 12)                  // floats of one instance's table of skinning matrices
#define SKIN_CHUNK EMD_SKIN_CHUNK
#define SKIN_PART EMD_SKIN_PARTIAL_FLOATS       // 288 sums of dL/dA + 3 of dL/dtrans
#define SKIN_BWD_THREADS 320                    // 256 point lanes; the first 291 threads own one sum of the slab each
#define SKIN_PITCH 260                          // floats between the staged columns: 16-byte aligned rows that start 4 banks apart

namespace {

// ---------------------------------------------------------------------------------------------------
// Joint chain.  One wave per instance, lane j < 24 owns joint j.  3x4 transforms are kept as G[0..8] = R row-major, G[9..11] = t inside
// the chain kernels; A and canon_inv are row-major 3x4 ([r00 r01 r02 t0 | r10 ...]) in memory.
// ---------------------------------------------------------------------------------------------------
struct ChainLane {
    float qu[4], n;      // theta_j / |theta_j| and |theta_j|
    float R[9];          // R(theta_j)
    float tl[3];         // joints_j - joints_parent (the root: joints_0)
    float J[3];          // joints_j
    int par;             // parents[j] held to [-1, j - 1]: any table is memory-safe
};

// Leaves G_j of every joint in sG (and lane j's own in G).  A joint reads only its finished parent: step s of the walk finishes joint s,
// and parents[s] < s.  Every lane of the wave reaches every barrier.
__device__ __forceinline__ void chain_walk(const EmdJointChainArgs& a, int p, int j, float (*sG)[12], ChainLane& c, float G[12]) {
    c.par = -1;
    if (j < SKIN_J) {
        const float4 q = *(const float4*)(a.theta + ((size_t)p * SKIN_J + j) * 4);
        const float qv[4] = {q.x, q.y, q.z, q.w};
        c.n = fmaxf(quat_norm(qv), 1e-12f);
#pragma unroll
        for (int k = 0; k < 4; k++) c.qu[k] = qv[k] / c.n;
        quat_to_R(c.qu, c.R);
        const float* Jp = a.joints + ((size_t)p * SKIN_J + j) * 3;
        c.J[0] = Jp[0]; c.J[1] = Jp[1]; c.J[2] = Jp[2];
        int par = j > 0 ? a.parents[j] : -1;
        par = par < j - 1 ? par : j - 1;
        par = par > -1 ? par : -1;
        c.par = par;
        c.tl[0] = c.J[0]; c.tl[1] = c.J[1]; c.tl[2] = c.J[2];
        if (par >= 0) {
            const float* Jq = a.joints + ((size_t)p * SKIN_J + par) * 3;
            c.tl[0] -= Jq[0]; c.tl[1] -= Jq[1]; c.tl[2] -= Jq[2];
        }
#pragma unroll
        for (int k = 0; k < 9; k++) G[k] = c.R[k];
        G[9] = c.tl[0]; G[10] = c.tl[1]; G[11] = c.tl[2];
#pragma unroll
        for (int k = 0; k < 12; k++) sG[j][k] = G[k];
    }
    __syncthreads();
    for (int s = 1; s < SKIN_J; s++) {
        if (j == s && c.par >= 0) {              // G_s = G_parent . L_s
            float Gp[12];
#pragma unroll
            for (int k = 0; k < 12; k++) Gp[k] = sG[c.par][k];
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int k = 0; k < 3; k++) G[3 * r + k] = (Gp[3 * r] * c.R[k] + Gp[3 * r + 1] * c.R[3 + k]) + Gp[3 * r + 2] * c.R[6 + k];
                G[9 + r] = ((Gp[3 * r] * c.tl[0] + Gp[3 * r + 1] * c.tl[1]) + Gp[3 * r + 2] * c.tl[2]) + Gp[9 + r];
            }
#pragma unroll
            for (int k = 0; k < 12; k++) sG[s][k] = G[k];
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64) k_joint_chain_forward(EmdJointChainArgs a) {
    __shared__ float sG[SKIN_J][12];
    const int p = blockIdx.x, j = threadIdx.x;
    ChainLane c;
    float G[12];
    chain_walk(a, p, j, sG, c, G);
    if (j >= SKIN_J) return;
    float A[12];                                 // A_j = [G.R | G.t - G.R joints_j]
#pragma unroll
    for (int r = 0; r < 3; r++) {
        A[4 * r] = G[3 * r]; A[4 * r + 1] = G[3 * r + 1]; A[4 * r + 2] = G[3 * r + 2];
        A[4 * r + 3] = G[9 + r] - ((G[3 * r] * c.J[0] + G[3 * r + 1] * c.J[1]) + G[3 * r + 2] * c.J[2]);
    }
    float4* out = (float4*)(a.A + ((size_t)p * SKIN_J + j) * 12);
    if (a.canon_inv) {                           // A_j o canon_inv_j
        const float4* Cp = (const float4*)(a.canon_inv + ((size_t)p * SKIN_J + j) * 12);
        const float4 c0 = Cp[0], c1 = Cp[1], c2 = Cp[2];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float x = A[4 * r], y = A[4 * r + 1], z = A[4 * r + 2];
            out[r] = make_float4((x * c0.x + y * c1.x) + z * c2.x, (x * c0.y + y * c1.y) + z * c2.y, (x * c0.z + y * c1.z) + z * c2.z,
                                 ((x * c0.w + y * c1.w) + z * c2.w) + A[4 * r + 3]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 3; r++) out[r] = make_float4(A[4 * r], A[4 * r + 1], A[4 * r + 2], A[4 * r + 3]);
    }
}

// dL/dA of instance p comes either dense (g_A) or as the chunk slabs of k_skin_backward, which are added here in ascending chunk order (and then
// written to dA_out / d_trans when those are asked for).  d_theta == NULL: that sum is all the call does.  Then the chain in reverse: joint s adds
// into its parent for s = 23 .. 1, one joint per step, so a parent receives its children in descending joint index.
__global__ void __launch_bounds__(64) k_joint_chain_backward(EmdJointChainArgs a, const float* __restrict__ g_A, const float* __restrict__ partials,
                                                             const int32_t* __restrict__ chunk_start, float* __restrict__ dA_out,
                                                             float* __restrict__ d_trans, float* __restrict__ d_theta) {
    __shared__ float sG[SKIN_J][12];
    __shared__ float sdG[SKIN_J][12];
    __shared__ float sdA[5 * 64];
    const int p = blockIdx.x, lane = threadIdx.x;
    if (partials) {
        const int c0 = chunk_start[p], c1 = chunk_start[p + 1];
        float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        // eight slabs' loads in flight at a time (the loop is latency-bound otherwise: 20 us for 40 chunks); the adds keep ascending chunk order
        for (int c = c0; c < c1; c += 8) {
            float v[8][5];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const float* row = partials + (size_t)(c + u) * SKIN_PART;
#pragma unroll
                for (int r = 0; r < 5; r++) {
                    const int i = lane + 64 * r;
                    v[u][r] = (c + u < c1 && i < SKIN_PART) ? row[i] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (c + u < c1) {
#pragma unroll
                    for (int r = 0; r < 5; r++) acc[r] = acc[r] + v[u][r];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const int i = lane + 64 * r;
            sdA[i] = acc[r];
            if (i < SKIN_TAB) { if (dA_out) dA_out[(size_t)p * SKIN_TAB + i] = acc[r]; }
            else if (i < SKIN_PART) { if (d_trans) d_trans[(size_t)p * 3 + (i - SKIN_TAB)] = acc[r]; }
        }
    } else {
#pragma unroll
        for (int r = 0; r < 5; r++) {
            const int i = lane + 64 * r;
            sdA[i] = i < SKIN_TAB ? g_A[(size_t)p * SKIN_TAB + i] : 0.f;
        }
    }
    if (!d_theta) return;
    __syncthreads();
    ChainLane c;
    float G[12];
    chain_walk(a, p, lane, sG, c, G);
    if (lane < SKIN_J) {
        float dA[12], dR[9], dt[3];
#pragma unroll
        for (int k = 0; k < 12; k++) dA[k] = sdA[lane * 12 + k];
        if (a.canon_inv) {                       // A' = A o C:  dA.R = dA'.R C.R^T + dA'.t (x) C.t,  dA.t = dA'.t
            const float* Cp = a.canon_inv + ((size_t)p * SKIN_J + lane) * 12;
            float Cv[12];
#pragma unroll
            for (int k = 0; k < 12; k++) Cv[k] = Cp[k];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int k = 0; k < 3; k++)
                    dR[3 * r + k] = ((dA[4 * r] * Cv[4 * k] + dA[4 * r + 1] * Cv[4 * k + 1]) + dA[4 * r + 2] * Cv[4 * k + 2]) + dA[4 * r + 3] * Cv[4 * k + 3];
        } else {
#pragma unroll
            for (int r = 0; r < 3; r++) { dR[3 * r] = dA[4 * r]; dR[3 * r + 1] = dA[4 * r + 1]; dR[3 * r + 2] = dA[4 * r + 2]; }
        }
        dt[0] = dA[3]; dt[1] = dA[7]; dt[2] = dA[11];
#pragma unroll
        for (int r = 0; r < 3; r++) {            // A.R = G.R, A.t = G.t - G.R joints_j
#pragma unroll
            for (int k = 0; k < 3; k++) sdG[lane][3 * r + k] = dR[3 * r + k] - dt[r] * c.J[k];
            sdG[lane][9 + r] = dt[r];
        }
    }
    __syncthreads();
    for (int s = SKIN_J - 1; s >= 1; s--) {
        if (lane == s && c.par >= 0) {           // G_s = G_p L_s:  dG_p.R += dG_s.R R_s^T + dG_s.t (x) tl_s,  dG_p.t += dG_s.t
            float g[12];
#pragma unroll
            for (int k = 0; k < 12; k++) g[k] = sdG[s][k];
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float add = ((g[3 * r] * c.R[3 * k] + g[3 * r + 1] * c.R[3 * k + 1]) + g[3 * r + 2] * c.R[3 * k + 2]) + g[9 + r] * c.tl[k];
                    sdG[c.par][3 * r + k] = sdG[c.par][3 * r + k] + add;
                }
                sdG[c.par][9 + r] = sdG[c.par][9 + r] + g[9 + r];
            }
        }
        __syncthreads();
    }
    if (lane < SKIN_J) {
        float g[9], dRl[9];
#pragma unroll
        for (int k = 0; k < 9; k++) g[k] = sdG[lane][k];
        if (c.par >= 0) {                        // dL_j.R = G_p.R^T dG_j.R
            float Gp[9];
#pragma unroll
            for (int k = 0; k < 9; k++) Gp[k] = sG[c.par][k];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int k = 0; k < 3; k++) dRl[3 * r + k] = (Gp[r] * g[k] + Gp[3 + r] * g[3 + k]) + Gp[6 + r] * g[6 + k];
        } else {
#pragma unroll
            for (int k = 0; k < 9; k++) dRl[k] = g[k];
        }
        float dq[4], out[4];
        dR_to_dq(c.qu, dRl, dq);
        dnormalize4(c.qu, c.n, dq, out);
        *(float4*)(d_theta + ((size_t)p * SKIN_J + lane) * 4) = make_float4(out[0], out[1], out[2], out[3]);
    }
}

// ---------------------------------------------------------------------------------------------------
// Skinning, one point per lane.
// ---------------------------------------------------------------------------------------------------
// T = sum_j w_j A_j over ascending j (At: the instance's table, in LDS or in global memory: inlined per call site)
__device__ __forceinline__ void skin_blend(const float w[SKIN_J], const float* __restrict__ At, float T[12]) {
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = 0.f;
#pragma unroll
    for (int j = 0; j < SKIN_J; j++) {
        const float4* r = (const float4*)(At + 12 * j);
        const float4 a0 = r[0], a1 = r[1], a2 = r[2];
        T[0] = T[0] + w[j] * a0.x; T[1] = T[1] + w[j] * a0.y; T[2] = T[2] + w[j] * a0.z; T[3] = T[3] + w[j] * a0.w;
        T[4] = T[4] + w[j] * a1.x; T[5] = T[5] + w[j] * a1.y; T[6] = T[6] + w[j] * a1.z; T[7] = T[7] + w[j] * a1.w;
        T[8] = T[8] + w[j] * a2.x; T[9] = T[9] + w[j] * a2.y; T[10] = T[10] + w[j] * a2.z; T[11] = T[11] + w[j] * a2.w;
    }
}

__device__ __forceinline__ void load_weights(const float* __restrict__ weights, int i, float w[SKIN_J]) {
    const float4* wp = (const float4*)(weights + (size_t)i * SKIN_J);
#pragma unroll
    for (int v = 0; v < SKIN_J / 4; v++) {
        const float4 t = wp[v];
        w[4 * v] = t.x; w[4 * v + 1] = t.y; w[4 * v + 2] = t.z; w[4 * v + 3] = t.w;
    }
}

// What the quaternion half of a skinned point keeps between its steps (the backward recomputes it).
struct SkinQuat {
    int k;               // branch of matrix_to_quaternion: index of the largest q_abs, the lowest on a tie
    float s, den;        // q_abs_k and the divisor 2 max(q_abs_k, 0.1)
    float qm[4];         // m2q(T.R): row k of the candidate matrix / den (not unit length)
    float qn[4], n;      // quat_act(quat) and |quat|
    float n2;            // |qm (x) qn|
    float wq[4];
};

// pytorch3d's matrix_to_quaternion on the blended 3x3 block of T, then world_quat = quat_act(quat_mult(m2q, quat_act(quat))).  The candidate rows
// are the rows of one symmetric 4x4 matrix: diagonal q_abs^2, off-diagonal ax = m21 - m12, ay = m02 - m20, az = m10 - m01 in row / column 0 and
// sxy = m10 + m01, sxz = m02 + m20, syz = m12 + m21 between x, y, z.  Only the chosen row is evaluated.
__device__ __forceinline__ void skin_quat(const float T[12], const float4 qraw, SkinQuat& o) {
    const float m00 = T[0], m11 = T[5], m22 = T[10];
    const float r0 = ((1.f + m00) + m11) + m22, r1 = ((1.f + m00) - m11) - m22, r2 = ((1.f - m00) + m11) - m22, r3 = ((1.f - m00) - m11) + m22;
    const float a0 = sqrtf(fmaxf(0.f, r0)), a1 = sqrtf(fmaxf(0.f, r1)), a2 = sqrtf(fmaxf(0.f, r2)), a3 = sqrtf(fmaxf(0.f, r3));
    int k = 0;
    float s = a0;
    if (a1 > s) { k = 1; s = a1; }
    if (a2 > s) { k = 2; s = a2; }
    if (a3 > s) { k = 3; s = a3; }
    const float ax = T[9] - T[6], ay = T[2] - T[8], az = T[4] - T[1];
    const float sxy = T[4] + T[1], sxz = T[2] + T[8], syz = T[6] + T[9];
    const float d = s * s;
    float row[4];
    row[0] = k == 0 ? d : (k == 1 ? ax : (k == 2 ? ay : az));
    row[1] = k == 0 ? ax : (k == 1 ? d : (k == 2 ? sxy : sxz));
    row[2] = k == 0 ? ay : (k == 1 ? sxy : (k == 2 ? d : syz));
    row[3] = k == 0 ? az : (k == 1 ? sxz : (k == 2 ? syz : d));
    o.k = k; o.s = s; o.den = 2.f * fmaxf(s, 0.1f);
#pragma unroll
    for (int c = 0; c < 4; c++) o.qm[c] = row[c] / o.den;
    const float ql[4] = {qraw.x, qraw.y, qraw.z, qraw.w};
    o.n = fmaxf(quat_norm(ql), 1e-12f);
#pragma unroll
    for (int c = 0; c < 4; c++) o.qn[c] = ql[c] / o.n;
    float pp[4];
    quat_mul(o.qm, o.qn, pp);
    o.n2 = fmaxf(quat_norm(pp), 1e-12f);
#pragma unroll
    for (int c = 0; c < 4; c++) o.wq[c] = pp[c] / o.n2;
}

__global__ void __launch_bounds__(EMD_BLOCK) k_skin_forward(EmdSkinArgs a) {
    __shared__ __attribute__((aligned(16))) float sA[SKIN_TAB];
    __shared__ int s_first[EMD_BLOCK / 64];
    const int t = threadIdx.x, i = blockIdx.x * EMD_BLOCK + t;
    int p = -1;
    if (i < a.num_points) { p = a.ids[i]; if (p >= a.num_instances) p = -1; }
    // the instance's 24 x 12 table goes through LDS when every bound point of the workgroup belongs to one instance, else through L2
    const unsigned long long has = __ballot(p >= 0);
    const int first_lane = has ? __ffsll((long long)has) - 1 : 0;
    const int first = has ? __builtin_amdgcn_readlane(p, first_lane) : -1;
    if ((t & 63) == 0) s_first[t >> 6] = first;
    __syncthreads();
    int p0 = s_first[0];
#pragma unroll
    for (int w = 1; w < EMD_BLOCK / 64; w++) p0 = p0 >= 0 ? p0 : s_first[w];
    const bool shared = __syncthreads_and(p < 0 || p == p0) && p0 >= 0;
    if (shared) for (int k = t; k < SKIN_TAB; k += EMD_BLOCK) sA[k] = a.A[(size_t)p0 * SKIN_TAB + k];
    __syncthreads();
    if (i >= a.num_points) return;
    const float m[3] = {a.means[3 * i], a.means[3 * i + 1], a.means[3 * i + 2]};
    const float4 q = *(const float4*)(a.quats + 4 * i);
    const float op = a.opacities[i];
    if (p < 0) {                                 // as transform_gaussians leaves a static point: unchanged
        a.world_means[3 * i] = m[0]; a.world_means[3 * i + 1] = m[1]; a.world_means[3 * i + 2] = m[2];
        *(float4*)(a.world_quats + 4 * i) = q;
        a.opacities_out[i] = op;
        return;
    }
    float w[SKIN_J], T[12];
    load_weights(a.weights, i, w);
    if (shared) skin_blend(w, sA, T);
    else skin_blend(w, a.A + (size_t)p * SKIN_TAB, T);
    const float* tr = a.trans + 3 * p;
    a.world_means[3 * i] = (((T[0] * m[0] + T[1] * m[1]) + T[2] * m[2]) + T[3]) + tr[0];
    a.world_means[3 * i + 1] = (((T[4] * m[0] + T[5] * m[1]) + T[6] * m[2]) + T[7]) + tr[1];
    a.world_means[3 * i + 2] = (((T[8] * m[0] + T[9] * m[1]) + T[10] * m[2]) + T[11]) + tr[2];
    SkinQuat sq;
    skin_quat(T, q, sq);
    *(float4*)(a.world_quats + 4 * i) = make_float4(sq.wq[0], sq.wq[1], sq.wq[2], sq.wq[3]);
    a.opacities_out[i] = op * (a.valid ? a.valid[p] : 1.f);
}

// One workgroup per chunk: at most 256 points of ONE instance (or of none: instance < 0, pass-through gradients), listed by the chunk table
// through `order`.  Threads 0 .. 255 are the point lanes: per-point gradients are stored directly, the point's weights and its dL/dT row are staged
// in LDS column by column.  Then thread (j, k) = t < 288 adds w[pt][j] * gT[pt][k] over the chunk's points in ascending position, threads
// 288 .. 290 add the translation part of gT (= dL/dtrans), and each stores its sum into the chunk's slab.  Padding columns hold zeros.
__global__ void __launch_bounds__(SKIN_BWD_THREADS) k_skin_backward(EmdSkinArgs a, EmdSkinGrads g) {
    __shared__ __attribute__((aligned(16))) float sA[SKIN_TAB];
    __shared__ __attribute__((aligned(16))) float sW[SKIN_J * SKIN_PITCH];
    __shared__ __attribute__((aligned(16))) float sG[12 * SKIN_PITCH];
    const int c = blockIdx.x, t = threadIdx.x;
    const int p = a.chunks[3 * c], first = a.chunks[3 * c + 1], cnt = a.chunks[3 * c + 2];
    // a table that does not describe this call's points is not followed out of bounds
    if (p >= a.num_instances || cnt < 0 || cnt > SKIN_CHUNK || first < 0 || first > a.num_points - cnt) return;
    if (p >= 0 && t < SKIN_TAB) sA[t] = a.A[(size_t)p * SKIN_TAB + t];
    __syncthreads();
    if (t < SKIN_CHUNK) {
        int i = -1;
        if (t < cnt) {
            i = a.order ? a.order[first + t] : first + t;
            if (i < 0 || i >= a.num_points) i = -1;
        }
        float gT[12], w[SKIN_J];
#pragma unroll
        for (int k = 0; k < 12; k++) gT[k] = 0.f;
#pragma unroll
        for (int j = 0; j < SKIN_J; j++) w[j] = 0.f;
        if (i >= 0) {
            const float gm[3] = {g.g_world_means[3 * i], g.g_world_means[3 * i + 1], g.g_world_means[3 * i + 2]};
            const float4 gq4 = *(const float4*)(g.g_world_quats + 4 * i);
            const float go = g.g_opacities_out[i];
            if (p < 0) {
                g.d_means[3 * i] = gm[0]; g.d_means[3 * i + 1] = gm[1]; g.d_means[3 * i + 2] = gm[2];
                *(float4*)(g.d_quats + 4 * i) = gq4;
                g.d_opacities[i] = go;
                if (g.d_weights) {
                    float4* dw = (float4*)(g.d_weights + (size_t)i * SKIN_J);
#pragma unroll
                    for (int v = 0; v < SKIN_J / 4; v++) dw[v] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            } else {
                const float m[3] = {a.means[3 * i], a.means[3 * i + 1], a.means[3 * i + 2]};
                const float4 q = *(const float4*)(a.quats + 4 * i);
                float T[12];
                load_weights(a.weights, i, w);
                skin_blend(w, sA, T);
                // world_mean = T.R m + T.t + trans
#pragma unroll
                for (int r = 0; r < 3; r++) {
                    gT[4 * r] = gm[r] * m[0]; gT[4 * r + 1] = gm[r] * m[1]; gT[4 * r + 2] = gm[r] * m[2]; gT[4 * r + 3] = gm[r];
                }
#pragma unroll
                for (int k = 0; k < 3; k++) g.d_means[3 * i + k] = (T[k] * gm[0] + T[4 + k] * gm[1]) + T[8 + k] * gm[2];
                g.d_opacities[i] = go * (a.valid ? a.valid[p] : 1.f);
                // world_quat = normalize(qm (x) qn)
                SkinQuat sq;
                skin_quat(T, q, sq);
                const float gq[4] = {gq4.x, gq4.y, gq4.z, gq4.w};
                float dp[4], dqm[4], dqn[4], dql[4];
                dnormalize4(sq.wq, sq.n2, gq, dp);
                const float bc[4] = {sq.qn[0], -sq.qn[1], -sq.qn[2], -sq.qn[3]}, ac[4] = {sq.qm[0], -sq.qm[1], -sq.qm[2], -sq.qm[3]};
                quat_mul(dp, bc, dqm);
                quat_mul(ac, dp, dqn);
                dnormalize4(sq.qn, sq.n, dqn, dql);
                *(float4*)(g.d_quats + 4 * i) = make_float4(dql[0], dql[1], dql[2], dql[3]);
                // qm = row_k / (2 s), row_k[k] = s^2, s = sqrt(radicand_k) >= 1 (the four radicands sum to 4): d qm_k / d s = 1/2,
                // d qm_c / d s = -qm_c / s for c != k, d qm_c / d row_c = 1 / (2 s)
                const int k = sq.k;
                float e[4], dot = 0.f;
#pragma unroll
                for (int cc = 0; cc < 4; cc++) {
                    e[cc] = cc == k ? 0.f : dqm[cc] / sq.den;
                    dot = dot + (cc == k ? 0.f : dqm[cc] * sq.qm[cc]);
                }
                const float dqk = k == 0 ? dqm[0] : (k == 1 ? dqm[1] : (k == 2 ? dqm[2] : dqm[3]));
                const float ds = 0.5f * dqk - dot / sq.s;
                const float drad = ds / (2.f * sq.s);
                gT[0] = gT[0] + ((k == 0 || k == 1) ? drad : -drad);
                gT[5] = gT[5] + ((k == 0 || k == 2) ? drad : -drad);
                gT[10] = gT[10] + ((k == 0 || k == 3) ? drad : -drad);
                const float g_ax = k == 0 ? e[1] : (k == 1 ? e[0] : 0.f), g_ay = k == 0 ? e[2] : (k == 2 ? e[0] : 0.f);
                const float g_az = k == 0 ? e[3] : (k == 3 ? e[0] : 0.f), g_sxy = k == 1 ? e[2] : (k == 2 ? e[1] : 0.f);
                const float g_sxz = k == 1 ? e[3] : (k == 3 ? e[1] : 0.f), g_syz = k == 2 ? e[3] : (k == 3 ? e[2] : 0.f);
                gT[9] = gT[9] + (g_syz + g_ax); gT[6] = gT[6] + (g_syz - g_ax);
                gT[2] = gT[2] + (g_sxz + g_ay); gT[8] = gT[8] + (g_sxz - g_ay);
                gT[4] = gT[4] + (g_sxy + g_az); gT[1] = gT[1] + (g_sxy - g_az);
                if (g.d_weights) {               // dL/dw_j = gT . A_j
                    float4* dw = (float4*)(g.d_weights + (size_t)i * SKIN_J);
#pragma unroll
                    for (int v = 0; v < SKIN_J / 4; v++) {
                        float o4[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            const float* Aj = sA + 12 * (4 * v + u);
                            float acc = 0.f;
#pragma unroll
                            for (int kk = 0; kk < 12; kk++) acc = acc + gT[kk] * Aj[kk];
                            o4[u] = acc;
                        }
                        dw[v] = make_float4(o4[0], o4[1], o4[2], o4[3]);
                    }
                }
            }
        }
        if (p >= 0) {
#pragma unroll
            for (int j = 0; j < SKIN_J; j++) sW[j * SKIN_PITCH + t] = w[j];
#pragma unroll
            for (int k = 0; k < 12; k++) sG[k * SKIN_PITCH + t] = gT[k];
        }
    }
    if (p < 0) return;
    __syncthreads();
    if (t >= SKIN_PART) return;
    const bool outer = t < SKIN_TAB;
    const float4* wr = (const float4*)(sW + (outer ? t / 12 : 0) * SKIN_PITCH);
    const float4* gr = (const float4*)(sG + (outer ? t % 12 : 3 + 4 * (t - SKIN_TAB)) * SKIN_PITCH);
    const int n4 = (cnt + 3) >> 2;
    float acc = 0.f;
    if (outer) {
        for (int v = 0; v < n4; v++) {
            const float4 wv = wr[v], gv = gr[v];
            acc = acc + wv.x * gv.x; acc = acc + wv.y * gv.y; acc = acc + wv.z * gv.z; acc = acc + wv.w * gv.w;
        }
    } else {
        for (int v = 0; v < n4; v++) {
            const float4 gv = gr[v];
            acc = acc + gv.x; acc = acc + gv.y; acc = acc + gv.z; acc = acc + gv.w;
        }
    }
    g.partials[(size_t)c * SKIN_PART + t] = acc;
}

bool chain_args_ok(const EmdJointChainArgs* a, const char* what) {
    if (!a) { emd_set_error("%s: null argument struct", what); return false; }
    if (a->num_instances <= 0) { emd_set_error("%s: num_instances = %d (must be > 0)", what, a->num_instances); return false; }
    if (!a->theta || !a->joints || !a->parents) { emd_set_error("%s: null theta, joints or parents", what); return false; }
    return true;
}

bool skin_args_ok(const EmdSkinArgs* a, bool backward, const char* what) {
    if (!a) { emd_set_error("%s: null argument struct", what); return false; }
    if (a->num_points < 0) { emd_set_error("%s: num_points = %d (must be >= 0)", what, a->num_points); return false; }
    if (a->num_instances <= 0) { emd_set_error("%s: num_instances = %d (must be > 0)", what, a->num_instances); return false; }
    if (!a->means || !a->quats || !a->opacities || !a->ids || !a->weights || !a->A || !a->trans) {
        emd_set_error("%s: null means, quats, opacities, ids, weights, A or trans", what);
        return false;
    }
    if (backward || a->chunks) {
        // every instance (and the unbound points) ends in at most one short chunk: ceil(N / 256) <= chunks <= N / 256 + P + 1
        const int64_t lo = ((int64_t)a->num_points + SKIN_CHUNK - 1) / SKIN_CHUNK, hi = (int64_t)a->num_points / SKIN_CHUNK + a->num_instances + 1;
        if (a->num_chunks < lo || a->num_chunks > hi || (a->num_chunks > 0 && !a->chunks)) {
            emd_set_error("%s: chunk table inconsistent with num_points: %d chunks for %d points of %d instances (%lld .. %lld)", what, a->num_chunks,
                          a->num_points, a->num_instances, (long long)lo, (long long)hi);
            return false;
        }
    }
    return true;
}

}  // namespace

extern "C" int emd_joint_chain_forward(const EmdJointChainArgs* a, void* hip_stream) {
    if (!chain_args_ok(a, "joint_chain_forward")) return EMD_ERR_INVALID;
    if (!a->A) { emd_set_error("joint_chain_forward: null A"); return EMD_ERR_INVALID; }
    hipLaunchKernelGGL(k_joint_chain_forward, dim3(a->num_instances), dim3(64), 0, (hipStream_t)hip_stream, *a);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_joint_chain_backward(const EmdJointChainArgs* a, const float* dL_dA, const float* partials, const int32_t* instance_chunk_start,
                                        float* dL_dA_out, float* dL_dtrans, float* dL_dtheta, void* hip_stream) {
    if (!a) { emd_set_error("joint_chain_backward: null argument struct"); return EMD_ERR_INVALID; }
    if (dL_dtheta && !chain_args_ok(a, "joint_chain_backward")) return EMD_ERR_INVALID;
    if (a->num_instances <= 0) { emd_set_error("joint_chain_backward: num_instances = %d (must be > 0)", a->num_instances); return EMD_ERR_INVALID; }
    if ((dL_dA != nullptr) == (partials != nullptr)) { emd_set_error("joint_chain_backward: exactly one of dL_dA and partials"); return EMD_ERR_INVALID; }
    if (partials && !instance_chunk_start) { emd_set_error("joint_chain_backward: partials without instance_chunk_start (null)"); return EMD_ERR_INVALID; }
    if (!dL_dtheta && !(partials && (dL_dA_out || dL_dtrans))) { emd_set_error("joint_chain_backward: nothing to compute (null outputs)"); return EMD_ERR_INVALID; }
    hipLaunchKernelGGL(k_joint_chain_backward, dim3(a->num_instances), dim3(64), 0, (hipStream_t)hip_stream, *a, dL_dA, partials, instance_chunk_start,
                       dL_dA_out, dL_dtrans, dL_dtheta);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_skin_forward(const EmdSkinArgs* a, void* hip_stream) {
    if (!skin_args_ok(a, false, "skin_forward")) return EMD_ERR_INVALID;
    if (!a->world_means || !a->world_quats || !a->opacities_out) { emd_set_error("skin_forward: null output"); return EMD_ERR_INVALID; }
    if (a->num_points == 0) return EMD_OK;
    hipLaunchKernelGGL(k_skin_forward, dim3((a->num_points + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, (hipStream_t)hip_stream, *a);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_skin_backward(const EmdSkinArgs* a, const EmdSkinGrads* g, void* hip_stream) {
    if (!skin_args_ok(a, true, "skin_backward")) return EMD_ERR_INVALID;
    if (!g || !g->g_world_means || !g->g_world_quats || !g->g_opacities_out || !g->d_means || !g->d_quats || !g->d_opacities || !g->partials) {
        emd_set_error("skin_backward: null gradient pointer (only d_weights may be null)");
        return EMD_ERR_INVALID;
    }
    if (a->num_chunks == 0) return EMD_OK;
    hipLaunchKernelGGL(k_skin_backward, dim3(a->num_chunks), dim3(SKIN_BWD_THREADS), 0, (hipStream_t)hip_stream, *a, *g);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}
