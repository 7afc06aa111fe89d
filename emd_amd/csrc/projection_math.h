// projection_math.h -- the projection chain of one Gaussian, written once for the three kernels that walk it: K1 and K8 (preprocess.hip) and
// the camera-gradient kernel (camera_grad.hip).  Included by those two units only (gaussian_math.h stays what the stand-alone entry points
// share).  Every operation is an individually rounded fp32 op in the order written here ("pinned evaluation order"): the three
// kernels read the same intermediates because they compile the same text.
//
// K8 sits at the 128-VGPR cap and its machine code is pinned (profiles/projection_shared_isa.txt): a piece lives here as a function where K1
// and K8 compile to the same instructions as before.  The blocks of K8 that the camera kernel repeats moved K8 in every function form tried, so they
// are *_body.inc texts beside this header, included inside both kernels: gaussian_pose_body.inc (loads, world pose), sh_dir_grad_body.inc (SH colour
// -> view direction), conic_bwd_body.inc (conic -> cov2D), cov2d_bwd_body.inc (cov2D -> J -> camera-space mean).  Results come back by value: an
// out-parameter of clip_transform was enough to reorder K8's register moves.
#pragma once
#include "gaussian_math.h"

#pragma clang fp contract(off)

// camera-space mean t = (m, 1) V
__device__ __forceinline__ void view_transform(const float* V, const float m[3], float& tx, float& ty, float& tz) {
    tx = ((V[0] * m[0] + V[4] * m[1]) + V[8] * m[2]) + V[12];
    ty = ((V[1] * m[0] + V[5] * m[1]) + V[9] * m[2]) + V[13];
    tz = ((V[2] * m[0] + V[6] * m[1]) + V[10] * m[2]) + V[14];
}

// clip-space mean (hx, hy, hw) = (m, 1) P with pw = 1 / (hw + 1e-7): ndc = (hx, hy) * pw
struct Clip { float hx, hy, pw; };
__device__ __forceinline__ Clip clip_transform(const float* P, const float m[3]) {
    float hx = ((P[0] * m[0] + P[4] * m[1]) + P[8] * m[2]) + P[12];
    float hy = ((P[1] * m[0] + P[5] * m[1]) + P[9] * m[2]) + P[13];
    float hw = ((P[3] * m[0] + P[7] * m[1]) + P[11] * m[2]) + P[15];
    return {hx, hy, 1.f / (hw + 0.0000001f)};
}

// Everything up to cov2D for one visible Gaussian (tx, ty, tz are the caller's: view_transform).
struct Proj {
    float tx, ty, tz, cx, cy;
    bool clx, cly;
    float M0[3], M1[3], T0[3], T1[3];
    float a, b, c, det;
};

// Returns the four non-constant entries of the projection's Jacobian (the camera kernel's dL/dV needs them; K1 and K8 do not look).
struct ProjJac { float J00, J02, J11, J12; };
__device__ __forceinline__ ProjJac project_cov2d(const EmdSettings& S, const float c3[6], float fx, float fy, Proj& p) {
    const float* V = S.viewmatrix;
    float limx = 1.3f * S.tanfovx, limy = 1.3f * S.tanfovy;
    float txtz = p.tx / p.tz, tytz = p.ty / p.tz;
    p.clx = (txtz < -limx) || (txtz > limx);
    p.cly = (tytz < -limy) || (tytz > limy);
    p.cx = fminf(limx, fmaxf(-limx, txtz)) * p.tz;
    p.cy = fminf(limy, fmaxf(-limy, tytz)) * p.tz;
    float J00 = fx / p.tz, J02 = -(fx * p.cx) / (p.tz * p.tz), J11 = fy / p.tz, J12 = -(fy * p.cy) / (p.tz * p.tz);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        p.M0[k] = J00 * V[4 * k + 0] + J02 * V[4 * k + 2];
        p.M1[k] = J11 * V[4 * k + 1] + J12 * V[4 * k + 2];
    }
    const float Sg[9] = {c3[0], c3[1], c3[2], c3[1], c3[3], c3[4], c3[2], c3[4], c3[5]};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        p.T0[k] = (p.M0[0] * Sg[k] + p.M0[1] * Sg[3 + k]) + p.M0[2] * Sg[6 + k];
        p.T1[k] = (p.M1[0] * Sg[k] + p.M1[1] * Sg[3 + k]) + p.M1[2] * Sg[6 + k];
    }
    p.a = ((p.T0[0] * p.M0[0] + p.T0[1] * p.M0[1]) + p.T0[2] * p.M0[2]) + 0.3f;
    p.b = (p.T0[0] * p.M1[0] + p.T0[1] * p.M1[1]) + p.T0[2] * p.M1[2];
    p.c = ((p.T1[0] * p.M1[0] + p.T1[1] * p.M1[1]) + p.T1[2] * p.M1[2]) + 0.3f;
    p.det = p.a * p.c - p.b * p.b;
    return {J00, J02, J11, J12};
}

