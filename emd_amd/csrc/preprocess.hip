// preprocess.hip -- K1 (fused explicit motion + projection + EWA covariance + SH colour) and K8 (its backward), with the two small
// kernels that read K1's records (k_sh_factor, k_export_geometry).  gfx950, one Gaussian per lane.  The per-Gaussian math K1 / K8 share
// with the stand-alone entry points (standalone_ops.hip) is in gaussian_math.h; the projection chain K1, K8 and the camera-gradient kernel
// (camera_grad.hip) walk is in projection_math.h, and the blocks of K8 that kernel repeats are the *_body.inc texts named there.
//
// Built with -ffp-contract=off: the view depth (sort key), radius and tile rectangle are a bit-exact
// contract with oracle/raster_oracle.c, so every operation here is an individually rounded fp32 op in
// the documented order ("pinned evaluation order").
//
// Reference behaviour this replaces (file:line):
//   activations + rasterizer preprocess   S3Gaussian/gaussian_renderer/__init__.py:99-101,145-155 [UPSTREAM K1]
//   cov3D                                 S3Gaussian/utils/general_utils.py:245-277, scene/gaussian_model.py:34-38
//   SH colour                             S3Gaussian/utils/sh_utils.py:57-112, gaussian_renderer/__init__.py:19-25
//   projection                            S3Gaussian/utils/graphics_utils.py:42-49
//   rigid actor motion + residual         OmniRe/models/nodes/rigid.py:478-568, deformable.py:57-69
#include "common.h"
#include "device_utils.h"
#include "gaussian_math.h"
#include "projection_math.h"

#pragma clang fp contract(off)

// Cache policy and traversal order (round 5).  A step moves ~2 GB through a 256 MiB Infinity Cache; what decides the two projection kernels'
// time is which of it is still there when they ask:
//   * streams that are touched once per step bypass the caches: the SH rows K1 reads (192 B per visible Gaussian, nontemporal loads), the
//     dense dL/dshs rows K8 writes (384 MB, nontemporal stores), the colour Jacobian K1 leaves for K8 a whole step's traffic later
//     (nontemporal stores);
//   * K1 walks the Gaussians from the LAST block to the first: the parameters K8 read last, at the end of the step before, are the ones
//     K1 asks for first;
//   * K8 takes the colour clamp bits from the spare word of the Jacobian row it reads anyway instead of fetching a 64-byte record for them.
// Measured together on one box: K1 0.159 -> 0.121 ms, K8 0.229 -> 0.214 ms, 748 -> 782 it/s.
//   * K8 compacts the visible Gaussians of a 256-block onto its first lanes (full waves do the work, the others only write zero rows) and
//     sends the five small gradients through the idle SH tile as whole 16-byte nontemporal stores: K8 0.201 -> 0.193 ms, 799 -> 806 it/s.
//   * K1 and K8 issue every index-addressed load of a Gaussian together, before the first use (round 5, late).
//   * the zero rows of the dense dL/dshs -- three quarters of its 384 MB -- are not K8's any more in the one-call default backward: K7's workgroups
//     zero ALL rows, a slice each, under their pixel loops (render.hip, emd_fill_slice), and K8 (the PZ instantiation) stores the rows of its
//     compacted Gaussians over them, walking the compaction list.  The dense instantiation serves every other call unchanged: the two-call form,
//     EMD_FLAG_DETERMINISTIC, M != 16 (profiles/backward_prefill_ab.txt).
// Tried and not kept: nontemporal loads of the Jacobian in K8 (+10 us there), nontemporal scalar stores of K8's small gradients (+8 us in
// K8 for -5 in K1), nontemporal stores of the projected records (K1 0.11 -> 0.19 ms: 48-byte pieces; and the render kernels do not care
// where the records come from: +2 us), the small-gradient tile without the compaction (-3 us in K1, +4 us in K8).
// Every one of these was a compile-time switch with its A/B recorded in profiles/r05_cache_policy_variants.txt (narrative:
// docs/history/DESIGN_rounds_1-5.md, "change (knob in csrc/preprocess.hip)"); the switches were retired once settled, and the A/B builds
// are reproducible from the last commit that carries them (profiles/README.md).
// (load_f4_nt / store_f4_nt: device_utils.h)

namespace {

__device__ __forceinline__ int tile_clamp(float f, int grid) {
    float g = (float)grid;
    if (!(f > 0.f)) return 0;
    if (f > g) return grid;
    return (int)f;
}

// ---------------------------------------------------------------------------------------------------
// SH rows through LDS.  shs is [N,16,3]: 192 contiguous bytes per Gaussian, so one-Gaussian-per-lane loads/stores
// touch 64 different cache lines per instruction.  Instead the block moves its rows (contiguous in HBM) with fully
// coalesced dwordx4 accesses and each lane reads / writes its own row in LDS -- HALF of the block's rows at a time, so that the
// staging tile (6.5 KB per wave in K1, 26 KB per 256 threads in K8 and the factor rebuild) does not cap the resident waves: with
// whole-block tiles K1 ran 3 waves per SIMD and 0.196 ms, with half tiles 4 and 0.154 ms.  Rows are padded to SH_ROW4 float4
// (gaussian_math.h).
// ---------------------------------------------------------------------------------------------------
// this lane's 48 coefficients [k][c] into registers straight from HBM (the M != 16 path; M == 16 goes through the staging tile)
__device__ __forceinline__ void sh_row_load(const float* __restrict__ shs, const float* __restrict__ r0, const float* __restrict__ r1, int i, int M,
                                            int K, float v[48]) {
    const size_t o = (size_t)i * M * 3;
#pragma unroll
    for (int k = 0; k < 48; k++) {
        float x = (k < 3 * K) ? shs[o + k] : 0.f;
        if (r0 && k < 3 * K) x = x + r0[o + k];          // (shs + r0) + r1, the order of the reference's two adds
        if (r1 && k < 3 * K) x = x + r1[o + k];
        v[k] = x;
    }
}

// ---------------------------------------------------------------------------------------------------
// K1.  One wave per workgroup.  Order of work: (1) geometry of the lane's Gaussian up to the visibility decision, (2) the
// wave stages the 192-byte SH rows of its VISIBLE Gaussians only (coalesced dwordx4 pieces, predicated per row by the
// visibility ballot: a quarter of the bench scene is culled and its coefficients are never read), (3) colour, the
// colour Jacobian and the record stores.  Twelve independent 13 KB workgroups per CU overlap these phases.
// ---------------------------------------------------------------------------------------------------
#define PRE_BLOCK 64
#define EMD_K1_WAVES 4
// PART 0: the whole kernel.  PART 1 / PART 2 (round 3): its geometry half (everything the binning needs, and rows 0, 1, 3 of the record)
// and its colour half (SH colour, clamp bits, colour Jacobian: row 2 of the record and shjac) as two launches -- the colour half is
// needed by K6 only, so with an auxiliary stream (EmdFwdArgs.aux_stream) it runs BESIDE the twenty launch-bound kernels of the binning
// stage instead of in front of them.  PART 2 recomputes the world mean of its Gaussian (one gather for an actor's point) and takes
// the visibility from the radii PART 1 wrote.
// RES: residuals of the SH coefficients are added while the rows are staged (EmdFwdArgs.shs_residual); a separate instantiation, so
// that the usual kernel keeps its registers (with the residual loads in the same code it spilled 24)
template <int PART, bool RES = false>
__global__ void __launch_bounds__(PRE_BLOCK) __attribute__((amdgpu_waves_per_eu(PART == 1 ? 6 : (RES ? 4 : EMD_K1_WAVES)))) k_preprocess(PreArgs a) {
    __shared__ float4 s_sh[PART == 1 ? 1 : (PRE_BLOCK / 2) * SH_ROW4];       // half of the wave's rows at a time: 6.5 KB keeps four waves per SIMD
    EmdSettings S = a.s;
    emd_settings_from_device(S, a.sdev, a.flags);
    const bool sh_staged = a.shs && a.M == 16;
    const uint32_t blk = gridDim.x - 1u - blockIdx.x;       // last block first: what K8 touched last is what K1 reads first
    const int i = blk * PRE_BLOCK + threadIdx.x;
    // the call's four status words are cleared here (the binning kernels behind this launch raise bits in them): no launch of its own
    if (PART != 2 && blockIdx.x == 0 && threadIdx.x < 4 && a.status) reinterpret_cast<uint32_t*>(a.status)[threadIdx.x] = 0u;
    uint32_t touched = 0, rect = 0, rect_h = 0, dkey = 0xFFFFFFFFu, skip = 0;
    int radius_out = 0;
    const float* V = S.viewmatrix;
    float m[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, op = 0.f, sc[3] = {1.f, 1.f, 1.f};
    float ix = 0.f, iy = 0.f, conA = 0.f, conB = 0.f, conC = 0.f;
    Proj p;
    p.tx = p.ty = p.tz = 0.f;
    // the scales are requested with the other parameters, not behind the near-plane test they used to wait for (one HBM round trip less
    // on the way to the visibility decision; a culled Gaussian's 12 bytes are read in vain: measured 0.180 -> 0.172 ms)
    float sc_raw[3] = {0.f, 0.f, 0.f};
    if (PART == 2) {
        // colour half: visibility from the geometry half's radii; the world mean again (static point: the parameter itself)
        if (i < a.N && a.radii[i] > 0) {
            touched = 1u;
            if (a.flags & EMD_FLAG_MOTION) motion_point(i, a.means3D, a.rotations, a.opacities, a.motion, m, q, &op, (a.flags & EMD_FLAG_RAW_PARAMS) != 0);
            else { m[0] = a.means3D[3 * i]; m[1] = a.means3D[3 * i + 1]; m[2] = a.means3D[3 * i + 2]; }
        }
    } else if (i < a.N) {
        const float* P = S.projmatrix;
        const int W = S.image_width, H = S.image_height;
        const int gx = (W + EMD_TILE_X - 1) / EMD_TILE_X, gy = (H + EMD_TILE_Y - 1) / EMD_TILE_Y;
        const float fx = (float)W / (2.f * S.tanfovx), fy = (float)H / (2.f * S.tanfovy);
        const bool raw = (a.flags & EMD_FLAG_RAW_PARAMS) != 0;
        {
            // (twin of gaussian_pose_body.inc, K8's loads and world pose: K1 has no gradient row to stand in for an absent array and forms the pose
            // inside its branches, so the shared text would change K1's machine code)
            // Round 5 (late), as in K8: every load whose address depends on the index alone is issued here, back to back, before any is used (optional
            // inputs through a pointer that is valid either way -- the Gaussian's own mean stands in --, selected where they are used); then the actor's pose
            // rows.  Before: mean -> actor id -> quaternion / pose rows -> opacity, each behind the wait of the one before.
            const bool motion = (a.flags & EMD_FLAG_MOTION) != 0;
            const bool has_ids = motion && a.motion.actor_id != nullptr, has_rot = a.rotations != nullptr;
            const bool has_rdx = motion && a.motion.residual_dx != nullptr, has_rdq = motion && has_rot && a.motion.residual_dq != nullptr;
            const float* mp = a.means3D + 3 * (size_t)i;
            const float* xp = has_rdx ? a.motion.residual_dx + 3 * (size_t)i : mp;
            const float* sp = a.cov3D_precomp ? mp : a.scales + 3 * (size_t)i;
            const int aid_raw = *(has_ids ? a.motion.actor_id + i : (const int*)mp);
            const float m0 = mp[0], m1 = mp[1], m2 = mp[2];
            const float x0 = xp[0], x1 = xp[1], x2 = xp[2];
            const float s0 = sp[0], s1 = sp[1], s2 = sp[2];
            const float opv = a.opacities[i];
            // (a quaternion row is 16 bytes at a 16-byte stride; without rotations the stand-in is read as three dwords + one)
            float4 qq = make_float4(0.f, 0.f, 0.f, 0.f), dqq = qq;
            if (has_rot) qq = *(const float4*)(a.rotations + 4 * (size_t)i);                 // (kernel-uniform; the loads above are already in flight)
            if (has_rdq) dqq = *(const float4*)(a.motion.residual_dq + 4 * (size_t)i);
            const int aid = has_ids ? aid_raw : -1;
            float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0;
            if (aid >= 0) {
                const float4* Pp = (const float4*)(a.motion.actor_pose + (size_t)aid * EMD_ACTOR_STRIDE);
                p0 = Pp[0]; p1 = Pp[1]; p2 = Pp[2];
            }
            if (!a.cov3D_precomp) { sc_raw[0] = s0; sc_raw[1] = s1; sc_raw[2] = s2; }
            if (motion) {
                const float ml[3] = {has_rdx ? m0 + x0 : m0, has_rdx ? m1 + x1 : m1, has_rdx ? m2 + x2 : m2};
                motion_apply(ml, aid, has_rot, qq, has_rdq, dqq, true, opv, p0, p1, p2, raw, m, q, &op);
            } else {
                op = raw ? sigmoidf_(opv) : opv;
                m[0] = m0; m[1] = m1; m[2] = m2;
                if (has_rot) {
                    q[0] = qq.x; q[1] = qq.y; q[2] = qq.z; q[3] = qq.w;
                    if (raw) { const float n = fmaxf(quat_norm(q), 1e-12f); q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n; }
                }
            }
        }
        view_transform(V, m, p.tx, p.ty, p.tz);
        if (p.tz > S.near_plane) {
            const Clip h = clip_transform(P, m);
            const float hx = h.hx, hy = h.hy, pw = h.pw;
            float px = hx * pw, py = hy * pw;
            float c3[6];
            if (a.cov3D_precomp) {
#pragma unroll
                for (int k = 0; k < 6; k++) c3[k] = a.cov3D_precomp[6 * i + k];
            } else {
                sc[0] = sc_raw[0]; sc[1] = sc_raw[1]; sc[2] = sc_raw[2];
                if (raw) { sc[0] = expf(sc[0]); sc[1] = expf(sc[1]); sc[2] = expf(sc[2]); }
                cov3d_from_sr(sc, S.scale_modifier, q, c3);
            }
            project_cov2d(S, c3, fx, fy, p);
            if (p.det != 0.f) {
                float det_inv = 1.f / p.det;
                conA = p.c * det_inv; conB = -p.b * det_inv; conC = p.a * det_inv;
                float mid = 0.5f * (p.a + p.c);
                float sq = sqrtf(fmaxf(0.1f, mid * mid - p.det));
                float lam1 = mid + sq, lam2 = mid - sq;
                float rad = ceilf(3.f * sqrtf(fmaxf(lam1, lam2)));
                ix = ((px + 1.f) * (float)W - 1.f) * 0.5f;
                iy = ((py + 1.f) * (float)H - 1.f) * 0.5f;
                int x0 = tile_clamp((ix - rad) / (float)EMD_TILE_X, gx);
                int y0 = tile_clamp((iy - rad) / (float)EMD_TILE_Y, gy);
                int x1 = tile_clamp((ix + rad + (float)(EMD_TILE_X - 1)) / (float)EMD_TILE_X, gx);
                int y1 = tile_clamp((iy + rad + (float)(EMD_TILE_Y - 1)) / (float)EMD_TILE_Y, gy);
                int area = (x1 - x0) * (y1 - y0);
                if (area > 0) {
                    touched = (uint32_t)area;
                    dkey = __float_as_uint(p.tz);
                    radius_out = (int)rad;
                    // Round 4: the rectangle the binning ENUMERATES is upstream's 3-sigma square cut down to the tiles the alpha >= 1/255
                    // ellipse of this Gaussian can reach: a pixel contributes only where d^T Conic d <= 2 ln(255 o), whose bounding box
                    // has the half extents sqrt(2 ln(255 o) cov_xx), sqrt(. cov_yy) -- straight from the 2-D covariance, no division.
                    // Pixel centres are integers, so the box is kept as the range of 8-pixel quadrant columns / rows that hold a centre
                    // inside it (11 bits each, clamped to the image): the duplicate kernel derives every pair's quadrant mask from it.
                    const float thr = 2.f * __logf(255.f * op) * 1.01f + 0.05f;           // (same margin as footprint.h)
                    float bx = __builtin_sqrtf(thr * p.a) * 1.0001f + 0.01f, by = __builtin_sqrtf(thr * p.c) * 1.0001f + 0.01f;
                    const bool never = !(op >= (1.f / 255.f));                            // cannot reach 1/255 anywhere (also NaN)
                    if (!(bx == bx) || !(by == by)) bx = by = 3.0e38f;                    // (NaN covariance entries: keep everything)
                    //  the render kernels evaluate alpha with the float conic adj(cov) / fl(det), whose relative error is
                    // ~1.2e-7 a c / det: for needle footprints (a c > 3e4 det -- hundreds of pixels long, under a pixel wide) the 1 % + 0.05
                    // margin above no longer covers it, so such a Gaussian keeps upstream's rectangle and all four quadrants, exactly as
                    // footprint.h refuses to cull it (`e.all`)
                    if (!(p.det * 3.0e4f > p.a * p.c)) bx = by = 3.0e38f;
                    const float QMAX = 2047.f;
                    const float lqxf = floorf(ceilf(ix - bx) * 0.125f), hqxf = floorf(floorf(ix + bx) * 0.125f);
                    const float lqyf = floorf(ceilf(iy - by) * 0.125f), hqyf = floorf(floorf(iy + by) * 0.125f);
                    const bool off = never || hqxf < 0.f || hqyf < 0.f || lqxf > QMAX || lqyf > QMAX || !(lqxf == lqxf) || !(lqyf == lqyf);
                    const int lqx = (int)fminf(fmaxf(lqxf, 0.f), QMAX), hqx = (int)fminf(fmaxf(hqxf, 0.f), QMAX);
                    const int lqy = (int)fminf(fmaxf(lqyf, 0.f), QMAX), hqy = (int)fminf(fmaxf(hqyf, 0.f), QMAX);
                    int cx0 = x0, cy0 = y0, cx1 = x1, cy1 = y1;
                    if (!(a.flags & EMD_FLAG_KEEP_ALL_PAIRS)) {
                        cx0 = max(x0, lqx >> 1); cx1 = min(x1, (hqx >> 1) + 1);
                        cy0 = max(y0, lqy >> 1); cy1 = min(y1, (hqy >> 1) + 1);
                        if (off || cx1 <= cx0 || cy1 <= cy0) { cx1 = cx0; cy1 = cy0; }
                        // Inside the cut rectangle every quadrant lies in the box except, possibly, the outer quadrant column / row of its
                        // first and last tile: where the rectangle ends at the box (not at upstream's square) and the box starts in the
                        // right (odd) / ends in the left (even) quadrant column -- rows likewise.  Four bits give every pair its mask.
                        skip = ((cx0 == (lqx >> 1) && (lqx & 1)) ? 1u : 0u) | ((cx1 - 1 == (hqx >> 1) && !(hqx & 1)) ? 2u : 0u) |
                               ((cy0 == (lqy >> 1) && (lqy & 1)) ? 4u : 0u) | ((cy1 - 1 == (hqy >> 1) && !(hqy & 1)) ? 8u : 0u);
                    }       // (with every pair kept the masks are all ones: the render forward's own sub-block test decides)
                    rect = (uint32_t)cx0 | ((uint32_t)cy0 << 10) | ((uint32_t)(cx1 - cx0) << 20) | ((skip & 3u) << 30);
                    rect_h = (uint32_t)(cy1 - cy0) | ((skip >> 2) << 10);
                }
            }
        }
        a.radii[i] = radius_out;
        // binning input (by Gaussian id), 8 bytes: x = ENUMERATED tile rectangle x0 | y0 << 10 | width << 20 | skip-left/right bits << 30,
        // y = its height | skip-top/bottom bits << 10 | upstream's tiles touched << 12
        a.g.binrec[i] = make_uint2(rect, rect_h | (touched << 12));
        a.g.depth_key[i] = dkey;                         // key of the depth sort (invisible: sorts last)
        a.g.contrib[i] = 0u;                             // every forward hands the backward a clean array: K7 raises the words, K8 reads them
    }
    const bool vis = touched != 0u;
    float sh[48];
    if (PART != 1 && sh_staged) {
        // rows of the VISIBLE Gaussians only, in two halves of 32 rows: coalesced dwordx4 pieces into LDS, then each lane of the half
        // takes its own row into registers
        const unsigned long long vmask = __ballot(vis);
        const size_t base4 = (size_t)blk * PRE_BLOCK * 12;
        const float4* src = (const float4*)a.shs;
        // Round 4: all twelve pieces of the wave's rows are requested at once -- both halves in flight together, one HBM round trip instead
        // of two -- and then staged half by half (48 registers more while they fly: four waves per SIMD instead of five; measured
        // 738 -> 745 it/s, and 730 at five waves, which spills).  The instantiation with residuals keeps the half-by-half loads.
        constexpr bool SH_ALL = !RES;
        float4 pv[SH_ALL ? 12 : 1];
        if (SH_ALL) {
#pragma unroll
            for (int j = 0; j < 12; j++) {
                const uint32_t idx = threadIdx.x + PRE_BLOCK * j, row = idx / 12;
                pv[SH_ALL ? j : 0] = make_float4(0.f, 0.f, 0.f, 0.f);
                if ((vmask >> row) & 1ull) pv[SH_ALL ? j : 0] = load_f4_nt(src + base4 + idx);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const uint32_t idx = threadIdx.x + PRE_BLOCK * (6 * h + j), row = idx / 12;
                if ((vmask >> row) & 1ull) {
                    float4 v;
                    if (SH_ALL) v = pv[SH_ALL ? 6 * h + j : 0];
                    else {
                        v = src[base4 + idx];
                        if (RES && a.shs_res0) {                          // (shs + r0) + r1, the order of the reference's two adds
                            const float4 r = ((const float4*)a.shs_res0)[base4 + idx];
                            v.x = v.x + r.x; v.y = v.y + r.y; v.z = v.z + r.z; v.w = v.w + r.w;
                        }
                        if (RES && a.shs_res1) {
                            const float4 r = ((const float4*)a.shs_res1)[base4 + idx];
                            v.x = v.x + r.x; v.y = v.y + r.y; v.z = v.z + r.z; v.w = v.w + r.w;
                        }
                    }
                    s_sh[(row - 32 * h) * SH_ROW4 + (idx % 12)] = v;
                }
            }
            __syncthreads();
            if ((int)(threadIdx.x >> 5) == h) {
#pragma unroll
                for (int j = 0; j < 12; j++) {
                    const float4 t = s_sh[(threadIdx.x & 31) * SH_ROW4 + j];
                    sh[4 * j] = t.x; sh[4 * j + 1] = t.y; sh[4 * j + 2] = t.z; sh[4 * j + 3] = t.w;
                }
            }
            __syncthreads();
        }
    }
    if (vis) {
        float col[3] = {0.f, 0.f, 0.f};
        uint32_t bits = 0;
        if (PART == 1) {
            // (geometry half: no colour)
        } else if (a.colors_precomp) {
            col[0] = a.colors_precomp[3 * i]; col[1] = a.colors_precomp[3 * i + 1];
            col[2] = a.colors_precomp[3 * i + 2];
        } else {
            float d[3] = {m[0] - S.campos[0], m[1] - S.campos[1], m[2] - S.campos[2]};
            float n = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            d[0] /= n; d[1] /= n; d[2] /= n;
            float bs[16];
            sh_basis(S.sh_degree, d, bs);
            const int K = (S.sh_degree + 1) * (S.sh_degree + 1);
            if (!sh_staged) sh_row_load(a.shs, RES ? a.shs_res0 : nullptr, RES ? a.shs_res1 : nullptr, i, a.M, K, sh);
            col[0] = col[1] = col[2] = 0.f;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if (k < K) { col[0] += bs[k] * sh[3 * k]; col[1] += bs[k] * sh[3 * k + 1]; col[2] += bs[k] * sh[3 * k + 2]; }
            }
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                col[ch] += 0.5f;
                if (col[ch] < 0.f) { col[ch] = 0.f; bits |= 1u << ch; }
                if ((a.flags & EMD_FLAG_CLAMP_RGB01) && col[ch] > 1.f) { col[ch] = 1.f; bits |= 1u << ch; }
            }
            float J[9];
            sh_dir_jacobian(S.sh_degree, d, sh, J);
            float4* jr = a.g.shjac + (size_t)i * 3;
            // (the spare word of row 0 carries the clamp bits: the projection backward reads them here, with the Jacobian it needs anyway)
            const float bw = __uint_as_float(bits);
            store_f4_nt(jr, make_float4(J[0], J[1], J[2], bw));
            store_f4_nt(jr + 1, make_float4(J[3], J[4], J[5], 0.f));
            store_f4_nt(jr + 2, make_float4(J[6], J[7], J[8], 0.f));
        }
        float4* rec = a.g.rec + (size_t)i * EMD_REC_F4;
        // the clamp bits of the colour ride in row 2 (with the colour they belong to), so that the two halves write disjoint rows
        if (PART != 2) { rec[0] = make_float4(ix, iy, p.tz, op); rec[1] = make_float4(conA, conB, conC, 0.f); }
        if (PART != 1) rec[2] = make_float4(col[0], col[1], col[2], __uint_as_float(bits));
        if (PART != 2 && (a.flags & EMD_FLAG_NORMAL)) {
            float nv[3] = {0.f, 0.f, 0.f};
            if (a.scales) {
                int ax = 0;
                if (sc[1] < sc[ax]) ax = 1;
                if (sc[2] < sc[ax]) ax = 2;
                float R[9];
                quat_to_R(q, R);
                float nw[3] = {R[ax], R[3 + ax], R[6 + ax]};
                nv[0] = (V[0] * nw[0] + V[4] * nw[1]) + V[8] * nw[2];
                nv[1] = (V[1] * nw[0] + V[5] * nw[1]) + V[9] * nw[2];
                nv[2] = (V[2] * nw[0] + V[6] * nw[1]) + V[10] * nw[2];
                float dp = (nv[0] * p.tx + nv[1] * p.ty) + nv[2] * p.tz;
                if (dp > 0.f) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
            }
            rec[3] = make_float4(nv[0], nv[1], nv[2], 0.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// K8
// ---------------------------------------------------------------------------------------------------
#define K8_BLOCK 256          // threads per workgroup of K8 (A/B: 64 = one wave per workgroup, no cross-wave barrier coupling)
#define K8_HALF (K8_BLOCK / 2)
#define EMD_K8_WAVES 4        // round 3: with the SH rows stored first the live state across the staging barriers needs 112 VGPRs; at 5 waves it spills
// PZ (PreBwdArgs.shs_prezeroed): the instantiation behind a render backward that zeroed dL/dshs; the dense one is the kernel as it was
template <bool PZ>
__global__ void __launch_bounds__(K8_BLOCK) __attribute__((amdgpu_waves_per_eu(EMD_K8_WAVES))) k_preprocess_backward(PreBwdArgs a) {
    EmdSettings S = a.s;
    emd_settings_from_device(S, a.sdev, a.flags);
    // staging of the dL/dshs rows (coalesced copy-out), half of the block's rows at a time: 26 KB instead of 52 keeps five
    // workgroup-waves per SIMD resident instead of three.  A row is the outer product basis[k] x gc[c]: the lane keeps the 19 factors
    // and multiplies them out when its half is staged.
    __shared__ float4 s_sh[K8_HALF * SH_ROW4];
    float sh_b[16], sh_g[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 16; k++) sh_b[k] = 0.f;
    const bool sh_staged = a.shs && a.M == 16;
    // Round 5: 47 % of the Gaussians of a view are invisible, so a lane-per-Gaussian wave works with half of its lanes.  The visible Gaussians
    // of the workgroup's 256 are compacted (in index order) onto its first lanes: ~2.1 full waves run the loads and the chain rule, the rest of
    // the workgroup only writes the zero rows of the invisible ones ("natural" duties: thread t for Gaussian t of the block).
    __shared__ uint32_t s_cscan[K8_BLOCK / 64];
    __shared__ uint16_t s_list[K8_BLOCK];
    const int inat = blockIdx.x * K8_BLOCK + threadIdx.x;
    const bool nat_in = inat < a.N;
    // "Visible" here is "the render backward added to this Gaussian's accumulator row" (GeomWs::contrib): more than half of the radii > 0 Gaussians of a
    // street view sit behind the depth at which their tiles saturate, their rows are all zero and so is every output -- they take the zero-row duty
    // instead of a compacted lane.  (EMD_FLAG_DETERMINISTIC keeps radii > 0: its pose rows are keyed by the radii.)  One pointer, chosen kernel-uniformly.
    const int32_t* const vis_words = emd_bwd_visible_words(a.flags, a.radii, a.g);
    const bool nat_vis = nat_in && vis_words[inat] > 0;
    uint32_t nv;
    {
        // inclusive scan of the visibility flags over the workgroup (any number of waves)
        const uint32_t winc = wave_scan_add_u32(nat_vis ? 1u : 0u), wv = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 63) s_cscan[wv] = winc;
        __syncthreads();
        uint32_t wbase = 0;
        nv = 0;
#pragma unroll
        for (uint32_t w = 0; w < K8_BLOCK / 64; w++) { const uint32_t c = s_cscan[w]; if (w < wv) wbase += c; nv += c; }
        const uint32_t incl = wbase + winc;
        if (nat_vis) s_list[incl - 1u] = (uint16_t)threadIdx.x;
        __syncthreads();
    }
    const bool in_range = threadIdx.x < nv;                        // this thread carries a visible Gaussian
    const int lrow = in_range ? (int)s_list[threadIdx.x] : 0;      // its row inside the block
    const int i = blockIdx.x * K8_BLOCK + lrow;
    const bool nat_zero = nat_in && !nat_vis;                      // this thread also owns the zero row of an invisible Gaussian
    const float* V = S.viewmatrix;
    const float* P = S.projmatrix;
    const int W = S.image_width, H = S.image_height;
    const float fx = (float)W / (2.f * S.tanfovx), fy = (float)H / (2.f * S.tanfovy);
    float dm[3] = {0.f, 0.f, 0.f}, dq[4] = {0.f, 0.f, 0.f, 0.f}, ds[3] = {0.f, 0.f, 0.f}, dop = 0.f;
    float dc6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float gm2[2] = {0.f, 0.f}, gabs[2] = {0.f, 0.f};
    int a_id = -1;
    float pose_g[12];
#pragma unroll
    for (int k = 0; k < 12; k++) pose_g[k] = 0.f;
    // Part 1: loads, the Gaussian's world pose, and the SH colour part (whose dense 192-byte rows leave FIRST, below: their stores
    // then drain while the wave works through the geometry chain of part 2 instead of at the very end of its life)
    const bool raw = (a.flags & EMD_FLAG_RAW_PARAMS) != 0;
    float m[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, op = 0.f, q_norm = 1.f;
    float gcol[3] = {0.f, 0.f, 0.f}, sh_gc[3] = {0.f, 0.f, 0.f};
    float g_depth = 0.f, gA = 0.f, gB = 0.f, gC = 0.f;
    float sc_in[3] = {0.f, 0.f, 0.f};       // (loaded in part 1: no global load waits behind the staging barriers)
    Proj p;
    p.tx = p.ty = p.tz = 0.f;
    // Round 5 (late): every load of a visible Gaussian is issued back to back before any of them is used, and its world pose formed from the loaded
    // values: gaussian_pose_body.inc, the text the camera-gradient kernel includes as well.  Before, the loads sat in the branches that use them (motion /
    // raw quaternion / scales / gradient row / Jacobian, each kernel-uniform or per-lane): seven load -> s_waitcnt -> use rounds one behind the other,
    // each a trip to the Infinity Cache or HBM, in a kernel whose compacted blocks keep ~2 waves busy.
    // (the three lines of flags are restated in K1 and in k_camera_backward, camera_grad.hip: as a function they moved this kernel's machine code)
    const bool motion = (a.flags & EMD_FLAG_MOTION) != 0;
    const bool has_ids = motion && a.motion.actor_id != nullptr, has_rot = a.rotations != nullptr;
    const bool has_rdx = motion && a.motion.residual_dx != nullptr, has_rdq = motion && has_rot && a.motion.residual_dq != nullptr;
    const float4 z4c = make_float4(0.f, 0.f, 0.f, 0.f);
    float mloc[3] = {0.f, 0.f, 0.f}, op_raw = 0.f;
    float4 q_raw = z4c, rdq = z4c, pr0 = z4c, pr1 = z4c, pr2 = z4c;
    if (in_range) {
        // (a_id of every compacted Gaussian: the pose-gradient reduction at the end looks at whole waves)
        constexpr bool consume_row = true;              // the opacity too, and the row is handed back clean
#include "gaussian_pose_body.inc"
        if (!a.cov3D_precomp) { sc_in[0] = s0; sc_in[1] = s1; sc_in[2] = s2; }
        gm2[0] = g0.x; gm2[1] = g0.y;
        if (a.flags & EMD_FLAG_ABSGRAD) { gabs[0] = g2.z; gabs[1] = g2.w; }
        g_depth = g0.z;
        dop = g0.w;
        gA = g1.x; gB = g1.y; gC = g1.z;
        gcol[0] = g1.w; gcol[1] = g2.x; gcol[2] = g2.y;
        view_transform(V, m, p.tx, p.ty, p.tz);
        // (e) colour
        if (!a.colors_precomp) {
#include "sh_dir_grad_body.inc"
            sh_gc[0] = gc[0]; sh_gc[1] = gc[1]; sh_gc[2] = gc[2];
            const int deg = S.sh_degree;
            const int K = (deg + 1) * (deg + 1);
            float bs[16];
            sh_basis(deg, d, bs);
            if (a.dL_dshs) {
                if (sh_staged) {          // the factors of this Gaussian's row; multiplied out at staging time
#pragma unroll
                    for (int k = 0; k < 16; k++) sh_b[k] = k < K ? bs[k] : 0.f;
                    sh_g[0] = gc[0]; sh_g[1] = gc[1]; sh_g[2] = gc[2];
                } else {
                    float* o = a.dL_dshs + (size_t)i * a.M * 3;
                    for (int k = 0; k < a.M; k++) {
                        float bk = k < K ? bs[k] : 0.f;
                        o[3 * k] = bk * gc[0]; o[3 * k + 1] = bk * gc[1]; o[3 * k + 2] = bk * gc[2];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 3; k++) dm[k] += (gd[k] - d[k] * dot) / n;
        }
    }
    if (nat_zero && a.dL_dshs && !sh_staged) {
        float* o = a.dL_dshs + (size_t)inat * a.M * 3;
        for (int k = 0; k < 3 * a.M; k++) o[k] = 0.f;
    }
    // PZ: K7's workgroups zeroed every row of dL/dshs in front of this kernel (api.hip), so only the compacted Gaussians' rows are staged and only their
    // 16-byte pieces stored: the copy-out walks the compaction list itself (the same `vis_words[i] > 0` flags, in index order: the first s_cscan[0] +
    // s_cscan[1] entries are the rows of the first half), twelve consecutive threads per row -- one or two trips for the ~30 rows of a half instead of six
    // over all 128.  A flagged Gaussian's row is written exactly as in the dense form, +-0 included; nobody writes a zero row into the tile, and a half
    // (so a workgroup) without a contributor skips its staging and its barriers.
    static_assert(K8_HALF == 128 && K8_BLOCK == 256, "the waves' counts s_cscan[0..1] / s_cscan[2..3] are the two halves' row counts");
    if (sh_staged && a.dL_dshs) {
        const size_t lim4 = (size_t)a.N * 12;
        float4* out = (float4*)a.dL_dshs;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            uint32_t k0 = 0, kn = 0;          // PZ: the half's rows are entries k0 .. k0 + kn - 1 of s_list (uniform over the workgroup)
            if (PZ) {
                // (read into scalar registers: the kernel has no vector register to spare across the barriers)
                const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(s_cscan[0] + s_cscan[1]));
                k0 = h ? c0 : 0u; kn = h ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(s_cscan[2] + s_cscan[3])) : c0;
                if (kn == 0) continue;
            }
            if (in_range && (int)(lrow / K8_HALF) == h) {
                float g48[48];
#pragma unroll
                for (int k = 0; k < 16; k++) { g48[3 * k] = sh_b[k] * sh_g[0]; g48[3 * k + 1] = sh_b[k] * sh_g[1]; g48[3 * k + 2] = sh_b[k] * sh_g[2]; }
#pragma unroll
                for (int j = 0; j < 12; j++)
                    s_sh[(lrow % K8_HALF) * SH_ROW4 + j] = make_float4(g48[4 * j], g48[4 * j + 1], g48[4 * j + 2], g48[4 * j + 3]);
            }
            if (!PZ && !nat_vis && (int)(threadIdx.x / K8_HALF) == h) {          // the zero row of an invisible (or absent) Gaussian
#pragma unroll
                for (int j = 0; j < 12; j++) s_sh[(threadIdx.x % K8_HALF) * SH_ROW4 + j] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            __syncthreads();
            if (PZ) {
                float4* const blk_out = out + (size_t)blockIdx.x * K8_BLOCK * 12;
                for (uint32_t p = threadIdx.x; p < 12u * kn; p += K8_BLOCK) {
                    const uint32_t row = s_list[k0 + p / 12u], piece = p % 12u;          // (a compacted row lies below N)
                    store_f4_nt(blk_out + row * 12u + piece, s_sh[(row % K8_HALF) * SH_ROW4 + piece]);
                }
            } else {
                const size_t base4 = ((size_t)blockIdx.x * K8_BLOCK + K8_HALF * h) * 12;
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    const uint32_t idx = threadIdx.x + K8_BLOCK * j;
                    if (base4 + idx < lim4) store_f4_nt(out + base4 + idx, s_sh[(idx / 12) * SH_ROW4 + (idx % 12)]);
                }
            }
            __syncthreads();
        }
    }
    // Part 2: the geometry chain and the remaining (small) stores
    // Round 5: the five small gradients every training step writes -- means3D [N,3], scales [N,3], rotations [N,4], opacities [N], means2D
    // [N,3]: 56 bytes per Gaussian as fourteen dword stores at strides of 12 / 16 / 4 bytes -- leave through the (now idle) SH staging tile
    // as whole 16-byte NONTEMPORAL stores: nothing reads them before the optimiser, and kept out of the Infinity Cache they stop evicting
    // the parameters this kernel has just read and the next step's projection kernel asks for first.
    // (the tile also is where the values of the compacted lanes and the zeros of the invisible Gaussians meet in index order)
    const bool staged5 = a.dL_dmeans3D && a.dL_dscales && a.dL_drotations && a.dL_dopacities && a.dL_dmeans2D &&
                         (((uintptr_t)a.dL_dmeans3D | (uintptr_t)a.dL_dscales | (uintptr_t)a.dL_drotations | (uintptr_t)a.dL_dopacities |
                           (uintptr_t)a.dL_dmeans2D) & 15) == 0 && (size_t)(blockIdx.x + 1) * K8_BLOCK <= (size_t)a.N;     // (uniform per workgroup; a ragged last block stores directly)
    float o_dl[3] = {0.f, 0.f, 0.f}, o_ds[3] = {0.f, 0.f, 0.f}, o_dq[4] = {0.f, 0.f, 0.f, 0.f}, o_dop = 0.f;
    if (in_range) {
        // (a) conic -> cov2D, (b) cov2D -> Sigma and J, t
        float c3[6];
        float sc[3] = {1.f, 1.f, 1.f};
        if (a.cov3D_precomp) {
#pragma unroll
            for (int k = 0; k < 6; k++) c3[k] = a.cov3D_precomp[6 * i + k];
        } else {
            sc[0] = sc_in[0]; sc[1] = sc_in[1]; sc[2] = sc_in[2];
            if (raw) { sc[0] = expf(sc[0]); sc[1] = expf(sc[1]); sc[2] = expf(sc[2]); }
            cov3d_from_sr(sc, S.scale_modifier, q, c3);
        }
        project_cov2d(S, c3, fx, fy, p);
#include "conic_bwd_body.inc"
        const float* M0 = p.M0; const float* M1 = p.M1;
        dc6[0] = da * M0[0] * M0[0] + db * M0[0] * M1[0] + dc * M1[0] * M1[0];
        dc6[3] = da * M0[1] * M0[1] + db * M0[1] * M1[1] + dc * M1[1] * M1[1];
        dc6[5] = da * M0[2] * M0[2] + db * M0[2] * M1[2] + dc * M1[2] * M1[2];
        dc6[1] = 2.f * da * M0[0] * M0[1] + db * (M0[0] * M1[1] + M0[1] * M1[0]) + 2.f * dc * M1[0] * M1[1];
        dc6[2] = 2.f * da * M0[0] * M0[2] + db * (M0[0] * M1[2] + M0[2] * M1[0]) + 2.f * dc * M1[0] * M1[2];
        dc6[4] = 2.f * da * M0[1] * M0[2] + db * (M0[1] * M1[2] + M0[2] * M1[1]) + 2.f * dc * M1[1] * M1[2];
#include "cov2d_bwd_body.inc"
#pragma unroll
        for (int k = 0; k < 3; k++) dm[k] += V[4 * k + 0] * dt[0] + V[4 * k + 1] * dt[1] + V[4 * k + 2] * dt[2];
        // (c) pixel mean -> clip -> world
        float gxn = 0.5f * (float)W * gm2[0], gyn = 0.5f * (float)H * gm2[1];
        gm2[0] = gxn; gm2[1] = gyn;
        gabs[0] *= 0.5f * (float)W; gabs[1] *= 0.5f * (float)H;
        const Clip h = clip_transform(P, m);
        const float hx = h.hx, hy = h.hy, pw = h.pw;
        float mul1 = hx * pw * pw, mul2 = hy * pw * pw;
#pragma unroll
        for (int k = 0; k < 3; k++)
            dm[k] += (P[4 * k] * pw - P[4 * k + 3] * mul1) * gxn + (P[4 * k + 1] * pw - P[4 * k + 3] * mul2) * gyn;
        // (f) Sigma -> scale, quaternion
        if (!a.cov3D_precomp) {
            float R[9], L[9];
            quat_to_R(q, R);
            const float mod = S.scale_modifier;
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int k = 0; k < 3; k++) L[3 * r + k] = R[3 * r + k] * (mod * sc[k]);
            const float Gf[9] = {dc6[0], 0.5f * dc6[1], 0.5f * dc6[2], 0.5f * dc6[1], dc6[3], 0.5f * dc6[4],
                                 0.5f * dc6[2], 0.5f * dc6[4], dc6[5]};
            float dL[9], dR[9];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int k = 0; k < 3; k++)
                    dL[3 * r + k] = 2.f * ((Gf[3 * r] * L[k] + Gf[3 * r + 1] * L[3 + k]) + Gf[3 * r + 2] * L[6 + k]);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                ds[k] = mod * ((dL[k] * R[k] + dL[3 + k] * R[3 + k]) + dL[6 + k] * R[6 + k]);
#pragma unroll
                for (int r = 0; r < 3; r++) dR[3 * r + k] = dL[3 * r + k] * (mod * sc[k]);
            }
            dR_to_dq(q, dR, dq);
            if (raw) { ds[0] *= sc[0]; ds[1] *= sc[1]; ds[2] *= sc[2]; }   // d exp(x) = exp(x)
        }
        if (a.dL_dmeans2D && !staged5) { a.dL_dmeans2D[3 * i] = gm2[0]; a.dL_dmeans2D[3 * i + 1] = gm2[1]; a.dL_dmeans2D[3 * i + 2] = 0.f; }
        if (a.dL_dmeans2D_abs) { a.dL_dmeans2D_abs[2 * i] = gabs[0]; a.dL_dmeans2D_abs[2 * i + 1] = gabs[1]; }
        if (a.dL_dsh_color) { a.dL_dsh_color[3 * i] = sh_gc[0]; a.dL_dsh_color[3 * i + 1] = sh_gc[1]; a.dL_dsh_color[3 * i + 2] = sh_gc[2]; }
        if (a.dL_dcolors) { a.dL_dcolors[3 * i] = gcol[0]; a.dL_dcolors[3 * i + 1] = gcol[1]; a.dL_dcolors[3 * i + 2] = gcol[2]; }
        for (int k = 0; k < a.num_extra; k++) {           // extra colour sets: the accumulated dL/d colour is the gradient of the input itself
            float4* gxp = (float4*)(a.grad_rec + (size_t)i * a.bwd_stride + EMD_BWD_PAYLOAD + 4 * k);
            const float4 gx = *gxp;
            if (a.flags & EMD_FLAG_BWD_WS_CLEAN) *gxp = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!a.dL_dextra[k]) continue;
            a.dL_dextra[k][3 * i] = gx.x; a.dL_dextra[k][3 * i + 1] = gx.y; a.dL_dextra[k][3 * i + 2] = gx.z;
        }
        if (a.dL_dcov3D) {
#pragma unroll
            for (int k = 0; k < 6; k++) a.dL_dcov3D[6 * i + k] = dc6[k];
        }
        if (a.dL_dscales && !staged5) { a.dL_dscales[3 * i] = ds[0]; a.dL_dscales[3 * i + 1] = ds[1]; a.dL_dscales[3 * i + 2] = ds[2]; }
        // (h) explicit motion
        float dl[3] = {dm[0], dm[1], dm[2]}, dql[4] = {dq[0], dq[1], dq[2], dq[3]}, dopl = dop;
        if (a_id >= 0)
            motion_backward_apply(mloc, has_rot, q_raw, has_rdq, rdq, true, op_raw, pr0, pr1, pr2, dm, dq, dop, dl, dql, &dopl, pose_g, raw);
        if (raw) {
            if (a_id < 0 && has_rot) dnormalize4(q, q_norm, dq, dql);              // through F.normalize of the raw quaternion
            const float o = sigmoidf_(op_raw);
            dopl *= o * (1.f - o);                                                 // through the sigmoid
        }
        if (staged5) {
            o_dl[0] = dl[0]; o_dl[1] = dl[1]; o_dl[2] = dl[2]; o_ds[0] = ds[0]; o_ds[1] = ds[1]; o_ds[2] = ds[2];
            o_dq[0] = dql[0]; o_dq[1] = dql[1]; o_dq[2] = dql[2]; o_dq[3] = dql[3]; o_dop = dopl;
        }
        if (a.dL_dmeans3D && !staged5) { a.dL_dmeans3D[3 * i] = dl[0]; a.dL_dmeans3D[3 * i + 1] = dl[1]; a.dL_dmeans3D[3 * i + 2] = dl[2]; }
        if (a.dL_dresidual_dx) { a.dL_dresidual_dx[3 * i] = dl[0]; a.dL_dresidual_dx[3 * i + 1] = dl[1]; a.dL_dresidual_dx[3 * i + 2] = dl[2]; }
        if (a.dL_drotations && !staged5) *(float4*)(a.dL_drotations + 4 * i) = make_float4(dql[0], dql[1], dql[2], dql[3]);
        if (a.dL_dresidual_dq) {
            *(float4*)(a.dL_dresidual_dq + 4 * i) = a_id >= 0 ? make_float4(dql[0], dql[1], dql[2], dql[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (a.dL_dopacities && !staged5) a.dL_dopacities[i] = dopl;
    }
    if (nat_zero) {
        // the rows no compacted lane owns: zeros (the five main arrays only when they do not leave through the tile below)
        const size_t z = (size_t)inat;
        if (!staged5) {
            if (a.dL_dmeans2D) { a.dL_dmeans2D[3 * z] = 0.f; a.dL_dmeans2D[3 * z + 1] = 0.f; a.dL_dmeans2D[3 * z + 2] = 0.f; }
            if (a.dL_dscales) { a.dL_dscales[3 * z] = 0.f; a.dL_dscales[3 * z + 1] = 0.f; a.dL_dscales[3 * z + 2] = 0.f; }
            if (a.dL_dmeans3D) { a.dL_dmeans3D[3 * z] = 0.f; a.dL_dmeans3D[3 * z + 1] = 0.f; a.dL_dmeans3D[3 * z + 2] = 0.f; }
            if (a.dL_drotations) *(float4*)(a.dL_drotations + 4 * z) = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a.dL_dopacities) a.dL_dopacities[z] = 0.f;
        }
        if (a.dL_dmeans2D_abs) { a.dL_dmeans2D_abs[2 * z] = 0.f; a.dL_dmeans2D_abs[2 * z + 1] = 0.f; }
        if (a.dL_dsh_color) { a.dL_dsh_color[3 * z] = 0.f; a.dL_dsh_color[3 * z + 1] = 0.f; a.dL_dsh_color[3 * z + 2] = 0.f; }
        if (a.dL_dcolors) { a.dL_dcolors[3 * z] = 0.f; a.dL_dcolors[3 * z + 1] = 0.f; a.dL_dcolors[3 * z + 2] = 0.f; }
        for (int k = 0; k < a.num_extra; k++)
            if (a.dL_dextra[k]) { a.dL_dextra[k][3 * z] = 0.f; a.dL_dextra[k][3 * z + 1] = 0.f; a.dL_dextra[k][3 * z + 2] = 0.f; }
        if (a.dL_dcov3D) {
#pragma unroll
            for (int k = 0; k < 6; k++) a.dL_dcov3D[6 * z + k] = 0.f;
        }
        if (a.dL_dresidual_dx) { a.dL_dresidual_dx[3 * z] = 0.f; a.dL_dresidual_dx[3 * z + 1] = 0.f; a.dL_dresidual_dx[3 * z + 2] = 0.f; }
        if (a.dL_dresidual_dq) *(float4*)(a.dL_dresidual_dq + 4 * z) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (staged5) {
        // tile: [B x 3 means3D | B x 3 scales | B x 4 rotations | B opacities | B x 3 means2D] floats (B = K8_BLOCK): 14 of the SH tile's 26 KB at B = 256
        constexpr int B = K8_BLOCK, O_SC = 3 * B, O_ROT = 6 * B, O_OP = 10 * B, O_M2 = 11 * B;
        static_assert(14 * B * 4 <= (int)sizeof(float4) * K8_HALF * SH_ROW4, "the small-gradient tile must fit the SH staging tile");
        float* sf = reinterpret_cast<float*>(s_sh);
        const int t = threadIdx.x;
        if (in_range) {
            const int u = lrow;
            sf[3 * u] = o_dl[0]; sf[3 * u + 1] = o_dl[1]; sf[3 * u + 2] = o_dl[2];
            sf[O_SC + 3 * u] = o_ds[0]; sf[O_SC + 3 * u + 1] = o_ds[1]; sf[O_SC + 3 * u + 2] = o_ds[2];
            *reinterpret_cast<float4*>(sf + O_ROT + 4 * u) = make_float4(o_dq[0], o_dq[1], o_dq[2], o_dq[3]);
            sf[O_OP + u] = o_dop;
            sf[O_M2 + 3 * u] = gm2[0]; sf[O_M2 + 3 * u + 1] = gm2[1]; sf[O_M2 + 3 * u + 2] = 0.f;
        }
        if (!nat_vis) {
            sf[3 * t] = 0.f; sf[3 * t + 1] = 0.f; sf[3 * t + 2] = 0.f;
            sf[O_SC + 3 * t] = 0.f; sf[O_SC + 3 * t + 1] = 0.f; sf[O_SC + 3 * t + 2] = 0.f;
            *reinterpret_cast<float4*>(sf + O_ROT + 4 * t) = make_float4(0.f, 0.f, 0.f, 0.f);
            sf[O_OP + t] = 0.f;
            sf[O_M2 + 3 * t] = 0.f; sf[O_M2 + 3 * t + 1] = 0.f; sf[O_M2 + 3 * t + 2] = 0.f;
        }
        __syncthreads();
        const size_t b = (size_t)blockIdx.x * K8_BLOCK;
        const float4* s4 = reinterpret_cast<const float4*>(sf);
        // (a plain forwarder: calling store_f4_nt directly is harmless, but three v_mov of K8 then change places against profiles/preprocess_split_isa.txt)
        auto st4 = [](float4* p, float4 v) { store_f4_nt(p, v); };
        if (t < 3 * B / 4) {
            st4(reinterpret_cast<float4*>(a.dL_dmeans3D + 3 * b) + t, s4[t]);
            st4(reinterpret_cast<float4*>(a.dL_dscales + 3 * b) + t, s4[O_SC / 4 + t]);
            st4(reinterpret_cast<float4*>(a.dL_dmeans2D + 3 * b) + t, s4[O_M2 / 4 + t]);
        }
        st4(reinterpret_cast<float4*>(a.dL_drotations + 4 * b) + t, s4[O_ROT / 4 + t]);
        if (t < B / 4) st4(reinterpret_cast<float4*>(a.dL_dopacities + b) + t, s4[O_OP / 4 + t]);
    }
    if ((a.flags & EMD_FLAG_MOTION) && a.dL_dactor_pose) {
        if (a.pose_rows) {
            // EMD_FLAG_DETERMINISTIC: the point's own row, summed per actor in a pinned order afterwards (api.hip, segsum.h) -- no atomics
            if (a_id >= 0) {
                float4* pr = reinterpret_cast<float4*>(a.pose_rows + (size_t)i * EMD_ACTOR_STRIDE);
                pr[0] = make_float4(pose_g[0], pose_g[1], pose_g[2], pose_g[3]);
                pr[1] = make_float4(pose_g[4], pose_g[5], pose_g[6], pose_g[7]);
                pr[2] = make_float4(pose_g[8], pose_g[9], pose_g[10], pose_g[11]);
            }
        } else reduce_pose_grad(a_id, pose_g, a.dL_dactor_pose);
    }
}

// EMD_FLAG_DETERMINISTIC: destination of every point's pose row -- its actor when K8 stores one (visible and bound), else dropped by the sort
__global__ void __launch_bounds__(EMD_BLOCK) k_det_pose_keys(int N, const int32_t* __restrict__ radii, const int32_t* __restrict__ actor_id,
                                                             uint32_t* __restrict__ keys_in) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i >= N) return;
    const int a = actor_id[i];
    keys_in[i] = (radii[i] > 0 && a >= 0) ? (uint32_t)a : 0xFFFFFFFFu;
}

__global__ void __launch_bounds__(EMD_BLOCK) k_export_geometry(int N, const float4* rec, const uint2* binrec,
                                                               float* means2D, float* depths, float* conic_opacity,
                                                               float* rgb, float* normal, uint32_t* tiles_touched) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i >= N) return;
    const uint32_t tt = binrec[i].y >> 12;               // upstream's tiles touched (the enumerated rectangle may be smaller)
    const bool vis = tt != 0;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 r0 = vis ? rec[(size_t)i * EMD_REC_F4] : z, r1 = vis ? rec[(size_t)i * EMD_REC_F4 + 1] : z,
                 r2 = vis ? rec[(size_t)i * EMD_REC_F4 + 2] : z;
    if (means2D) { means2D[2 * i] = r0.x; means2D[2 * i + 1] = r0.y; }
    if (depths) depths[i] = r0.z;
    if (conic_opacity) *(float4*)(conic_opacity + 4 * i) = make_float4(r1.x, r1.y, r1.z, r0.w);
    if (rgb) { rgb[3 * i] = r2.x; rgb[3 * i + 1] = r2.y; rgb[3 * i + 2] = r2.z; }
    if (normal) { const float4 r3 = vis ? rec[(size_t)i * EMD_REC_F4 + 3] : z; normal[3 * i] = r3.x; normal[3 * i + 1] = r3.y; normal[3 * i + 2] = r3.z; }
    if (tiles_touched) tiles_touched[i] = tt;
}

}  // namespace

int emd_launch_preprocess(const PreArgs& a, int part, hipStream_t st) {
    if (a.N <= 0) return EMD_OK;
    const int nb = (a.N + PRE_BLOCK - 1) / PRE_BLOCK;
    const bool res = a.shs_res0 != nullptr;
    if (part == 1) hipLaunchKernelGGL(k_preprocess<1>, dim3(nb), dim3(PRE_BLOCK), 0, st, a);
    else if (part == 2 && res) hipLaunchKernelGGL((k_preprocess<2, true>), dim3(nb), dim3(PRE_BLOCK), 0, st, a);
    else if (part == 2) hipLaunchKernelGGL(k_preprocess<2>, dim3(nb), dim3(PRE_BLOCK), 0, st, a);
    else if (res) hipLaunchKernelGGL((k_preprocess<0, true>), dim3(nb), dim3(PRE_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(k_preprocess<0>, dim3(nb), dim3(PRE_BLOCK), 0, st, a);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_preprocess_backward(const PreBwdArgs& a, hipStream_t st) {
    if (a.N <= 0) return EMD_OK;
    const int nb = (a.N + K8_BLOCK - 1) / K8_BLOCK;
    if (a.shs_prezeroed) hipLaunchKernelGGL(k_preprocess_backward<true>, dim3(nb), dim3(K8_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(k_preprocess_backward<false>, dim3(nb), dim3(K8_BLOCK), 0, st, a);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_det_pose_keys(int N, const int32_t* radii, const int32_t* actor_id, uint32_t* keys_in, hipStream_t st) {
    if (N <= 0) return EMD_OK;
    hipLaunchKernelGGL(k_det_pose_keys, dim3((N + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, st, N, radii, actor_id, keys_in);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

// dL/d(SH colour) of every Gaussian, clamp-masked (0 when not visible): what K8 writes as dL_dsh_color, available as soon as the render
// backward has run -- accumulator row columns 7..9 and the clamp bits K1 left in row 2 of the record
__global__ void __launch_bounds__(EMD_BLOCK) k_sh_factor(int N, const int32_t* __restrict__ radii, const float4* __restrict__ rec,
                                                         const float* __restrict__ grad_rec, int stride, float* __restrict__ out) {
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (i >= N) return;
    float g[3] = {0.f, 0.f, 0.f};
    if (radii[i] > 0) {
        const float* r = grad_rec + (size_t)i * stride;
        const uint32_t bits = __float_as_uint(rec[(size_t)i * EMD_REC_F4 + 2].w);
        g[0] = (bits & 1u) ? 0.f : r[7]; g[1] = (bits & 2u) ? 0.f : r[8]; g[2] = (bits & 4u) ? 0.f : r[9];
    }
    out[3 * i] = g[0]; out[3 * i + 1] = g[1]; out[3 * i + 2] = g[2];
}

int emd_launch_sh_factor(int N, const int32_t* radii, const GeomWs& g, const float* grad_rec, int bwd_stride, float* dL_dsh_color, hipStream_t st) {
    if (N <= 0) return EMD_OK;
    hipLaunchKernelGGL(k_sh_factor, dim3((N + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, st, N, radii, g.rec, grad_rec, bwd_stride, dL_dsh_color);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

int emd_launch_export_geometry(int N, const GeomWs& g, float* means2D, float* depths, float* conic_opacity, float* rgb,
                               float* normal, uint32_t* tiles_touched, hipStream_t st) {
    if (N <= 0) return EMD_OK;
    hipLaunchKernelGGL(k_export_geometry, dim3((N + EMD_BLOCK - 1) / EMD_BLOCK), dim3(EMD_BLOCK), 0, st, N, g.rec,
                       g.binrec, means2D, depths, conic_opacity, rgb, normal, tiles_touched);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}
