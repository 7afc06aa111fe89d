// sky.hip -- sky cube-map lookup + final blend, forward and backward.
//
// Replaces, for the two call sites of the reference,
//   S3Gaussian/scene/sky_cubemap.py:41-87 + gaussian_renderer/__init__.py:299-301   (rays, mask, dr.texture, clamp, blend)
//   OmniRe/models/modules.py:174-208 + models/trainers/base.py:491-497              (dr.texture on view directions, blend)
// the chain get_rays_torch (7 element-wise / matmul launches over H*W*3) -> boolean-mask gather -> nvdiffrast
// `dr.texture(..., filter_mode='linear', boundary_mode='cube')` (CUDA-only) -> masked scatter -> permute -> clamp -> blend
// by ONE kernel per direction of the pass: a lane owns a pixel, builds its ray from the pinhole parameters in registers,
// selects the cube face (OpenGL convention), gathers the four bilinear taps (taps that leave the face are fetched from
// the adjacent face; at a cube corner the missing fourth tap is dropped and the other three renormalised), clamps and
// blends.  The backward recomputes the taps (cheaper than storing 4 indices + 4 weights per pixel) and scatters
// dL/dtexel with float atomics; dL/d(foreground) and dL/d(opacity) of the blend come out of the same kernel.
// HBM-bound by construction: 3 planar image reads/writes per pixel + 4 x 12 B texel gathers that hit L2.
// The lookup restates the published nvdiffrast algorithm (oracle/sky_oracle.py; PARITY UNPINNED for that part).
// The ray and tap arithmetic is sky_taps.h and the per-pixel half of the backward is sky_pixel_bwd_body.inc; the opt-in deterministic backward, which
// shares both and uses no atomics, is sky_det.hip.
#include "common.h"
#include "device_utils.h"
#include "sky_det.h"
#include "sky_taps.h"

namespace {

__global__ void __launch_bounds__(EMD_BLOCK) k_sky_forward(EmdSkyArgs a) {
    const size_t P = (size_t)a.height * a.width;
    const size_t p = (size_t)blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (p >= P) return;
    const float acc = a.acc ? a.acc[p] : 0.f;
    const bool sampled = !(a.acc && a.mask_threshold >= 0.f) || (1.f - acc) > a.mask_threshold;
    float s[3] = {a.fill, a.fill, a.fill};
    if (sampled) {
        float dx, dy, dz;
        pixel_ray(a, (int)(p % (size_t)a.width), (int)(p / (size_t)a.width), p, dx, dy, dz);
        Tap tp;
        cube_taps(dx, dy, dz, a.resolution, tp);
        s[0] = s[1] = s[2] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float* t = a.cube + (size_t)tp.idx[k] * 3;
            s[0] += tp.w[k] * t[0]; s[1] += tp.w[k] * t[1]; s[2] += tp.w[k] * t[2];
        }
    }
    if (a.flags & EMD_SKY_CLAMP01) {
#pragma unroll
        for (int c = 0; c < 3; c++) s[c] = fminf(fmaxf(s[c], 0.f), 1.f);
    }
    if (a.sky) {
        if (a.flags & EMD_SKY_INTERLEAVED) { a.sky[3 * p] = s[0]; a.sky[3 * p + 1] = s[1]; a.sky[3 * p + 2] = s[2]; }
        else { a.sky[p] = s[0]; a.sky[P + p] = s[1]; a.sky[2 * P + p] = s[2]; }
    }
    if (a.out && a.fg) {
        const bool il = (a.flags & EMD_SKY_INTERLEAVED) != 0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const size_t q = il ? 3 * p + c : (size_t)c * P + p;
            const float f = a.fg[q];
            a.out[q] = (a.flags & EMD_SKY_BLEND_S3G) ? f * acc + s[c] * (1.f - acc) : f + s[c] * (1.f - acc);
        }
    }
}

// Texel gradients are combined per workgroup before they touch memory.  A workgroup owns a 16 x 16 pixel tile, whose
// bilinear taps fall on a few dozen texels when the map is magnified (1024^2 faces under a 1700-px focal length: ~7
// pixels per texel); issued one by one, that many float atomics to the same address serialise in L2 (measured
// 1.17 ms for a 1066 x 1600 view).  The tile's taps lie in a small window of one face, so the workgroup accumulates into
// an LDS window of SKY_WIN x SKY_WIN texels anchored at the tap of its first pixel (plain ds_add_f32, no hashing); taps
// outside the window or on another face (tiles that straddle a cube edge, heavily minified maps) go straight to the
// global atomic.  One global atomic per touched texel and channel leaves the workgroup.
#define SKY_WIN 24
__global__ void __launch_bounds__(EMD_BLOCK) k_sky_backward(EmdSkyBwdArgs b) {
    // fp64 cells: ds_add_f64 is the native LDS float add that runs at rate on gfx950 (8.9 clocks per wave64 instruction; ds_add_f32, which a plain
    // atomicAdd on a __shared__ float compiles to, takes 193: profiles/r03_lds_atomic_microbench.txt -- twelve of them per pixel were this kernel)
    __shared__ double s_val[SKY_WIN * SKY_WIN * 3];
    __shared__ int s_org[3];     // face, u0, v0 of the window
    const EmdSkyArgs& a = b.f;
    for (int i = threadIdx.x; i < SKY_WIN * SKY_WIN * 3; i += EMD_BLOCK) s_val[i] = 0.0;
    const size_t P = (size_t)a.height * a.width;
    const int res = a.resolution;
    size_t p;
    int px, py;
    bool valid;
    if (a.height > 1) {        // 16 x 16 pixel tiles: neighbouring pixels share texels
        const int tiles_x = (a.width + 15) / 16;
        px = (int)(blockIdx.x % (unsigned)tiles_x) * 16 + (int)(threadIdx.x & 15);
        py = (int)(blockIdx.x / (unsigned)tiles_x) * 16 + (int)(threadIdx.x >> 4);
        valid = px < a.width && py < a.height;
        p = (size_t)py * a.width + px;
    } else {
        p = (size_t)blockIdx.x * EMD_BLOCK + threadIdx.x;
        valid = p < P;
        px = (int)p; py = 0;
    }
#include "sky_pixel_bwd_body.inc"
    if (!b.dL_dcube) return;
    // window origin: centred on the first tap of the lowest contributing lane of the workgroup
    __shared__ int s_leader;
    if (threadIdx.x == 0) s_leader = EMD_BLOCK;
    __syncthreads();                                  // also: s_val is cleared
    const bool contributes = valid && sampled && (gs[0] != 0.f || gs[1] != 0.f || gs[2] != 0.f);
    if (contributes) atomicMin(&s_leader, (int)threadIdx.x);
    __syncthreads();
    if (s_leader == EMD_BLOCK) return;                // nothing to scatter (uniform)
    if ((int)threadIdx.x == s_leader) {
        const uint32_t t0 = tp.idx[0];
        const int f = (int)(t0 / (uint32_t)(res * res)), r = (int)(t0 % (uint32_t)(res * res));
        s_org[0] = f; s_org[1] = r % res - SKY_WIN / 2; s_org[2] = r / res - SKY_WIN / 2;
    }
    __syncthreads();
    const int of = s_org[0], ou = s_org[1], ov = s_org[2];
    if (contributes) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (tp.w[k] == 0.f) continue;
            const uint32_t key = tp.idx[k];
            const int f = (int)(key / (uint32_t)(res * res)), r = (int)(key % (uint32_t)(res * res));
            const int wu = r % res - ou, wv = r / res - ov;
            const bool in_win = f == of && wu >= 0 && wu < SKY_WIN && wv >= 0 && wv < SKY_WIN;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if (gs[c] == 0.f) continue;
                if (in_win) lds_add_f64(&s_val[(wv * SKY_WIN + wu) * 3 + c], tp.w[k] * gs[c]);
                else atomicAdd(b.dL_dcube + (size_t)key * 3 + c, tp.w[k] * gs[c]);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SKY_WIN * SKY_WIN * 3; i += EMD_BLOCK) {
        const float v = (float)s_val[i];
        if (v == 0.f) continue;
        const int t = i / 3, wu = t % SKY_WIN + ou, wv = t / SKY_WIN + ov;
        if (wu < 0 || wu >= res || wv < 0 || wv >= res) continue;     // never written: in_win implies a real texel
        atomicAdd(b.dL_dcube + ((size_t)(of * res + wv) * res + wu) * 3 + (i % 3), v);
    }
}

int check_sky(const EmdSkyArgs* a, const char* who) {
    if (!a) { emd_set_error("%s: null args", who); return EMD_ERR_INVALID; }
    if (a->height <= 0 || a->width <= 0 || a->resolution <= 0) { emd_set_error("%s: bad sizes H=%d W=%d res=%d", who, a->height, a->width, a->resolution); return EMD_ERR_INVALID; }
    if (!a->cube) { emd_set_error("%s: cube must not be null", who); return EMD_ERR_INVALID; }
    if ((a->flags & EMD_SKY_BLEND_S3G) && (a->flags & EMD_SKY_BLEND_ADD)) { emd_set_error("%s: choose one blend mode", who); return EMD_ERR_INVALID; }
    if (a->out && (!a->fg || !a->acc || !(a->flags & (EMD_SKY_BLEND_S3G | EMD_SKY_BLEND_ADD)))) { emd_set_error("%s: blend output needs fg, acc and a blend mode", who); return EMD_ERR_INVALID; }
    return EMD_OK;
}

}  // namespace

extern "C" int emd_sky_forward(const EmdSkyArgs* a, void* hip_stream) {
    int rc = check_sky(a, "sky_forward");
    if (rc) return rc;
    if (!a->sky && !a->out) { emd_set_error("sky_forward: no output requested"); return EMD_ERR_INVALID; }
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t P = (size_t)a->height * a->width;
    hipLaunchKernelGGL(k_sky_forward, dim3((unsigned)((P + EMD_BLOCK - 1) / EMD_BLOCK)), dim3(EMD_BLOCK), 0, st, *a);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

// the argument checks of the backward, for both of its entries (emd_sky_backward_det: sky_det.hip)
int emd_sky_backward_checks(const EmdSkyBwdArgs* b, const char* who) {
    if (!b) { emd_set_error("%s: null args", who); return EMD_ERR_INVALID; }
    int rc = check_sky(&b->f, who);
    if (rc) return rc;
    if (!b->dL_dout && !b->dL_dsky) { emd_set_error("%s: no incoming gradient", who); return EMD_ERR_INVALID; }
    return EMD_OK;
}

extern "C" int emd_sky_backward(const EmdSkyBwdArgs* b, void* hip_stream) {
    int rc = emd_sky_backward_checks(b, "sky_backward");
    if (rc) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t P = (size_t)b->f.height * b->f.width;
    if (b->dL_dcube)
        { int zrc = emd_zero_async(b->dL_dcube, (size_t)6 * b->f.resolution * b->f.resolution * 3 * sizeof(float), st); if (zrc) return zrc; }
    const unsigned grid = b->f.height > 1 ? (unsigned)(((b->f.width + 15) / 16) * ((b->f.height + 15) / 16))
                                          : (unsigned)((P + EMD_BLOCK - 1) / EMD_BLOCK);
    hipLaunchKernelGGL(k_sky_backward, dim3(grid), dim3(EMD_BLOCK), 0, st, *b);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}
