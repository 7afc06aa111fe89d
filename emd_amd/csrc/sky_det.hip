// sky_det.hip -- the deterministic sky cube-map backward (emd_sky_backward_det; contract: include/emd_raster.h).  gfx950.
// The default backward (sky.hip) adds every tap's weighted colour gradient to its texel through fp64 LDS windows and global float atomics, in
// whatever order the workgroups run.  Here every contribution is STORED once, a stable sort lists the contributions per texel in a fixed order, and
// the segmented row sum adds each list with its pinned association (segsum.h) -- the construction of the deterministic render backward (section 8.8):
//   k_sky_det_rows           lane = pixel: dL_dfg / dL_dacc as the default kernel writes them (the same text: sky_taps.h and sky_pixel_bwd_body.inc,
//                            which k_sky_backward includes too), the four weighted rows to slots k P + p, the texels as keys (0xFFFFFFFF: not
//                            sampled, or a tap of weight zero)
//   emd_det_sort_and_sum     (det_reduce.h) the compacting, stable sort: slots per texel in ascending slot order = ascending (tap, pixel);
//                            the segmented row sum -> dL_dcube
// No atomics and no device-scope fences anywhere.
#include <string.h>

#include "sky_det.h"
#include "sky_taps.h"

namespace {

// Flat indexing: the 16 x 16 tiles of k_sky_backward serve its LDS window alone.  rows == NULL: no cube-map gradient is asked for.
__global__ void __launch_bounds__(EMD_BLOCK) k_sky_det_rows(EmdSkyBwdArgs b, float4* __restrict__ rows, uint32_t* __restrict__ keys_in) {
    const EmdSkyArgs& a = b.f;
    const size_t P = (size_t)a.height * a.width;
    const size_t p = (size_t)blockIdx.x * EMD_BLOCK + threadIdx.x;
    const bool valid = p < P;
    const int px = (int)(p % (size_t)a.width), py = (int)(p / (size_t)a.width);
    const int res = a.resolution;
#include "sky_pixel_bwd_body.inc"
    if (!rows || !valid) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const size_t e = (size_t)k * P + p;
        // a row whose gs is all zero stays a contribution; a tap of weight zero (a cube corner's missing fourth tap) is none, as in k_sky_backward
        const bool kept = sampled && tp.w[k] != 0.f;
        if (kept) rows[e] = make_float4(tp.w[k] * gs[0], tp.w[k] * gs[1], tp.w[k] * gs[2], 0.f);
        keys_in[e] = kept ? tp.idx[k] : 0xFFFFFFFFu;
    }
}

int64_t sky_texels(int32_t res) { return (int64_t)6 * res * res; }
// sizes the mode serves: 4 P slots in 32 bits, the texel ids in the int the sort's pass count is computed from
int check_sizes(int64_t P, int32_t res, const char* who) {
    if (P < 0 || !emd_det_slots_fit(4 * P)) { emd_set_error("%s: the deterministic mode numbers 4 P slots in 32 bits (P = %lld)", who, (long long)P); return EMD_ERR_INVALID; }
    if (res <= 0 || sky_texels(res) > ((int64_t)1 << 30)) { emd_set_error("%s: resolution %d is not in 1 .. 13377", who, res); return EMD_ERR_INVALID; }
    return EMD_OK;
}

}  // namespace

extern "C" size_t emd_sky_det_workspace_size(int64_t num_pixels) {
    if (num_pixels < 0 || !emd_det_slots_fit(4 * num_pixels)) return 0;
    DetUnitWs w;
    emd_carve_sky_det(nullptr, num_pixels, &w);
    return w.bytes;
}

extern "C" int emd_sky_det_workspace_offsets(int64_t num_pixels, int32_t resolution, size_t out[6]) {
    if (!out) { emd_set_error("sky_det_workspace_offsets: null argument"); return EMD_ERR_INVALID; }
    const int rc = check_sizes(num_pixels, resolution, "sky_det_workspace_offsets");
    if (rc) return rc;
    DetUnitWs w;
    emd_carve_sky_det(nullptr, num_pixels, &w);
    emd_det_unit_offsets(w, sky_texels(resolution), out);
    return EMD_OK;
}

extern "C" int emd_sky_backward_det(const EmdSkyBwdArgs* b, void* det_ws, size_t det_bytes, void* hip_stream) {
    int rc = emd_sky_backward_checks(b, "sky_backward_det");
    if (rc) return rc;
    // everything is decided here, before the first launch
    const int64_t P = (int64_t)b->f.height * b->f.width;
    rc = check_sizes(P, b->f.resolution, "sky_backward_det");
    if (rc) return rc;
    DetUnitWs w;
    memset(&w, 0, sizeof(w));
    if (b->dL_dcube) {
        emd_carve_sky_det(det_ws, P, &w);
        rc = emd_det_check_ws("sky_backward_det", det_ws, det_bytes, w.bytes, 256, EMD_ERR_WORKSPACE, "emd_sky_det_workspace_size");
        if (rc) return rc;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int64_t texels = sky_texels(b->f.resolution);
    if (b->dL_dcube) { rc = emd_zero_async(b->dL_dcube, (size_t)texels * 3 * sizeof(float), st); if (rc) return rc; }
    hipLaunchKernelGGL(k_sky_det_rows, dim3((unsigned)(((size_t)P + EMD_BLOCK - 1) / EMD_BLOCK)), dim3(EMD_BLOCK), 0, st, *b, (float4*)w.r.rows, w.r.s.keys_in);
    EMD_LAUNCH_CHECK();
    if (!b->dL_dcube) return EMD_OK;
    return emd_det_sort_and_sum(w.r, texels, nullptr, w.counts, b->dL_dcube, 3, st);
}
