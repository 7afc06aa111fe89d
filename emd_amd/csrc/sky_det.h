// sky_det.h -- workspace of the deterministic sky backward (emd_sky_backward_det, sky_det.hip): the [4 P] float4 contribution
// rows of a call's P pixels (slot e = k P + p holds tap k of pixel p) with the buffers of the reduction (det_reduce.h) that lists them per texel and
// adds each list.  include/emd_raster.h states the size formula.
#pragma once
#include "det_reduce.h"

#define EMD_SKY_DET_ROW_PITCH 4      // floats per row: the three channels and a pad, so that a row is one 16-byte store

struct SkyDetWs {
    float* rows;             // [4 P][4]
    DetSortWs r;             // n = 4 P slots -> texels
    uint32_t* counts;        // [16] device-side counts: [0] slots the sort kept
    size_t bytes;
};
static inline void emd_carve_sky_det(void* base, int64_t P, SkyDetWs* w) {
    char* p = (char*)base;
    size_t off = 0;
    const size_t n = 4 * (size_t)(P > 0 ? P : 1);
    w->rows = (float*)(p + off); off = emd_align_up(off + n * EMD_SKY_DET_ROW_PITCH * sizeof(float), 256);
    emd_carve_det_sort(p, off, n, 3, &w->r);
    w->counts = (uint32_t*)(p + off); off = emd_align_up(off + 64, 256);
    w->bytes = off + 256;
}
// the slots are numbered in 32 bits, and the sort rounds its launch up to whole tiles
static inline bool emd_det_slots_fit(int64_t slots) { return slots >= 0 && slots <= (int64_t)0xFFFFFFFFu - EMD_SORT_TILE; }

// the argument checks of emd_sky_backward (sky.hip), shared with emd_sky_backward_det
int emd_sky_backward_checks(const EmdSkyBwdArgs* b, const char* who);
