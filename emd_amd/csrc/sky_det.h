// sky_det.h -- workspace of the deterministic sky backward (emd_sky_backward_det, sky_det.hip): one reduction and its counts
// (DetUnitWs, det_reduce.h) over the [4 P] float4 contribution rows of a call's P pixels (slot e = k P + p holds tap k of pixel p), listed per texel.
// include/emd_raster.h states the size formula.
#pragma once
#include "det_reduce.h"

#define EMD_SKY_DET_ROW_PITCH 4      // floats per row: the three channels and a pad, so that a row is one 16-byte store

static inline void emd_carve_sky_det(void* base, int64_t P, DetUnitWs* w) { emd_carve_det_unit(base, 4 * (size_t)(P > 0 ? P : 1), EMD_SKY_DET_ROW_PITCH, 3, w); }

// the argument checks of emd_sky_backward (sky.hip), shared with emd_sky_backward_det
int emd_sky_backward_checks(const EmdSkyBwdArgs* b, const char* who);
