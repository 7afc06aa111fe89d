// hexplane_det.h -- workspace and launcher of the deterministic HexPlane backward (EMD_HEX_FLAG_DETERMINISTIC, EmdHexGrads.det_ws; DESIGN.md section
// 8.9; hexplane_det.hip): the [4 N][C] contribution rows of ONE plane with the buffers of the reduction (det_reduce.h) that lists them per texel and
// adds each list, reused from plane to plane, and the per-point time column with its one-run sum.
// include/emd_raster.h states the size formula.
#pragma once
#include "det_reduce.h"

struct HexDetWs : DetUnitWs {   // r: the [4 N][C] rows of the plane in flight (slot e = k N + n holds tap k of point n) and the sort of the slots by texel
                                // counts: [0] slots the sort kept (= 4 N: every slot has a texel)
    float* tcol;             // [N] dL/dtimes of every point, when only its sum is asked for (EmdHexGrads.dL_dtime_sum)
    uint32_t *tkeys, *tslots;   // [N] each: one run under key 0, slots 0 .. N - 1
    double* tpartials;       // chunk sums of that run
};
static inline void emd_carve_hex_det(void* base, int64_t N, int C, HexDetWs* w) {
    char* p = (char*)base;
    const size_t n = (size_t)(N > 0 ? N : 1);
    size_t off = emd_carve_det_unit(base, 4 * n, C, C, w);
    w->tcol = (float*)(p + off); off = emd_align_up(off + n * 4, 256);
    w->tkeys = (uint32_t*)(p + off); off = emd_align_up(off + n * 4, 256);
    w->tslots = (uint32_t*)(p + off); off = emd_align_up(off + n * 4, 256);
    w->tpartials = (double*)(p + off); off = emd_align_up(off + emd_segsum_partial_bytes(n, 1), 256);
    w->bytes = off + 256;
}
// plane p of scale s spans axes (A_[p], B_[p]): its W x H texels are the destination ids of its sort
static inline int64_t emd_hex_plane_texels(const EmdHexArgs* a, int s, int p) {
    const int A_[6] = {0, 0, 0, 1, 1, 2}, B_[6] = {1, 2, 3, 2, 3, 3};
    return (int64_t)a->res[s][A_[p]] * a->res[s][B_[p]];
}

// the branch of emd_hexplane_backward behind EMD_HEX_FLAG_DETERMINISTIC (args already through check_hex, num_points > 0)
int emd_hexplane_backward_det(const EmdHexArgs* a, const EmdHexGrads* g, hipStream_t st);
