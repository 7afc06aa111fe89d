// det_backward.h -- workspace of the deterministic backward (EMD_FLAG_DETERMINISTIC, EmdBwdArgs.det_ws): the contribution rows
// of the render backward and the pose rows of K8, each with the buffers of the reduction (det_reduce.h) that lists the rows per destination and adds
// each list; and the workspace of the stand-alone motion backward's deterministic form (emd_motion_backward_det, section 8.10), which is the pose half
// alone.  Included by api.hip alone; include/emd_raster.h states the size formulas.
#pragma once
#include "det_reduce.h"

struct DetWs {
    float* part;             // [4 * capacity][row pitch] contribution rows of the render backward: the survivor's own slot, as BinWs::surv lays them out
    DetSortWs r;             // n = 4 * capacity slots -> Gaussian ids
    uint32_t* counts;        // [16] device-side counts: [0] slots in use (4 D)  [1] contributions the render sort kept  [2] points the pose sort kept
    float* pose_rows;        // [N][EMD_ACTOR_STRIDE] pose gradient of every visible, actor-bound point (K8)
    DetSortWs p;             // n = N points -> actor ids
    size_t bytes;
};
static inline void emd_carve_det(void* base, int N, int64_t capacity, int num_extra, DetWs* w) {
    char* p = (char*)base;
    size_t off = 0;
    const size_t n = (size_t)(N > 0 ? N : 1), R = 4 * (size_t)(capacity > 0 ? capacity : 1);
    w->part = (float*)(p + off); off = emd_align_up(off + R * emd_bwd_stride(num_extra) * sizeof(float), 256);
    emd_carve_det_sort(p, off, R, EMD_BWD_PAYLOAD + 4 * num_extra, &w->r);
    w->counts = (uint32_t*)(p + off); off = emd_align_up(off + 64, 256);
    w->pose_rows = (float*)(p + off); off = emd_align_up(off + n * EMD_ACTOR_STRIDE * sizeof(float), 256);
    emd_carve_det_sort(p, off, n, EMD_ACTOR_STRIDE, &w->p);
    w->bytes = off + 256;
}

struct MotionDetWs {
    float* pose_rows;        // [n][EMD_ACTOR_STRIDE] pose gradient of every actor-bound point (k_motion_backward_det)
    DetSortWs p;             // n points -> actor ids
    uint32_t* counts;        // [16] device-side counts: [0] points the sort kept
    size_t bytes;
};
static inline void emd_carve_motion_det(void* base, int64_t n_points, MotionDetWs* w) {
    char* p = (char*)base;
    size_t off = 0;
    const size_t n = (size_t)(n_points > 0 ? n_points : 1);
    w->pose_rows = (float*)(p + off); off = emd_align_up(off + n * EMD_ACTOR_STRIDE * sizeof(float), 256);
    emd_carve_det_sort(p, off, n, EMD_ACTOR_STRIDE, &w->p);
    w->counts = (uint32_t*)(p + off); off = emd_align_up(off + 64, 256);
    w->bytes = off + 256;
}
