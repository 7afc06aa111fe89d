// det_backward.h -- workspace of the deterministic backward (EMD_FLAG_DETERMINISTIC, EmdBwdArgs.det_ws): two reductions
// (det_reduce.h) and the counts.  Included by api.hip alone; include/emd_raster.h states the size formula.
#pragma once
#include "det_reduce.h"

struct DetWs : DetUnitWs {   // r: the [4 * capacity][row pitch] contribution rows of the render backward -- the survivor's own slot, as BinWs::surv lays
                             //    them out -- and the sort of the slots by Gaussian id
                             // counts: [0] slots in use (4 D)  [1] contributions the render sort kept  [2] points the pose sort kept
    DetReduction p;          // the [N][EMD_ACTOR_STRIDE] pose gradient of every visible, actor-bound point (K8) and the sort of the points by actor id
};
static inline void emd_carve_det(void* base, int N, int64_t capacity, int num_extra, DetWs* w) {
    size_t off = emd_carve_det_unit(base, 4 * (size_t)(capacity > 0 ? capacity : 1), emd_bwd_stride(num_extra), EMD_BWD_PAYLOAD + 4 * num_extra, w);
    emd_carve_det_reduction((char*)base, off, (size_t)(N > 0 ? N : 1), EMD_ACTOR_STRIDE, EMD_ACTOR_STRIDE, &w->p);
    w->bytes = off + 256;
}
