// det_backward.h -- workspace of the deterministic backward (EMD_FLAG_DETERMINISTIC, EmdBwdArgs.det_ws): the contribution rows
// of the render backward and the pose rows of K8, each with the buffers of the stable sort (radix_sort.h) that lists the rows per destination and of
// the segmented row sum (segsum.h) that adds each list.  Included by api.hip alone; include/emd_raster.h states the size formula.
#pragma once
#include "radix_sort.h"
#include "segsum.h"

// A sort of n destination ids: ceil(log2 n) key bits in passes of at most nine.
static inline int emd_det_sort_passes(int64_t n_ids) { const int b = emd_tile_bits((int)(n_ids > 1 ? n_ids : 2)); return (b + 8) / 9; }
static inline int emd_det_sort_bits(int64_t n_ids) { const int b = emd_tile_bits((int)(n_ids > 1 ? n_ids : 2)), p = emd_det_sort_passes(n_ids); return (b + p - 1) / p; }
struct DetSortWs {
    uint32_t* keys_in;       // [n] raw destination ids, 0xFFFFFFFF = no contribution (dropped by the compacting first pass)
    uint32_t *keys[2], *vals[2];   // [n] ping-pong of the stable sort: destination id, and the slot / point index it came from
    uint32_t* hist;          // [512][ceil(n / EMD_SORT_TILE)]
    double* partials;        // chunk sums of the segmented row sum (segsum.h)
};
struct DetWs {
    float* part;             // [4 * capacity][row pitch] contribution rows of the render backward: the survivor's own slot, as BinWs::surv lays them out
    DetSortWs r;             // n = 4 * capacity slots -> Gaussian ids
    uint32_t* counts;        // [16] device-side counts: [0] slots in use (4 D)  [1] contributions the render sort kept  [2] points the pose sort kept
    float* pose_rows;        // [N][EMD_ACTOR_STRIDE] pose gradient of every visible, actor-bound point (K8)
    DetSortWs p;             // n = N points -> actor ids
    size_t bytes;
};
static inline void emd_carve_det_sort(char* p, size_t& off, size_t n, int width, DetSortWs* w) {
    w->keys_in = (uint32_t*)(p + off); off = emd_align_up(off + n * 4, 256);
    for (int i = 0; i < 2; i++) { w->keys[i] = (uint32_t*)(p + off); off = emd_align_up(off + n * 4, 256); }
    for (int i = 0; i < 2; i++) { w->vals[i] = (uint32_t*)(p + off); off = emd_align_up(off + n * 4, 256); }
    w->hist = (uint32_t*)(p + off); off = emd_align_up(off + (n + EMD_SORT_TILE - 1) / EMD_SORT_TILE * EMD_DEPTH_BINS_MAX * 4, 256);
    w->partials = (double*)(p + off); off = emd_align_up(off + emd_segsum_partial_bytes(n, width), 256);
}
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
