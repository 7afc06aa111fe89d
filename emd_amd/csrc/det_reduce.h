// det_reduce.h -- the deterministic reduction: a stable compacting sort of destination ids (radix_sort.h) followed by the segmented row sum of each list
// (segsum.h), with the workspace of one such reduction.  Users: the deterministic backward of the rasterizer (det_backward.h, api.hip; DESIGN.md section
// 8.8) and of the HexPlane (hexplane_det.h, hexplane_det.hip; section 8.9).  Host code only.
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
static inline void emd_carve_det_sort(char* p, size_t& off, size_t n, int width, DetSortWs* w) {
    w->keys_in = (uint32_t*)(p + off); off = emd_align_up(off + n * 4, 256);
    for (int i = 0; i < 2; i++) { w->keys[i] = (uint32_t*)(p + off); off = emd_align_up(off + n * 4, 256); }
    for (int i = 0; i < 2; i++) { w->vals[i] = (uint32_t*)(p + off); off = emd_align_up(off + n * 4, 256); }
    w->hist = (uint32_t*)(p + off); off = emd_align_up(off + (n + EMD_SORT_TILE - 1) / EMD_SORT_TILE * EMD_DEPTH_BINS_MAX * 4, 256);
    w->partials = (double*)(p + off); off = emd_align_up(off + emd_segsum_partial_bytes(n, width), 256);
}

// One deterministic reduction.  The caller's key-build launch left every row's destination id in w.keys_in (0xFFFFFFFF: no contribution): a
// stable compacting sort lists the rows per destination -- in ascending row order inside a destination, a function of the bit-exact forward alone -- and
// every list is summed in the pinned order (segsum.h) into out[destination].  *count_out: the rows the sort kept, on the device.
static inline int emd_det_sort_and_sum(const DetSortWs& w, size_t n_cap, int64_t n_ids, const uint32_t* n_dev_in, uint32_t* count_out, const float* rows, int row_pitch,
                                       int width, float* out, int out_pitch, hipStream_t st) {
    RadixSortArgs rs;
    rs.keys_in = w.keys_in;
    for (int i = 0; i < 2; i++) { rs.keys[i] = w.keys[i]; rs.vals[i] = w.vals[i]; }
    rs.hist = w.hist; rs.n_cap = n_cap; rs.n_dev = n_dev_in;
    rs.passes = emd_det_sort_passes(n_ids); rs.bits = emd_det_sort_bits(n_ids);
    rs.count_out = count_out;
    const int buf = emd_launch_radix_sort(rs, st);
    if (buf < 0) return buf;
    SegSumArgs ss;
    ss.keys = w.keys[buf]; ss.slots = w.vals[buf]; ss.n_dev = count_out; ss.n_cap = n_cap;
    ss.rows = rows; ss.row_pitch = row_pitch; ss.width = width;
    ss.out = out; ss.out_pitch = out_pitch; ss.partials = w.partials;
    return emd_launch_segmented_row_sum(ss, st);
}
