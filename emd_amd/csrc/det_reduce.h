// det_reduce.h -- the deterministic reduction: a stable compacting sort of destination ids (radix_sort.h) followed by the segmented row sum of each list
// (segsum.h), with everything its users share: the workspace of one reduction (rows + sort), its counts, the size bounds, the workspace check and the
// offsets report.  Users: the deterministic backward of the rasterizer (det_backward.h, api.hip), of the HexPlane
// (hexplane_det.h/.hip; section 8.9), of the sky cube map and the stand-alone motion backward (sky_det.h/.hip, api.hip; section 8.10), and the per-actor
// row sum of the actor chain (track_det.hip; section 8.15).  Host code only.
#pragma once
#include "radix_sort.h"
#include "segsum.h"

// A sort of n destination ids: ceil(log2 n) key bits in passes of at most nine.
static inline int emd_det_sort_passes(int64_t n_ids) { const int b = emd_tile_bits((int)(n_ids > 1 ? n_ids : 2)); return (b + 8) / 9; }
static inline int emd_det_sort_bits(int64_t n_ids) { const int b = emd_tile_bits((int)(n_ids > 1 ? n_ids : 2)), p = emd_det_sort_passes(n_ids); return (b + p - 1) / p; }
// which of keys[] / vals[] holds the sorted lists after a sort of n_ids destination ids
static inline int emd_det_sorted_buf(int64_t n_ids) { return emd_radix_result_buf(true, emd_det_sort_passes(n_ids)); }
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

// The rows of one reduction and its sort: rows, then the sort, each rounded up to 256 bytes.
struct DetReduction {
    float* rows;             // [n][pitch] contribution rows: the first `width` floats of a row are summed
    DetSortWs s;             // n rows -> destination ids
    size_t n;
    int pitch, width;
};
static inline void emd_carve_det_reduction(char* p, size_t& off, size_t n, int pitch, int width, DetReduction* r) {
    r->n = n; r->pitch = pitch; r->width = width;
    r->rows = (float*)(p + off); off = emd_align_up(off + n * (size_t)pitch * sizeof(float), 256);
    emd_carve_det_sort(p, off, n, width, &r->s);
}
// [16] device-side counts of a workspace: what its sorts kept
static inline uint32_t* emd_carve_det_counts(char* p, size_t& off) { uint32_t* c = (uint32_t*)(p + off); off = emd_align_up(off + 64, 256); return c; }

// A workspace that starts with one reduction and the counts: the whole workspace of the sky and motion entries, the head of the rasterizer's and the
// HexPlane's.  -> the offset behind the counts, where such a user goes on carving (it then sets `bytes` again: 256 spare bytes close every workspace).
struct DetUnitWs {
    DetReduction r;
    uint32_t* counts;        // [0] rows the sort of r kept
    size_t bytes;
};
static inline size_t emd_carve_det_unit(void* base, size_t n, int pitch, int width, DetUnitWs* w) {
    size_t off = 0;
    emd_carve_det_reduction((char*)base, off, n, pitch, width, &w->r);
    w->counts = emd_carve_det_counts((char*)base, off);
    w->bytes = off + 256;
    return off;
}

// The size bounds.  Slots are numbered in 32 bits, and the sort rounds its launch up to whole tiles ...
static inline bool emd_det_slots_fit(int64_t slots) { return slots >= 0 && slots <= (int64_t)0xFFFFFFFFu - EMD_SORT_TILE; }
// ... the HexPlane's four taps of a point each leave room for a tile ...
static inline bool emd_det_hex_points_fit(int64_t num_points) { return num_points < ((int64_t)1 << 30) - EMD_SORT_TILE; }
// ... and the actor chain numbers its points in an int.
static inline bool emd_det_track_points_fit(int64_t n) { return n >= 0 && n <= (int64_t)0x7FFFFFFF - EMD_SORT_TILE; }

// A missing or short workspace is EMD_ERR_WORKSPACE; one at an address that is no multiple of `align` is `misaligned_rc`.  size_fn: the entry that
// reports `need`.
static inline int emd_det_check_ws(const char* who, const void* ws, size_t have, size_t need, unsigned align, int misaligned_rc, const char* size_fn) {
    const bool small = !ws || have < need;
    if (!small && !((uintptr_t)ws & (align - 1))) return EMD_OK;
    emd_set_error("%s: needs a %u-byte aligned det_ws of %zu bytes (%s), got %zu at %p", who, align, need, size_fn, ws ? have : (size_t)0, ws);
    return small ? EMD_ERR_WORKSPACE : misaligned_rc;
}

// The offsets reports describe a workspace carved at address 0.
static inline size_t emd_det_offset(const void* p) { return (size_t)(uintptr_t)p; }
// the six words of the sky and motion entries: rows, raw keys, sorted keys, sorted slots, counts, bytes
static inline void emd_det_unit_offsets(const DetUnitWs& w, int64_t n_ids, size_t out[6]) {
    const int buf = emd_det_sorted_buf(n_ids);
    out[0] = emd_det_offset(w.r.rows); out[1] = emd_det_offset(w.r.s.keys_in); out[2] = emd_det_offset(w.r.s.keys[buf]);
    out[3] = emd_det_offset(w.r.s.vals[buf]); out[4] = emd_det_offset(w.counts); out[5] = w.bytes;
}

// One deterministic reduction.  The caller's key-build launch left every row's destination id in r.s.keys_in (0xFFFFFFFF: no contribution): a
// stable compacting sort lists the rows per destination -- in ascending row order inside a destination, a function of the bit-exact forward alone -- and
// every list is summed in the pinned order (segsum.h) into out[destination].  *count_out: the rows the sort kept, on the device.
static inline int emd_det_sort_and_sum(const DetReduction& r, int64_t n_ids, const uint32_t* n_dev_in, uint32_t* count_out, float* out, int out_pitch, hipStream_t st) {
    const DetSortWs& w = r.s;
    RadixSortArgs rs;
    rs.keys_in = w.keys_in;
    for (int i = 0; i < 2; i++) { rs.keys[i] = w.keys[i]; rs.vals[i] = w.vals[i]; }
    rs.hist = w.hist; rs.n_cap = r.n; rs.n_dev = n_dev_in;
    rs.passes = emd_det_sort_passes(n_ids); rs.bits = emd_det_sort_bits(n_ids);
    rs.count_out = count_out;
    const int buf = emd_launch_radix_sort(rs, st);
    if (buf < 0) return buf;
    SegSumArgs ss;
    ss.keys = w.keys[buf]; ss.slots = w.vals[buf]; ss.n_dev = count_out; ss.n_cap = r.n;
    ss.rows = r.rows; ss.row_pitch = r.pitch; ss.width = r.width;
    ss.out = out; ss.out_pitch = out_pitch; ss.partials = w.partials;
    return emd_launch_segmented_row_sum(ss, st);
}
