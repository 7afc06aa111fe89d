// radix_sort.h -- stable LSD radix sort of (32-bit key, 32-bit value) pairs on the device (radix_sort.hip).
// Callers: the depth sort and the tile sort of the binning stage (binning.hip), the Z-order sort and the reverse lists of knn.hip, and the compacting
// sort of the deterministic reduction (det_reduce.h: the rasterizer's backward in api.hip, the HexPlane's in hexplane_det.hip).
#pragma once
#include "common.h"

struct RadixSortArgs {
    const uint32_t* keys_in = nullptr;   // compacting sort: the raw keys -- the values are the element indices, keys equal to 0xFFFFFFFF are dropped and
                                         //   the count kept is published to *count_out by pass 0; null: the pairs start in keys[0] / vals[0]
    uint32_t *keys[2], *vals[2];         // [n_cap] ping-pong
    uint32_t* hist;                      // [1 << (bits == 9 ? 9 : 8)][ceil(n_cap / EMD_SORT_TILE)] digit histograms, reused by every pass
    size_t n_cap;                        // launch bound (ceil(n_cap / EMD_SORT_TILE) workgroups per kernel) and the element count itself, unless that is
    const uint32_t *n_dev = nullptr, *n_dev_overflow = nullptr;   // *n_dev on the device (0 while *n_dev_overflow is set); *count_out after a compacting pass 0
    int passes, bits = EMD_RADIX_BITS;   // digit width per pass: 9 selects the 512-bin kernels, <= 8 the 256-bin ones
    uint32_t offset = 0;                 // subtracted from every key before its digit is taken
    int range_bits = 32;                 // compacting sort: a kept key with (key - offset) >> range_bits != 0 raises bit 1 of *overflow_word
    uint32_t *overflow_word = nullptr, *count_out = nullptr;
    bool hist0_ready = false;            // the producer of the pairs built pass 0's histogram (k_duplicate)
};
// -> index (0 / 1) of the buffer pair that holds the sorted result (emd_radix_result_buf(keys_in != null, passes), common.h), or a negative EMD_ERR_*
int emd_launch_radix_sort(const RadixSortArgs& a, hipStream_t st);
