// segsum.h -- segmented row sum with a PINNED association (segsum.hip): the deterministic replacement of "every contribution adds itself to its
// destination with a float atomic".  Callers: the deterministic reduction (det_reduce.h) for the render backward's per-Gaussian accumulator rows and
// the actor-pose gradient (api.hip, EMD_FLAG_DETERMINISTIC) and for the HexPlane's plane gradients (hexplane_det.hip, EMD_HEX_FLAG_DETERMINISTIC), whose
// time-column sum calls it directly; the C entry emd_segmented_row_sum (include/emd_raster.h) for the tests.
//
// Input: n elements in a fixed order; element e has a destination keys[e] (NON-DECREASING in e) and a row slots[e] of `rows` (row_pitch floats
// apart, the first `width` of them payload).  A RUN is a maximal range of elements with equal keys.  For every run the launcher writes
//     out[key * out_pitch + f],  f < width;
// destinations without a run are not written, the floats of a row behind `width` are neither read nor written.
//
// The association -- it depends on the run's LENGTH and on an element's POSITION IN ITS RUN only, never on how lanes, waves or launches are
// laid out, so any implementation of this header gives the same bits:
//   1. a run is cut into consecutive CHUNKS of EMD_SEG_CHUNK elements (the last one may be shorter);
//   2. a chunk is summed in ascending element order in fp64, starting from 0.0 (the fp32 payload converts exactly);
//   3. the chunk sums are added in ascending chunk order in fp64, starting from 0.0;
//   4. the result is rounded to fp32 once (round to nearest even).
// (Consequences the tests pin: a run of -0.0 gives +0.0; the order is the ELEMENT order, whatever the order of the slots in memory.)
// fp64 because an actor's pose run is thousands of points long: a sequential fp32 sum of 5 000 terms does not stay inside POSE_TERM_RTOL x sum|terms|.
// EMD_SEG_CHUNK = 512 rows (include/emd_raster.h): long enough that the 2.6-row runs of the render backward and all but the largest actors are
// one chunk, short enough that one frame-filling Gaussian (4 x 6 700 rows) spreads over 50 lane groups instead of being one group's tail.
//
// Layout (not part of the contract): launch 1 visits every element with a group of G = 16 or 32 lanes (lane = float of the row; the groups stride
// over the elements up to the device-side count).  The group of a
// run's first element walks the run's first chunk; a group whose element lies a whole number of chunks behind its run's start (found by a binary
// search in the sorted keys, only ever made EMD_SEG_CHUNK elements deep inside a run) walks that chunk.  Runs of one chunk are written at once; the
// chunk sums of longer runs go to `partials` (fp64) and launch 2 adds them per run.  Both launches derive everything from the keys: nothing in
// `partials` is read that the same call did not write, so the buffer needs no clearing.  No atomics, no fences, no look-back.
#pragma once
#include "common.h"

static_assert(EMD_SEG_CHUNK == 512, "the chunk length is part of the pinned association: changing it changes every deterministic gradient");

struct SegSumArgs {
    const uint32_t* keys;          // [n] non-decreasing destination ids
    const uint32_t* slots;         // [n] row index of every element
    const uint32_t* n_dev;         // device-side element count (<= n_cap), or null: n = n_cap
    size_t n_cap;                  // launch bound
    const float* rows;             // [.., row_pitch]
    int row_pitch, width;          // 1 <= width <= 32, width <= row_pitch
    float* out;                    // [.., out_pitch]
    int out_pitch;
    double* partials;              // emd_segsum_partial_bytes(n_cap, width) bytes, 8-byte aligned; never cleared
};
// lanes per element: the payload rounded up to 16 or 32
static inline int emd_segsum_group(int width) { return width <= 16 ? 16 : 32; }
// two chunk sums per EMD_SEG_CHUNK elements (a window of that many elements holds at most two chunk starts of runs longer than a chunk)
static inline size_t emd_segsum_partial_bytes(size_t n_cap, int width) {
    return 2 * ((n_cap + EMD_SEG_CHUNK - 1) / EMD_SEG_CHUNK) * (size_t)emd_segsum_group(width) * sizeof(double);
}
int emd_launch_segmented_row_sum(const SegSumArgs& a, hipStream_t st);
