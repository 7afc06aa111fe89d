// temporal_sample.h -- the sampling set-up of the coarse-to-fine temporal embedding (rows, columns, taps) and the argument check of its entry points:
// shared by embed.hip, embed_det.hip and track_det.hip (the backwards without atomics, DESIGN.md sections 8.14 and 8.15).  The sampling text is
// embed.hip's own, moved here unchanged.  (The accumulation the two backwards without atomics share is te_gather_body.inc.)
#pragma once
#include "common.h"

namespace {

// grid_sample coordinate: align_corners un-normalise, reflect over [0, size-1], clip; *mult = d(result)/d(coord)
// (no contraction in the sampling arithmetic of this file -- reflect_coord, resized_row, te_rows, the column coordinate, te_eval: the same source is
//  inlined into several kernels whose results are compared bit for bit, and left to itself the compiler fused e.g. `scale * r - h0` in one copy only)
__device__ __forceinline__ float reflect_coord(float c, int size, float* mult) {
#pragma clang fp contract(off)
    float v = ((c + 1.f) * 0.5f) * (float)(size - 1);
    float m = 0.5f * (float)(size - 1);
    if (size <= 1) { *mult = 0.f; return 0.f; }
    const float span = (float)(size - 1);
    if (v < 0.f) { v = -v; m = -m; }
    const float extra = fmodf(v, span);
    const int flips = (int)floorf(v / span);
    if (flips & 1) { v = span - extra; m = -m; } else v = extra;
    if (!(v > 0.f)) { v = 0.f; m = 0.f; }                       // clip_coordinates_set_grad
    else if (!(v < span)) { v = span; m = 0.f; }
    *mult = m;
    return v;
}

// row r of the table resized to k rows (upsample_bilinear2d, align_corners): two source rows and their weights
__device__ __forceinline__ void resized_row(int r, int k, int rows, int* h0, int* h1, float* l0, float* l1) {
#pragma clang fp contract(off)
    const float scale = k > 1 ? (float)(rows - 1) / (float)(k - 1) : 0.f;
    const float src = scale * (float)r;
    *h0 = (int)src;
    *h1 = *h0 + (*h0 < rows - 1 ? 1 : 0);
    *l1 = src - (float)*h0;
    *l0 = 1.f - *l1;
}

// the sample of the k-row resize at time t: the two resized rows around it (each two source rows ha / hb with weights la / lb) and their weights
struct TeSample { int ha[2], hb[2]; float la[2], lb[2], wy0, wy1; bool in1; };      // in1: the row past the end contributes nothing

__device__ __forceinline__ TeSample te_rows(float t, int k, int rows) {
#pragma clang fp contract(off)
    TeSample s;
    float my;
    const float iy = reflect_coord((t - 0.5f) * 2.f, k, &my);
    const float y0f = floorf(iy);
    const int y0 = (int)y0f, y1 = y0 + 1;
    s.wy1 = iy - y0f; s.wy0 = 1.f - s.wy1;
    resized_row(min(y0, k - 1), k, rows, &s.ha[0], &s.hb[0], &s.la[0], &s.lb[0]);
    resized_row(min(y1, k - 1), k, rows, &s.ha[1], &s.hb[1], &s.la[1], &s.lb[1]);
    s.in1 = y1 <= k - 1;
    return s;
}

// column j of a sample: the reference samples it at x = (j / (dim-1) - 0.5) * 2, which un-normalises to j up to rounding
struct TeCol { int x0, x1; float wx0, wx1; bool inx1; };

__device__ __forceinline__ TeCol te_col(int j, int dim) {
#pragma clang fp contract(off)
    TeCol c;
    float mx;
    const float gx = dim > 1 ? ((float)j / (float)(dim - 1) - 0.5f) * 2.f : -1.f;
    const float ix = reflect_coord(gx, dim, &mx);
    const float x0f = floorf(ix);
    c.x0 = (int)x0f; c.x1 = c.x0 + 1;
    c.wx1 = ix - x0f; c.wx0 = 1.f - c.wx1;
    c.inx1 = c.x1 <= dim - 1;
    return c;
}

// the eight taps of a sample, unconditionally (a tap the sample does not use -- the row past the table's end, the column past its width -- is read
// from a valid neighbour and selected away): with the loads inside the row loop's branches each row waited for its own round trip
__device__ __forceinline__ void te_taps(const float* __restrict__ weight, int dim, const TeSample& s, const TeCol& c, float (&wv)[2][4]) {
    const int x1c = c.inx1 ? c.x1 : c.x0;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        wv[r][0] = weight[s.ha[r] * dim + c.x0]; wv[r][1] = weight[s.hb[r] * dim + c.x0];
        wv[r][2] = weight[s.ha[r] * dim + x1c]; wv[r][3] = weight[s.hb[r] * dim + x1c];
    }
}

int check_te(const float* weight, int tables, int rows, int dim, int k, const float* t, const char* who) {
    if (!weight || !t) { emd_set_error("%s: null table / time", who); return EMD_ERR_INVALID; }
    if (tables < 1 || rows < 1 || dim < 1 || k < 1) { emd_set_error("%s: bad sizes tables=%d rows=%d dim=%d k=%d", who, tables, rows, dim, k); return EMD_ERR_INVALID; }
    return EMD_OK;
}

}  // namespace
