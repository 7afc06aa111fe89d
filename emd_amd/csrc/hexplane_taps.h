// hexplane_taps.h -- the tap arithmetic of the HexPlane lookup, shared by hexplane.hip and hexplane_det.hip: grid_sample's coordinate handling
// (bilinear, align_corners, border padding), the plane -> axis pairing and the addressing of a channel-last plane.
#pragma once
#include "common.h"

namespace {

struct Bilin { int x0, x1, y0, y1; float fx, fy, cx, cy; };   // cx, cy: d(ix)/d(coord) incl. the border-clip mask

// F.grid_sample coordinate handling: align_corners=True, padding_mode='border'
__device__ __forceinline__ void unnormalize(float c, int size, float& idx, float& dscale) {
    const float s = 0.5f * (float)(size - 1);
    float v = (c + 1.f) * s;
    dscale = s;
    if (!(v > 0.f)) { v = 0.f; dscale = 0.f; }                       // clip_coordinates_set_grad: 0 outside [0, size-1]
    else if (!(v < (float)(size - 1))) { v = (float)(size - 1); dscale = 0.f; }
    idx = v;
}

__device__ __forceinline__ Bilin bilin(float cx, float cy, int W, int H) {
    Bilin b;
    float ix, iy;
    unnormalize(cx, W, ix, b.cx);
    unnormalize(cy, H, iy, b.cy);
    const float x0 = floorf(ix), y0 = floorf(iy);
    b.fx = ix - x0; b.fy = iy - y0;
    b.x0 = (int)x0; b.y0 = (int)y0;
    b.x1 = min(b.x0 + 1, W - 1); b.y1 = min(b.y0 + 1, H - 1);      // the out-of-range neighbour has weight 0
    return b;
}

// One axis of a tap.  A scale has four axes (x, y, z, t) and six planes that pair them: the un-normalise / clip / floor work is
// done once per axis and shared by the three planes the axis takes part in (both lookup kernels are VALU-heavy -- at the measured
// 2.35 cycles per plain wave instruction, profiles/r02_issue_rate_microbench.txt, rocprofv3's SQ_INSTS_VALU fills ~60 % of the
// forward's run time -- and every lane of a point repeats this arithmetic).
struct Tap1 { int i0, i1; float f, ds; };
__device__ __forceinline__ Tap1 tap1(float coord, int size) {
    Tap1 t;
    float idx;
    unnormalize(coord, size, idx, t.ds);
    const float i0 = floorf(idx);
    t.f = idx - i0;
    t.i0 = (int)i0;
    t.i1 = min(t.i0 + 1, size - 1);                                  // the out-of-range neighbour has weight 0
    return t;
}
__device__ __forceinline__ Bilin make_bilin(const Tap1& tx, const Tap1& ty) {
    Bilin b;
    b.x0 = tx.i0; b.x1 = tx.i1; b.fx = tx.f; b.cx = tx.ds;
    b.y0 = ty.i0; b.y1 = ty.i1; b.fy = ty.f; b.cy = ty.ds;
    return b;
}

// plane pair p of (0,1),(0,2),(0,3),(1,2),(1,3),(2,3): first index -> width axis, second -> height axis
// (arithmetic, not a table: with a lane-varying p -- the staging phases, item = (point, plane) -- a table is a load from constant memory, and
// the a.res[s][axis] behind it a second, dependent one from the kernel arguments: two to three HBM-latency round trips per staging call)
__device__ __forceinline__ void pair_axes(int p, int& a, int& b) {
    a = (p >= 3) + (p >= 5);
    b = p < 3 ? p + 1 : (p == 3 ? 2 : 3);
}

__device__ __forceinline__ int sel4i(int v0, int v1, int v2, int v3, int k) { return k == 0 ? v0 : (k == 1 ? v1 : (k == 2 ? v2 : v3)); }
__device__ __forceinline__ float sel4f(float v0, float v1, float v2, float v3, int k) { return k == 0 ? v0 : (k == 1 ? v1 : (k == 2 ? v2 : v3)); }

// element offset of tap (x, y), channel c, in a channel-last plane (32-bit: a plane holds < 2^30 floats, checked on the host)
__device__ __forceinline__ uint32_t tap_at(int x, int y, int W, int C, int c) { return ((uint32_t)y * (uint32_t)W + (uint32_t)x) * (uint32_t)C + (uint32_t)c; }

__device__ __forceinline__ float sample(const float* __restrict__ pl, const Bilin& t, int W, int C, int c) {
    const float nw = pl[tap_at(t.x0, t.y0, W, C, c)], ne = pl[tap_at(t.x1, t.y0, W, C, c)];
    const float sw = pl[tap_at(t.x0, t.y1, W, C, c)], se = pl[tap_at(t.x1, t.y1, W, C, c)];
    // grid_sampler_2d: nw * (1-fx)(1-fy) + ne * fx (1-fy) + sw * (1-fx) fy + se * fx fy
    return nw * ((1.f - t.fx) * (1.f - t.fy)) + ne * (t.fx * (1.f - t.fy)) + sw * ((1.f - t.fx) * t.fy) + se * (t.fx * t.fy);
}

// the sample and its slopes d/d(ix), d/d(iy) (already times the border-clip masks) from one read of the four corners
__device__ __forceinline__ float sample_slopes(const float* __restrict__ pl, const Bilin& t, int W, int C, int c, float& dix, float& diy) {
    const float nw = pl[tap_at(t.x0, t.y0, W, C, c)], ne = pl[tap_at(t.x1, t.y0, W, C, c)];
    const float sw = pl[tap_at(t.x0, t.y1, W, C, c)], se = pl[tap_at(t.x1, t.y1, W, C, c)];
    // the clamped neighbour (x1 == x0 at the border) contributes no slope there: its weight is 0 and cx = 0
    dix = ((ne - nw) * (1.f - t.fy) + (se - sw) * t.fy) * t.cx;
    diy = ((sw - nw) * (1.f - t.fx) + (se - ne) * t.fx) * t.cy;
    return nw * ((1.f - t.fx) * (1.f - t.fy)) + ne * (t.fx * (1.f - t.fy)) + sw * ((1.f - t.fx) * t.fy) + se * (t.fx * t.fy);
}

}  // namespace
