// hexplane_det.hip -- the deterministic HexPlane backward (EMD_HEX_FLAG_DETERMINISTIC; contract: include/emd_raster.h).  gfx950.
// The default backward (hexplane.hip) adds every tap row to its texel with float atomics, partly through fp64 LDS windows, in whatever order the
// workgroups run.  Here every contribution is STORED once, a stable sort lists the contributions per texel in a fixed order, and the segmented row
// sum adds each list with its pinned association (segsum.h) -- the construction of the deterministic render backward (section 8.8), plane by plane:
//   k_hexplane_det_rows<P>   lane = channel: the six samples of the scale, gi of plane P, the four weighted rows to slots k N + n, the texels as keys
//   emd_det_sort_and_sum     (det_reduce.h) the compacting, stable sort: slots per texel in ascending slot order = ascending (tap, point);
//                            the segmented row sum -> dL_dplanes[s][P]
// and one k_hexplane_det_points launch for dL_dpts / dL_dtimes / the time column, whose one-run sum is dL_dtime_sum.  No atomics anywhere.
#include <string.h>

#include "hexplane_det.h"
#include "hexplane_taps.h"

namespace {

// box-normalised x, y, z and the time of point n (the arithmetic of k_hexplane_bwd)
__device__ __forceinline__ void det_coords(const EmdHexArgs& a, long n, float q[4]) {
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = (a.pts[3 * n + k] - a.aabb[k]) * (2.f / (a.aabb[3 + k] - a.aabb[k])) - 1.f;
    q[3] = a.times[a.times_broadcast ? 0 : n];
}

// The rows of plane P of scale s.  A lane group past the last point stands on the last point (its loads are unconditional) and stores nothing.
template <int P>
__global__ void __launch_bounds__(EMD_BLOCK) k_hexplane_det_rows(EmdHexArgs a, const float* __restrict__ dL_dout, int s, float* __restrict__ rows,
                                                                 uint32_t* __restrict__ keys_in) {
    const int C = a.channels, S = a.num_scales;
    const int group = threadIdx.x / C, c = threadIdx.x % C, per_block = EMD_BLOCK / C;
    const long N = a.num_points, slot = (long)blockIdx.x * per_block + group;
    const bool live = slot < N;
    const long n = live ? slot : N - 1;
    float q[4];
    det_coords(a, n, q);
    Tap1 axis[4];
#pragma unroll
    for (int k = 0; k < 4; k++) axis[k] = tap1(q[k], a.res[s][k]);
    float f[6];
#pragma unroll
    for (int p = 0; p < 6; p++) {
        int ax, ay;
        pair_axes(p, ax, ay);
        f[p] = sample(a.planes[s][p], make_bilin(axis[ax], axis[ay]), a.res[s][ax], C, c);
    }
    const float go = dL_dout[(size_t)n * (S * C) + s * C + c];
    float pre[7], suf[7];
    pre[0] = 1.f; suf[6] = 1.f;
#pragma unroll
    for (int p = 0; p < 6; p++) pre[p + 1] = pre[p] * f[p];
#pragma unroll
    for (int p = 5; p >= 0; p--) suf[p] = suf[p + 1] * f[p];
    const float gi = go * (pre[P] * suf[P + 1]);                         // dL / d interp of plane P, channel c
    int ax, ay;
    pair_axes(P, ax, ay);
    const int W = a.res[s][ax];
    const Bilin b = make_bilin(axis[ax], axis[ay]);
    if (live) {
        // slot e = k N + n, taps in the order k_hexplane_bwd adds them; every row is stored, zeros too
        float* r = rows + ((size_t)n * C + c);
        const size_t tap_stride = (size_t)N * C;
        r[0] = gi * ((1.f - b.fx) * (1.f - b.fy));
        r[tap_stride] = gi * (b.fx * (1.f - b.fy));
        r[2 * tap_stride] = gi * ((1.f - b.fx) * b.fy);
        r[3 * tap_stride] = gi * (b.fx * b.fy);
        if (c == 0) {
            keys_in[n] = (uint32_t)(b.y0 * W + b.x0);
            keys_in[N + n] = (uint32_t)(b.y0 * W + b.x1);
            keys_in[2 * N + n] = (uint32_t)(b.y1 * W + b.x0);
            keys_in[3 * N + n] = (uint32_t)(b.y1 * W + b.x1);
        }
    }
}

// dL/dpts, dL/dtimes (or the time column of dL_dtime_sum) of every point: over scales, then planes, in the registers of the point's own C lanes, then a
// fixed xor-shuffle tree over them -- k_hexplane_bwd without its plane rows and without its atomic on the time sum
__global__ void __launch_bounds__(EMD_BLOCK) k_hexplane_det_points(EmdHexArgs a, EmdHexGrads g, float* __restrict__ tcol, uint32_t* __restrict__ tkeys,
                                                                   uint32_t* __restrict__ tslots) {
    const int C = a.channels, S = a.num_scales;
    const int group = threadIdx.x / C, c = threadIdx.x % C, per_block = EMD_BLOCK / C;
    const long N = a.num_points, slot = (long)blockIdx.x * per_block + group;
    const bool live = slot < N;
    const long n = live ? slot : N - 1;
    float q[4];
    det_coords(a, n, q);
    float dq[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; s++) {
        float f[6], dix[6], diy[6];
        Tap1 axis[4];
#pragma unroll
        for (int k = 0; k < 4; k++) axis[k] = tap1(q[k], a.res[s][k]);
#pragma unroll
        for (int p = 0; p < 6; p++) {
            int ax, ay;
            pair_axes(p, ax, ay);
            f[p] = sample_slopes(a.planes[s][p], make_bilin(axis[ax], axis[ay]), a.res[s][ax], C, c, dix[p], diy[p]);
        }
        const float go = g.dL_dout[(size_t)n * (S * C) + s * C + c];
        float pre[7], suf[7];
        pre[0] = 1.f; suf[6] = 1.f;
#pragma unroll
        for (int p = 0; p < 6; p++) pre[p + 1] = pre[p] * f[p];
#pragma unroll
        for (int p = 5; p >= 0; p--) suf[p] = suf[p + 1] * f[p];
#pragma unroll
        for (int p = 0; p < 6; p++) {
            int ax, ay;
            pair_axes(p, ax, ay);
            const float gi = go * (pre[p] * suf[p + 1]);
            dq[ax] += gi * dix[p];
            dq[ay] += gi * diy[p];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float v = dq[k];
        for (int off = C >> 1; off; off >>= 1) v += __shfl_xor(v, off, C);      // every lane of the group is here: none has left
        if (c == 0 && live) {
            if (k < 3) { if (g.dL_dpts) g.dL_dpts[3 * n + k] = v * (2.f / (a.aabb[3 + k] - a.aabb[k])); }     // through normalize_aabb
            else if (g.dL_dtimes) g.dL_dtimes[n] = v;
            else if (tcol) { tcol[n] = v; tkeys[n] = 0u; tslots[n] = (uint32_t)n; }                          // one run under key 0, in point order
        }
    }
}

// rows, sort, sum of one plane
int det_plane(const EmdHexArgs* a, const EmdHexGrads* g, int s, int p, const HexDetWs& w, hipStream_t st) {
    const int per_block = EMD_BLOCK / a->channels;
    with_int<0, 5>(p, [&](auto pc) {
        hipLaunchKernelGGL(k_hexplane_det_rows<decltype(pc)::value>, dim3((unsigned)((a->num_points + per_block - 1) / per_block)), dim3(EMD_BLOCK), 0, st, *a,
                           g->dL_dout, s, w.r.rows, w.r.s.keys_in);
    });
    EMD_LAUNCH_CHECK();
    return emd_det_sort_and_sum(w.r, emd_hex_plane_texels(a, s, p), nullptr, w.counts, g->dL_dplanes[s][p], a->channels, st);
}

}  // namespace

int emd_hexplane_backward_det(const EmdHexArgs* a, const EmdHexGrads* g, hipStream_t st) {
    const int C = a->channels, S = a->num_scales;
    // everything is decided here, before the first launch
    if (C > 32) { emd_set_error("hexplane_backward: the deterministic mode serves up to 32 channels (the row width of the segmented sum), got %d", C); return EMD_ERR_INVALID; }
    if (!emd_det_hex_points_fit(a->num_points)) { emd_set_error("hexplane_backward: the deterministic mode numbers 4 N slots in 32 bits"); return EMD_ERR_INVALID; }
    if (g->det_keep_plane > (uint32_t)(6 * S)) { emd_set_error("hexplane_backward: det_keep_plane %u names no plane of %d scales", g->det_keep_plane, S); return EMD_ERR_INVALID; }
    bool any_plane = false;
    for (int s = 0; s < S; s++)
        for (int p = 0; p < 6; p++) any_plane |= g->dL_dplanes[s][p] != nullptr;
    const bool time_sum = g->dL_dtime_sum && !g->dL_dtimes;
    HexDetWs w;
    memset(&w, 0, sizeof(w));
    if (any_plane || time_sum) {
        emd_carve_hex_det(g->det_ws, a->num_points, C, &w);
        const int rc = emd_det_check_ws("hexplane_backward: the deterministic mode", g->det_ws, g->det_bytes, w.bytes, 256, EMD_ERR_INVALID, "emd_hexplane_det_workspace_size");
        if (rc) return rc;
    }
    if (g->dL_dpts || g->dL_dtimes || time_sum) {
        const int per_block = EMD_BLOCK / C;
        hipLaunchKernelGGL(k_hexplane_det_points, dim3((unsigned)((a->num_points + per_block - 1) / per_block)), dim3(EMD_BLOCK), 0, st, *a, *g,
                           time_sum ? w.tcol : (float*)nullptr, w.tkeys, w.tslots);
        EMD_LAUNCH_CHECK();
    }
    if (time_sum) {
        SegSumArgs ss;
        ss.keys = w.tkeys; ss.slots = w.tslots; ss.n_dev = nullptr; ss.n_cap = (size_t)a->num_points;
        ss.rows = w.tcol; ss.row_pitch = 1; ss.width = 1;
        ss.out = g->dL_dtime_sum; ss.out_pitch = 1; ss.partials = w.tpartials;
        const int rc = emd_launch_segmented_row_sum(ss, st);
        if (rc) return rc;
    }
    // plane by plane through the one workspace; the kept plane last, so that its rows and lists are what the workspace holds afterwards
    const int keep = (int)g->det_keep_plane - 1;
    for (int i = 0; i <= 6 * S; i++) {
        const int sp = i < 6 * S ? i : keep;
        if (sp < 0 || (i < 6 * S && sp == keep) || !g->dL_dplanes[sp / 6][sp % 6]) continue;
        const int rc = det_plane(a, g, sp / 6, sp % 6, w, st);
        if (rc) return rc;
    }
    return EMD_OK;
}

extern "C" int emd_hexplane_det_workspace_size(const EmdHexArgs* a, size_t* bytes) {
    if (!a || !bytes || a->num_points < 0 || a->channels < 1 || a->channels > 32) {
        emd_set_error("hexplane_det_workspace_size: bad argument (need num_points >= 0 and 1 <= channels <= 32)");
        return EMD_ERR_INVALID;
    }
    HexDetWs w;
    emd_carve_hex_det(nullptr, a->num_points, a->channels, &w);
    *bytes = w.bytes;
    return EMD_OK;
}

extern "C" int emd_hexplane_det_workspace_offsets(const EmdHexArgs* a, int32_t plane, size_t out[8]) {
    if (!a || !out || a->num_points < 0 || a->channels < 1 || a->channels > 32 || a->num_scales < 1 || a->num_scales > EMD_HEX_MAX_SCALES || plane < 1 ||
        plane > 6 * a->num_scales) {
        emd_set_error("hexplane_det_workspace_offsets: bad argument (plane = 1 + 6 s + p of a call with 1 <= channels <= 32)");
        return EMD_ERR_INVALID;
    }
    HexDetWs w;
    emd_carve_hex_det(nullptr, a->num_points, a->channels, &w);
    const int64_t texels = emd_hex_plane_texels(a, (plane - 1) / 6, (plane - 1) % 6);
    const int buf = emd_det_sorted_buf(texels);
    out[0] = emd_det_offset(w.r.rows); out[1] = emd_det_offset(w.r.s.keys[buf]); out[2] = emd_det_offset(w.r.s.vals[buf]); out[3] = emd_det_offset(w.tcol);
    out[4] = emd_det_offset(w.r.s.keys_in); out[5] = emd_det_offset(w.counts); out[6] = (size_t)emd_det_sort_passes(texels); out[7] = w.bytes;
    return EMD_OK;
}
