// trainer_loss.hip -- the image tail of an OmniRe training step: the per-image affine colour correction (models/trainers/base.py:251-258) and the
// trainer's image losses (compute_losses, base.py:518-620, with models/losses.py, pytorch_msssim.SSIM(data_range=1, channel=3) and
// kornia.losses.inverse_depth_smoothness_loss).  The contract is in include/emd_raster.h (EmdTrainerLossArgs); DESIGN.md section 8.13 has the
// launch shape and the measurements.
//
// Everything is fp32 and channels-last: rgb, gt_rgb [H][W][3]; opacity, sky_mask, depth, lidar_depth [H][W].  A colour image is read as an
// [H][R] matrix of R = 3 W floats: the window of a channel is then an 11-tap filter down the rows and an 11-tap filter with taps THREE floats
// apart along a row, and no kernel needs to know which channel a float belongs to.  Rows are not 16-byte aligned for odd W: every access is a
// dword access, contiguous across the wave.
//   k_tl_pointwise    a workgroup owns one chunk of EMD_TRAINER_LOSS_CHUNK pixels: the sums of every point-wise term (a pixel owns the
//                     smoothness pair to its right and the pair below it), dL/dopacity, and dL/drgb when there is no SSIM term
//   k_tl_ssim_forward 32 x 32 tile of the [H-10][3(W-10)] SSIM map per workgroup: 42 x 62 halo of both images in LDS, separable filter of x, y,
//                     x^2, y^2, xy; the map summed; its three partial derivatives stored for the backward
//   k_tl_finalize     one workgroup: the chunks' and the tiles' fp64 partials added in ascending order, seven floats out, 1 / |v| kept
//   k_tl_ssim_backward 32 x 32 tile of the [H][3 W] image per workgroup: the same filter over the derivative maps (zero outside the map), the
//                     L1 sign gradient added, dL/drgb written once
//   k_tl_depth_grad   dL/ddepth: the depth term with the 1 / |v| of the finalize, and the smoothness term gathered from the four pairs a pixel
//                     belongs to
//   k_affine_forward / k_affine_backward / k_affine_finalize   the colour correction, dL/drgb, and the 12 sums of dL/dA by the same scheme
// No atomics anywhere: every output is a fixed function of the inputs.
#include "common.h"
#include "fixed_sum.h"

namespace {

#define TL_PIX_PER_THREAD (EMD_TRAINER_LOSS_CHUNK / EMD_BLOCK)
static_assert(EMD_TRAINER_LOSS_CHUNK % EMD_BLOCK == 0, "a chunk is whole passes of the workgroup");
#define TL_NSUM 8                    // doubles per chunk: rgb, mask, depth, |v|, entropy, smooth x, smooth y, (spare)
#define TL_FINAL_THREADS 1024
#define SS_R 10                      // taps - 1: a valid window of 11 taps reaches 10 rows down and 10 pixels = 30 floats right
#define SS_T EMD_TRAINER_SSIM_TILE   // output tile: 32 rows x 32 floats per 256-thread workgroup, 4 vertically adjacent outputs per thread
#define SS_HY (SS_T + SS_R)          // 42 rows of halo
#define SS_HX (SS_T + 3 * SS_R)      // 62 floats of halo
#define SS_V 4
static_assert(SS_T == 32 && EMD_BLOCK == 256, "the thread mapping of the SSIM kernels");
#define AFF_NSUM 12

struct Win { float w[11]; };

// the terms a call evaluates (host, tl_plan) and what the kernels derive from the weights once
struct Plan {
    int H, W;
    bool rgb, ssim, mask, depth, entropy, smooth;
    float k_rgb;                     // w_rgb / (3 P): the L1 gradient's magnitude (0 when the term is skipped)
    float k_ssim;                    // -w_ssim / (3 (H-10) (W-10))
    int64_t chunks, tiles_x, tiles_y, map_rows, map_cols;
};

__device__ __forceinline__ float tl_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// one wave: rows 0 .. n-1 of column q of a [n][stride] table of doubles.  Lane l owns the rows l, l + 64, ...: it adds them in ascending order into
// four accumulators taken in turn (four loads in flight: one accumulator made the single workgroup of a finalize wait for ~80 dependent loads),
// then the four, then the fixed tree
__device__ __forceinline__ double tl_column_sum(const double* __restrict__ tab, int64_t n, int stride, int q) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t i = threadIdx.x & 63;
    for (; i + 3 * EMD_WAVE < n; i += 4 * EMD_WAVE) {
#pragma unroll
        for (int k = 0; k < 4; k++) a[k] += tab[(i + k * EMD_WAVE) * stride + q];
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (i + k * EMD_WAVE < n) a[k] += tab[(i + k * EMD_WAVE) * stride + q];
    return fixed_wave_sum((a[0] + a[1]) + (a[2] + a[3]));
}

__device__ __forceinline__ float tl_inv_depth(float d) { return 1.f / (d + 1e-5f); }
// exp(-mean_c |a_c - b_c|) of two pixels of the ground truth
__device__ __forceinline__ float tl_edge_weight(const float (&p)[3], const float (&q)[3]) {
    const float s = fabsf(p[0] - q[0]) + fabsf(p[1] - q[1]) + fabsf(p[2] - q[2]);
    return expf(-(s / 3.f));
}

// the depth term of one pixel: the error e (0 outside the hit set, with hit = false) and de / dd
struct DepthTerm { float e, de; bool hit; };
__device__ __forceinline__ DepthTerm tl_depth_term(const EmdTrainerLossArgs& a, float d, float l, float sky) {
    DepthTerm r = {0.f, 0.f, false};
    if (!((1.f - sky) > 0.f && l > 0.01f && l < a.upper_bound && d > 1e-4f)) return r;
    r.hit = true;
    float u = d, v = l, du = 1.f;
    if (a.normalize) { u = d / a.upper_bound; v = l / a.upper_bound; du = 1.f / a.upper_bound; }
    if (a.inverse) { u = 1.f / (u + 1e-5f); v = 1.f / (v + 1e-5f); du *= -(u * u); }
    const float z = u - v;
    if (a.depth_type == EMD_TL_DEPTH_L2) { r.e = z * z; r.de = 2.f * z * du; }
    else if (a.depth_type == EMD_TL_DEPTH_SMOOTH_L1 && fabsf(z) < 1.f) { r.e = 0.5f * z * z; r.de = z * du; }
    else if (a.depth_type == EMD_TL_DEPTH_SMOOTH_L1) { r.e = fabsf(z) - 0.5f; r.de = tl_sign(z) * du; }
    else { r.e = fabsf(z); r.de = tl_sign(z) * du; }
    return r;
}

// what the point-wise pass reads of one pixel: itself, and (SMOOTH) the depth and the ground truth of its right and lower neighbours
struct Pix { float x[3], y[3], yr[3], yd[3], o, sky, d, l, dr, dd; };

// Two phases: every load of the thread's TL_PIX_PER_THREAD pixels first, unconditionally (a pixel past the end reads pixel 0, an absent input reads
// the image instead, a neighbour outside the image reads the pixel itself; none of those is used), then the arithmetic and the stores.  With the
// loads inside the branches that use them a thread made a dozen trips to memory one after the other.
template <bool SMOOTH>
__global__ void __launch_bounds__(EMD_BLOCK) k_tl_pointwise(EmdTrainerLossArgs a, Plan pl, double* __restrict__ partials) {
    const size_t P = (size_t)pl.H * pl.W;
    const int W = pl.W, H = pl.H;
    const float* __restrict__ po = a.opacity ? a.opacity : a.rgb;
    const float* __restrict__ ps = a.sky_mask ? a.sky_mask : a.rgb;
    const float* __restrict__ pd = a.depth ? a.depth : a.rgb;
    const float* __restrict__ plid = a.lidar_depth ? a.lidar_depth : a.rgb;
    Pix px[TL_PIX_PER_THREAD];
    bool right[TL_PIX_PER_THREAD], below[TL_PIX_PER_THREAD];
#pragma unroll
    for (int it = 0; it < TL_PIX_PER_THREAD; it++) {
        const size_t p = (size_t)blockIdx.x * EMD_TRAINER_LOSS_CHUNK + (size_t)it * EMD_BLOCK + threadIdx.x;
        const size_t pc = p < P ? p : 0;
        Pix& q = px[it];
#pragma unroll
        for (int c = 0; c < 3; c++) { q.x[c] = a.rgb[3 * pc + c]; q.y[c] = a.gt_rgb[3 * pc + c]; }
        q.o = po[pc]; q.sky = ps[pc]; q.d = pd[pc]; q.l = plid[pc];
        if (SMOOTH) {
            const int i = (int)(pc / (size_t)W), j = (int)(pc - (size_t)i * W);
            right[it] = j + 1 < W; below[it] = i + 1 < H;
            const size_t pr = right[it] ? pc + 1 : pc, pb = below[it] ? pc + W : pc;
            q.dr = pd[pr]; q.dd = pd[pb];
#pragma unroll
            for (int c = 0; c < 3; c++) { q.yr[c] = a.gt_rgb[3 * pr + c]; q.yd[c] = a.gt_rgb[3 * pb + c]; }
        }
    }
    double s[TL_NSUM];
#pragma unroll
    for (int q = 0; q < TL_NSUM; q++) s[q] = 0.0;
    const float inv_p = 1.f / (float)P;
#pragma unroll
    for (int it = 0; it < TL_PIX_PER_THREAD; it++) {
        const size_t p = (size_t)blockIdx.x * EMD_TRAINER_LOSS_CHUNK + (size_t)it * EMD_BLOCK + threadIdx.x;
        if (p >= P) continue;
        const Pix& q = px[it];
        if (pl.rgb) s[0] += (double)((fabsf(q.y[0] - q.x[0]) + fabsf(q.y[1] - q.x[1])) + fabsf(q.y[2] - q.x[2]));
        if (a.dL_drgb && !pl.ssim) {             // (with an SSIM term its backward writes the sum of both gradients)
#pragma unroll
            for (int c = 0; c < 3; c++) a.dL_drgb[3 * p + c] = pl.k_rgb * tl_sign(q.x[c] - q.y[c]);
        }
        if (a.dL_dopacity || pl.mask || pl.entropy) {
            const float o = q.o;
            float g = 0.f;
            if (pl.mask) {
                const bool t = (1.f - q.sky) > 0.f;
                float val, gm;
                if (a.mask_type == EMD_TL_MASK_SAFE_BCE) {
                    const float oc = fminf(fmaxf(o, 0.f), 1.f);
                    val = -fmaxf(logf(t ? oc : 1.f - oc), logf(a.safe_limit));
                    const float oh = fminf(fmaxf(oc, a.safe_limit), 1.f - a.safe_limit);
                    gm = t ? -1.f / oh : 1.f / (1.f - oh);
                } else {
                    val = -fmaxf(t ? logf(o) : log1pf(-o), -100.f);
                    gm = (o - (t ? 1.f : 0.f)) / fmaxf(o * (1.f - o), 1e-12f);
                }
                s[1] += (double)val;
                g += a.w_mask * inv_p * gm;
            }
            if (pl.entropy) {
                const float oc = fminf(fmaxf(o, 1e-6f), 1.f - 1e-6f), lg = logf(oc);
                s[4] += (double)(-oc * lg);
                if (o >= 1e-6f && o <= 1.f - 1e-6f) g += a.w_entropy * inv_p * -(lg + 1.f);
            }
            if (a.dL_dopacity) a.dL_dopacity[p] = g;
        }
        if (pl.depth) {
            const DepthTerm t = tl_depth_term(a, q.d, q.l, q.sky);
            if (t.hit) { s[2] += (double)t.e; s[3] += 1.0; }
        }
        if (SMOOTH) {
            const float iq = tl_inv_depth(q.d);
            if (right[it]) s[5] += (double)fabsf((iq - tl_inv_depth(q.dr)) * tl_edge_weight(q.y, q.yr));
            if (below[it]) s[6] += (double)fabsf((iq - tl_inv_depth(q.dd)) * tl_edge_weight(q.y, q.yd));
        }
    }
    fixed_block_store<TL_NSUM>(s, partials + (size_t)blockIdx.x * TL_NSUM);
}

// stage the SS_HY x SS_HX halos of NIMG [rows][cols] matrices whose local (0, 0) is (y0, x0), zero outside the matrix.  All of a thread's loads are
// requested before the first LDS store (as loss.hip's load_halos).
template <int NIMG>
__device__ __forceinline__ void tl_load_halos(const float* __restrict__ i0, const float* __restrict__ i1, const float* __restrict__ i2, int rows, int cols,
                                              int x0, int y0, float (*s0)[SS_HX + 1], float (*s1)[SS_HX + 1], float (*s2)[SS_HX + 1]) {
    constexpr int IT = (SS_HY * SS_HX + EMD_BLOCK - 1) / EMD_BLOCK;
    float v[3][IT];
#pragma unroll
    for (int k = 0; k < IT; k++) {
        const int i = threadIdx.x + k * EMD_BLOCK, ly = i / SS_HX, lx = i % SS_HX;
        const int x = x0 + lx, y = y0 + ly;
        const bool in = i < SS_HY * SS_HX && x >= 0 && x < cols && y >= 0 && y < rows;
        const size_t off = in ? (size_t)y * cols + x : 0;
        v[0][k] = i0[off];
        if (NIMG > 1) v[1][k] = i1[off];
        if (NIMG > 2) v[2][k] = i2[off];
    }
#pragma unroll
    for (int k = 0; k < IT; k++) {
        const int i = threadIdx.x + k * EMD_BLOCK, ly = i / SS_HX, lx = i % SS_HX;
        const int x = x0 + lx, y = y0 + ly;
        const bool in = x >= 0 && x < cols && y >= 0 && y < rows;
        if (i < SS_HY * SS_HX) {
            s0[ly][lx] = in ? v[0][k] : 0.f;
            if (NIMG > 1) s1[ly][lx] = in ? v[1][k] : 0.f;
            if (NIMG > 2) s2[ly][lx] = in ? v[2][k] : 0.f;
        }
    }
}

// the vertical pass of NQ horizontally filtered quantities: the thread's SS_V outputs at column lx, rows lyb .. lyb + SS_V - 1 of the tile
template <int NQ>
__device__ __forceinline__ void tl_vertical(const float (*hz)[SS_HY][SS_T + 1], const Win& win, int lx, int lyb, float (&acc)[SS_V][NQ]) {
#pragma unroll
    for (int j = 0; j < SS_V; j++)
#pragma unroll
        for (int m = 0; m < NQ; m++) acc[j][m] = 0.f;
#pragma unroll
    for (int r = 0; r < SS_R + SS_V; r++) {         // row lyb + r feeds output j with tap r - j
        float v[NQ];
#pragma unroll
        for (int m = 0; m < NQ; m++) v[m] = hz[m][lyb + r][lx];
#pragma unroll
        for (int j = 0; j < SS_V; j++) {
            if (r - j >= 0 && r - j < 11) {
                const float w = win.w[r - j];
#pragma unroll
                for (int m = 0; m < NQ; m++) acc[j][m] += w * v[m];
            }
        }
    }
}

__global__ void __launch_bounds__(EMD_BLOCK) k_tl_ssim_forward(EmdTrainerLossArgs a, Plan pl, Win win, double* __restrict__ tile_sums,
                                                               float* __restrict__ dmaps /* [3][map_rows][map_cols] or null */) {
    __shared__ float sx[SS_HY][SS_HX + 1], sy[SS_HY][SS_HX + 1];
    __shared__ float hz[5][SS_HY][SS_T + 1];        // horizontally filtered x, y, xx, yy, xy
    const int R = 3 * pl.W, MR = (int)pl.map_rows, MC = (int)pl.map_cols;
    const int x0 = (int)(blockIdx.x % (unsigned)pl.tiles_x) * SS_T, y0 = (int)(blockIdx.x / (unsigned)pl.tiles_x) * SS_T;
    tl_load_halos<2>(a.rgb, a.gt_rgb, nullptr, pl.H, R, x0, y0, sx, sy, nullptr);
    __syncthreads();
    for (int i = threadIdx.x; i < SS_HY * SS_T; i += EMD_BLOCK) {
        const int ly = i / SS_T, lx = i % SS_T;
        float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            const float u = sx[ly][lx + 3 * k], v = sy[ly][lx + 3 * k], w = win.w[k];
            m1 += w * u; m2 += w * v; xx += w * (u * u); yy += w * (v * v); xy += w * (u * v);
        }
        hz[0][ly][lx] = m1; hz[1][ly][lx] = m2; hz[2][ly][lx] = xx; hz[3][ly][lx] = yy; hz[4][ly][lx] = xy;
    }
    __syncthreads();
    const int lx = threadIdx.x & 31, lyb = (threadIdx.x >> 5) * SS_V;
    const int x = x0 + lx;
    float acc[SS_V][5];
    tl_vertical<5>(hz, win, lx, lyb, acc);
    float val = 0.f;
    const size_t MS = (size_t)MR * MC;
#pragma unroll
    for (int j = 0; j < SS_V; j++) {
        const int y = y0 + lyb + j;
        if (x < MC && y < MR) {
            const float mu1 = acc[j][0], mu2 = acc[j][1], xx = acc[j][2], yy = acc[j][3], xy = acc[j][4];
            const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
            const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = xx - mu1s, s2 = yy - mu2s, s12 = xy - mu12;
            const float A = 2.f * mu12 + C1, B = 2.f * s12 + C2, Cc = mu1s + mu2s + C1, D = s1 + s2 + C2;
            val += (A * B) / (Cc * D);
            if (dmaps) {
                // d map / d mu1 (through mu1^2 and mu1 mu2 everywhere they occur), d map / d filt(x^2), d map / d filt(xy)
                const float dm_dmu1 = (mu2 * 2.f * B) / (Cc * D) - (mu2 * 2.f * A) / (Cc * D) - (mu1 * 2.f * A * B) / (Cc * Cc * D) +
                                      (mu1 * 2.f * A * B) / (Cc * D * D);
                const size_t q = (size_t)y * MC + x;
                dmaps[q] = dm_dmu1;
                dmaps[MS + q] = -(A * B) / (Cc * D * D);
                dmaps[2 * MS + q] = (2.f * A) / (Cc * D);
            }
        }
    }
    const double v1[1] = {(double)val};
    fixed_block_store<1>(v1, tile_sums + blockIdx.x);
}

__global__ void __launch_bounds__(EMD_BLOCK) k_tl_ssim_backward(EmdTrainerLossArgs a, Plan pl, Win win, const float* __restrict__ dmaps) {
    __shared__ float s0[SS_HY][SS_HX + 1], s1[SS_HY][SS_HX + 1], s2[SS_HY][SS_HX + 1];
    __shared__ float hz[3][SS_HY][SS_T + 1];
    const int R = 3 * pl.W, MR = (int)pl.map_rows, MC = (int)pl.map_cols;
    const size_t MS = (size_t)MR * MC;
    const int tiles_x = (R + SS_T - 1) / SS_T;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * SS_T, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * SS_T;
    // image float (y, x) lies in the windows of the map entries (y - 10 .. y, x - 30 .. x step 3); the window is symmetric, so the filter
    // over them is the forward's filter with the halo's origin moved up and left
    tl_load_halos<3>(dmaps, dmaps + MS, dmaps + 2 * MS, MR, MC, x0 - 3 * SS_R, y0 - SS_R, s0, s1, s2);
    __syncthreads();
    for (int i = threadIdx.x; i < SS_HY * SS_T; i += EMD_BLOCK) {
        const int ly = i / SS_T, lx = i % SS_T;
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) { const float w = win.w[k]; t0 += w * s0[ly][lx + 3 * k]; t1 += w * s1[ly][lx + 3 * k]; t2 += w * s2[ly][lx + 3 * k]; }
        hz[0][ly][lx] = t0; hz[1][ly][lx] = t1; hz[2][ly][lx] = t2;
    }
    __syncthreads();
    const int lx = threadIdx.x & 31, lyb = (threadIdx.x >> 5) * SS_V;
    const int x = x0 + lx;
    float acc[SS_V][3];
    tl_vertical<3>(hz, win, lx, lyb, acc);
    // the four outputs' inputs first (a float outside the image reads float 0 and is not stored), then the arithmetic and the stores
    size_t q[SS_V];
    bool ok[SS_V];
    float xv[SS_V], yv[SS_V];
#pragma unroll
    for (int j = 0; j < SS_V; j++) {
        const int y = y0 + lyb + j;
        ok[j] = x < R && y < pl.H;
        q[j] = ok[j] ? (size_t)y * R + x : 0;
        xv[j] = a.rgb[q[j]]; yv[j] = a.gt_rgb[q[j]];
    }
#pragma unroll
    for (int j = 0; j < SS_V; j++)
        if (ok[j]) a.dL_drgb[q[j]] = pl.k_rgb * tl_sign(xv[j] - yv[j]) + pl.k_ssim * (acc[j][0] + 2.f * xv[j] * acc[j][1] + yv[j] * acc[j][2]);
}

// results the later kernels read: [0] 1 / max(|v|, 1) of the depth term
#define TL_NRES 2
__global__ void __launch_bounds__(TL_FINAL_THREADS) k_tl_finalize(EmdTrainerLossArgs a, Plan pl, const double* __restrict__ partials,
                                                                  const double* __restrict__ tile_sums, double* __restrict__ results) {
    __shared__ double tot[TL_NSUM + 1];
    const int wave = threadIdx.x >> 6;
    if (wave < TL_NSUM) {
        const double v = tl_column_sum(partials, pl.chunks, TL_NSUM, wave);
        if ((threadIdx.x & 63) == 0) tot[wave] = v;
    } else if (wave == TL_NSUM) {
        const double v = pl.ssim ? tl_column_sum(tile_sums, pl.tiles_x * pl.tiles_y, 1, 0) : 0.0;
        if ((threadIdx.x & 63) == 0) tot[TL_NSUM] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double P = (double)pl.H * (double)pl.W, H = (double)pl.H, W = (double)pl.W;
        const double cnt = tot[3] > 1.0 ? tot[3] : 1.0;
        double t[6];
        t[0] = pl.rgb ? (double)a.w_rgb * (tot[0] / (3.0 * P)) : 0.0;
        t[1] = pl.ssim ? (double)a.w_ssim * (1.0 - tot[TL_NSUM] / (3.0 * (double)pl.map_rows * (double)(pl.W - 10))) : 0.0;
        t[2] = pl.mask ? (double)a.w_mask * (tot[1] / P) : 0.0;
        t[3] = pl.depth ? (double)a.w_depth * (tot[2] / cnt) : 0.0;
        t[4] = pl.entropy ? (double)a.w_entropy * (tot[4] / P) : 0.0;
        t[5] = pl.smooth ? (double)a.w_smooth * (tot[5] / (H * (W - 1.0)) + tot[6] / ((H - 1.0) * W)) : 0.0;
        a.losses[0] = (float)(((t[0] + t[1]) + (t[2] + t[3])) + (t[4] + t[5]));
#pragma unroll
        for (int k = 0; k < 6; k++) a.losses[1 + k] = (float)t[k];
        results[0] = 1.0 / cnt;
        results[1] = 0.0;
    }
}

// Every load first, unconditionally, as the point-wise pass (a neighbour outside the image reads the pixel itself and is not used).
__global__ void __launch_bounds__(EMD_BLOCK) k_tl_depth_grad(EmdTrainerLossArgs a, Plan pl, const double* __restrict__ results) {
    const size_t P = (size_t)pl.H * pl.W;
    const size_t p = (size_t)blockIdx.x * EMD_BLOCK + threadIdx.x;
    if (p >= P) return;
    const int W = pl.W, H = pl.H;
    const int i = (int)(p / (size_t)W), j = (int)(p - (size_t)i * W);
    const bool has[4] = {j + 1 < W, j > 0, i + 1 < H, i > 0};                    // right, left, below, above
    const size_t nb[4] = {has[0] ? p + 1 : p, has[1] ? p - 1 : p, has[2] ? p + W : p, has[3] ? p - W : p};
    const float* __restrict__ ps = a.sky_mask ? a.sky_mask : a.depth;
    const float* __restrict__ plid = a.lidar_depth ? a.lidar_depth : a.depth;
    const float d = a.depth[p], l = plid[p], sky = ps[p], inv_cnt = (float)((double)a.w_depth * results[0]);
    float dn[4], y[3], yn[4][3];
#pragma unroll
    for (int c = 0; c < 3; c++) y[c] = a.gt_rgb[3 * p + c];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        dn[k] = a.depth[nb[k]];
#pragma unroll
        for (int c = 0; c < 3; c++) yn[k][c] = a.gt_rgb[3 * nb[k] + c];
    }
    float g = 0.f;
    if (pl.depth) {
        const DepthTerm t = tl_depth_term(a, d, l, sky);
        if (t.hit) g += inv_cnt * t.de;
    }
    if (pl.smooth) {
        const float q = tl_inv_depth(d);
        float gx = 0.f, gy = 0.f;               // d / dq of the sums over the x pairs and over the y pairs
        if (has[0]) gx += tl_sign(q - tl_inv_depth(dn[0])) * tl_edge_weight(y, yn[0]);
        if (has[1]) gx -= tl_sign(tl_inv_depth(dn[1]) - q) * tl_edge_weight(yn[1], y);
        if (has[2]) gy += tl_sign(q - tl_inv_depth(dn[2])) * tl_edge_weight(y, yn[2]);
        if (has[3]) gy -= tl_sign(tl_inv_depth(dn[3]) - q) * tl_edge_weight(yn[3], y);
        const float kx = a.w_smooth / ((float)H * (float)(W - 1)), ky = a.w_smooth / ((float)(H - 1) * (float)W);
        g += (kx * gx + ky * gy) * -(q * q);
    }
    a.dL_ddepth[p] = g;
}

// ---- the affine colour correction ----
__global__ void __launch_bounds__(EMD_BLOCK) k_affine_forward(int64_t P, const float* __restrict__ rgb, const float* __restrict__ A, float* __restrict__ out) {
    float m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = A[k];
    for (int it = 0; it < TL_PIX_PER_THREAD; it++) {
        const int64_t p = (int64_t)blockIdx.x * EMD_TRAINER_LOSS_CHUNK + (int64_t)it * EMD_BLOCK + threadIdx.x;
        if (p >= P) break;
        const float r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2];
#pragma unroll
        for (int c = 0; c < 3; c++) out[3 * p + c] = ((m[4 * c] * r + m[4 * c + 1] * g) + m[4 * c + 2] * b) + m[4 * c + 3];
    }
}

__global__ void __launch_bounds__(EMD_BLOCK) k_affine_backward(int64_t P, const float* __restrict__ rgb, const float* __restrict__ A,
                                                               const float* __restrict__ g_out, float* __restrict__ d_rgb, double* __restrict__ partials) {
    float m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = A[k];
    double s[AFF_NSUM];
#pragma unroll
    for (int k = 0; k < AFF_NSUM; k++) s[k] = 0.0;
    for (int it = 0; it < TL_PIX_PER_THREAD; it++) {
        const int64_t p = (int64_t)blockIdx.x * EMD_TRAINER_LOSS_CHUNK + (int64_t)it * EMD_BLOCK + threadIdx.x;
        if (p >= P) break;
        const float g[3] = {g_out[3 * p], g_out[3 * p + 1], g_out[3 * p + 2]};
        if (d_rgb) {
#pragma unroll
            for (int c = 0; c < 3; c++) d_rgb[3 * p + c] = (m[c] * g[0] + m[4 + c] * g[1]) + m[8 + c] * g[2];
        }
        if (partials) {
            const float x[3] = {rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]};
#pragma unroll
            for (int c = 0; c < 3; c++) {
#pragma unroll
                for (int k = 0; k < 3; k++) s[4 * c + k] += (double)g[c] * (double)x[k];          // exact products
                s[4 * c + 3] += (double)g[c];
            }
        }
    }
    if (partials) fixed_block_store<AFF_NSUM>(s, partials + (size_t)blockIdx.x * AFF_NSUM);
}

__global__ void __launch_bounds__(TL_FINAL_THREADS) k_affine_finalize(int64_t chunks, const double* __restrict__ partials, float* __restrict__ d_A) {
    const int wave = threadIdx.x >> 6;
    if (wave >= AFF_NSUM) return;
    const double v = tl_column_sum(partials, chunks, AFF_NSUM, wave);
    if ((threadIdx.x & 63) == 0) d_A[wave] = (float)v;
}

const int64_t TL_MAX_SIDE = 32768;

Win tl_window() {
    // pytorch_msssim._fspecial_gauss_1d(11, 1.5): exp(-(k - 5)^2 / (2 sigma^2)), normalised
    Win win;
    double g[11], s = 0.0;
    for (int k = 0; k < 11; k++) { g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)); s += g[k]; }
    for (int k = 0; k < 11; k++) win.w[k] = (float)(g[k] / s);
    return win;
}

struct TlWs { size_t partials, tiles, results, dmaps, bytes; };
TlWs tl_carve(const Plan& pl) {
    TlWs w;
    size_t off = 0;
    w.partials = off; off += (size_t)pl.chunks * TL_NSUM * sizeof(double);
    w.tiles = off; off += (size_t)(pl.tiles_x * pl.tiles_y) * sizeof(double);
    w.results = off; off += TL_NRES * sizeof(double);
    w.dmaps = off; off += (size_t)3 * pl.map_rows * pl.map_cols * sizeof(float);
    w.bytes = off;
    return w;
}

// Validates everything but the workspace and decides which terms run.  0 or a negative code.
int tl_plan(const EmdTrainerLossArgs* a, bool pointers, Plan* pl, const char* who) {
    if (!a) { emd_set_error("%s: null args", who); return EMD_ERR_INVALID; }
    if (a->height < 1 || a->width < 1 || a->height > TL_MAX_SIDE || a->width > TL_MAX_SIDE) {
        emd_set_error("%s: bad size %d x %d (1 .. %d each)", who, a->height, a->width, (int)TL_MAX_SIDE);
        return EMD_ERR_INVALID;
    }
    const float w[6] = {a->w_rgb, a->w_ssim, a->w_mask, a->w_depth, a->w_entropy, a->w_smooth};
    for (int k = 0; k < 6; k++)
        if (!(w[k] == w[k]) || w[k] - w[k] != 0.f) { emd_set_error("%s: weight %d is not finite", who, k); return EMD_ERR_INVALID; }
    if (a->mask_type != EMD_TL_MASK_BCE && a->mask_type != EMD_TL_MASK_SAFE_BCE) { emd_set_error("%s: bad mask_type %d", who, a->mask_type); return EMD_ERR_INVALID; }
    if (a->depth_type < EMD_TL_DEPTH_L1 || a->depth_type > EMD_TL_DEPTH_SMOOTH_L1) { emd_set_error("%s: bad depth_type %d", who, a->depth_type); return EMD_ERR_INVALID; }
    pl->H = a->height; pl->W = a->width;
    pl->rgb = a->w_rgb != 0.f;
    pl->ssim = a->w_ssim != 0.f;
    pl->mask = a->w_mask != 0.f && a->opacity && a->sky_mask;
    pl->depth = a->w_depth != 0.f && a->depth && a->lidar_depth && a->sky_mask;
    pl->entropy = a->w_entropy != 0.f && a->opacity;
    pl->smooth = a->w_smooth != 0.f && a->depth;
    if (pl->ssim && (a->height < 11 || a->width < 11)) {
        emd_set_error("%s: the SSIM window needs 11 x 11 pixels, the image is %d x %d", who, a->height, a->width);
        return EMD_ERR_INVALID;
    }
    if (pl->smooth && (a->height < 2 || a->width < 2)) {
        emd_set_error("%s: the smoothness term needs 2 x 2 pixels, the image is %d x %d", who, a->height, a->width);
        return EMD_ERR_INVALID;
    }
    if (pl->mask && a->mask_type == EMD_TL_MASK_SAFE_BCE && !(a->safe_limit > 0.f && a->safe_limit < 0.5f)) {
        emd_set_error("%s: safe_limit %g outside (0, 0.5)", who, (double)a->safe_limit);
        return EMD_ERR_INVALID;
    }
    if (pl->depth && !(a->upper_bound > 0.01f)) { emd_set_error("%s: upper_bound %g is not above 0.01", who, (double)a->upper_bound); return EMD_ERR_INVALID; }
    const double P = (double)a->height * (double)a->width;
    pl->k_rgb = pl->rgb ? (float)((double)a->w_rgb / (3.0 * P)) : 0.f;
    const bool window = a->height >= 11 && a->width >= 11;
    pl->map_rows = window ? a->height - 10 : 0;
    pl->map_cols = window ? 3 * (int64_t)(a->width - 10) : 0;
    pl->k_ssim = pl->ssim ? (float)(-(double)a->w_ssim / ((double)pl->map_rows * (double)pl->map_cols)) : 0.f;
    pl->tiles_x = (pl->map_cols + SS_T - 1) / SS_T;
    pl->tiles_y = (pl->map_rows + SS_T - 1) / SS_T;
    pl->chunks = ((int64_t)a->height * a->width + EMD_TRAINER_LOSS_CHUNK - 1) / EMD_TRAINER_LOSS_CHUNK;
    if (pointers) {
        if (!a->rgb || !a->gt_rgb || !a->losses) { emd_set_error("%s: null rgb / gt_rgb / losses", who); return EMD_ERR_INVALID; }
        if (a->dL_dopacity && !a->opacity) { emd_set_error("%s: dL_dopacity without opacity", who); return EMD_ERR_INVALID; }
        if (a->dL_ddepth && !a->depth) { emd_set_error("%s: dL_ddepth without depth", who); return EMD_ERR_INVALID; }
        const void* ps[] = {a->rgb, a->gt_rgb, a->opacity, a->sky_mask, a->depth, a->lidar_depth, a->losses, a->dL_drgb, a->dL_dopacity, a->dL_ddepth};
        for (const void* q : ps)
            if ((uintptr_t)q & 3) { emd_set_error("%s: a pointer is not 4-byte aligned", who); return EMD_ERR_INVALID; }
    }
    return EMD_OK;
}

int aff_check(int64_t P, const char* who) {
    if (P < 1 || P > TL_MAX_SIDE * TL_MAX_SIDE) { emd_set_error("%s: bad pixel count %lld", who, (long long)P); return EMD_ERR_INVALID; }
    return EMD_OK;
}
int64_t aff_chunks(int64_t P) { return (P + EMD_TRAINER_LOSS_CHUNK - 1) / EMD_TRAINER_LOSS_CHUNK; }

}  // namespace

extern "C" size_t emd_trainer_loss_workspace_size(const EmdTrainerLossArgs* a) {
    Plan pl;
    if (tl_plan(a, false, &pl, "trainer_loss_workspace_size") != EMD_OK) return 0;
    return tl_carve(pl).bytes;
}

extern "C" int emd_trainer_loss(const EmdTrainerLossArgs* a, void* workspace, size_t workspace_bytes, void* hip_stream) {
    Plan pl;
    const int rc = tl_plan(a, true, &pl, "trainer_loss");
    if (rc != EMD_OK) return rc;
    const TlWs ws = tl_carve(pl);
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < ws.bytes) {
        emd_set_error("trainer_loss: workspace missing, misaligned or smaller than emd_trainer_loss_workspace_size()");
        return EMD_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    char* base = (char*)workspace;
    double* partials = (double*)(base + ws.partials);
    double* tiles = (double*)(base + ws.tiles);
    double* results = (double*)(base + ws.results);
    float* dmaps = (float*)(base + ws.dmaps);
    const Win win = tl_window();
    with_bool(pl.smooth, [&](auto smooth) {
        hipLaunchKernelGGL(k_tl_pointwise<decltype(smooth)::value>, dim3((unsigned)pl.chunks), dim3(EMD_BLOCK), 0, st, *a, pl, partials);
        return 0;
    });
    EMD_LAUNCH_CHECK();
    if (pl.ssim) {
        hipLaunchKernelGGL(k_tl_ssim_forward, dim3((unsigned)(pl.tiles_x * pl.tiles_y)), dim3(EMD_BLOCK), 0, st, *a, pl, win, tiles,
                           a->dL_drgb ? dmaps : nullptr);
        EMD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_tl_finalize, dim3(1), dim3(TL_FINAL_THREADS), 0, st, *a, pl, (const double*)partials, (const double*)tiles, results);
    EMD_LAUNCH_CHECK();
    if (pl.ssim && a->dL_drgb) {
        const int64_t bx = (3 * (int64_t)pl.W + SS_T - 1) / SS_T, by = ((int64_t)pl.H + SS_T - 1) / SS_T;
        hipLaunchKernelGGL(k_tl_ssim_backward, dim3((unsigned)(bx * by)), dim3(EMD_BLOCK), 0, st, *a, pl, win, (const float*)dmaps);
        EMD_LAUNCH_CHECK();
    }
    if (a->dL_ddepth) {
        const int64_t P = (int64_t)pl.H * pl.W;
        hipLaunchKernelGGL(k_tl_depth_grad, dim3((unsigned)((P + EMD_BLOCK - 1) / EMD_BLOCK)), dim3(EMD_BLOCK), 0, st, *a, pl, (const double*)results);
        EMD_LAUNCH_CHECK();
    }
    return EMD_OK;
}

extern "C" size_t emd_affine_workspace_size(int64_t num_pixels) {
    if (num_pixels < 1 || num_pixels > TL_MAX_SIDE * TL_MAX_SIDE) return 0;
    return (size_t)aff_chunks(num_pixels) * AFF_NSUM * sizeof(double);
}

extern "C" int emd_affine_forward(int64_t num_pixels, const float* rgb, const float* affine, float* out, void* hip_stream) {
    const int rc = aff_check(num_pixels, "affine_forward");
    if (rc != EMD_OK) return rc;
    if (!rgb || !affine || !out || (((uintptr_t)rgb | (uintptr_t)affine | (uintptr_t)out) & 3)) {
        emd_set_error("affine_forward: null or misaligned rgb / affine / out");
        return EMD_ERR_INVALID;
    }
    hipLaunchKernelGGL(k_affine_forward, dim3((unsigned)aff_chunks(num_pixels)), dim3(EMD_BLOCK), 0, (hipStream_t)hip_stream, num_pixels, rgb, affine, out);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_affine_backward(int64_t num_pixels, const float* rgb, const float* affine, const float* dL_dout, float* dL_drgb, float* dL_daffine,
                                   void* workspace, size_t workspace_bytes, void* hip_stream) {
    const int rc = aff_check(num_pixels, "affine_backward");
    if (rc != EMD_OK) return rc;
    if (!affine || !dL_dout || (!dL_drgb && !dL_daffine) || (dL_daffine && !rgb)) {
        emd_set_error("affine_backward: null affine / dL_dout, no output asked for, or dL_daffine without rgb");
        return EMD_ERR_INVALID;
    }
    if (((uintptr_t)rgb | (uintptr_t)affine | (uintptr_t)dL_dout | (uintptr_t)dL_drgb | (uintptr_t)dL_daffine) & 3) {
        emd_set_error("affine_backward: a pointer is not 4-byte aligned");
        return EMD_ERR_INVALID;
    }
    if (dL_daffine && (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < emd_affine_workspace_size(num_pixels))) {
        emd_set_error("affine_backward: workspace missing, misaligned or smaller than emd_affine_workspace_size()");
        return EMD_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int64_t chunks = aff_chunks(num_pixels);
    double* partials = dL_daffine ? (double*)workspace : nullptr;
    hipLaunchKernelGGL(k_affine_backward, dim3((unsigned)chunks), dim3(EMD_BLOCK), 0, st, num_pixels, rgb, affine, dL_dout, dL_drgb, partials);
    EMD_LAUNCH_CHECK();
    if (dL_daffine) {
        hipLaunchKernelGGL(k_affine_finalize, dim3(1), dim3(TL_FINAL_THREADS), 0, st, chunks, (const double*)partials, dL_daffine);
        EMD_LAUNCH_CHECK();
    }
    return EMD_OK;
}
