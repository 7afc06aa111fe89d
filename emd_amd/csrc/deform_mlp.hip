// deform_mlp.hip -- OmniRe's ConditionalDeformNetwork (D ReLU layers of width W <= 256 with one skip layer, three small heads) on fp32 MFMA, forward and
// backward, without BLAS, without float atomics and without a second mode: every output is a fixed function of the call's inputs (DESIGN.md section 8.20,
// the contract: include/emd_raster.h).  The 64-wide kernels of mlp.hip keep a level's whole weight set in LDS; a 256 x 256 layer (256 KB) does not fit, so
// the kernels here work layer by layer and pass a layer's weights through LDS in blocks of 32 summation indices.
//
//   k_deform_gemm<NT, BWD, NARROW>   a workgroup = 4 waves x 32 rows x all 32 NT output columns.  Per block of 32 summation indices: the block of the
//                       weights is staged into LDS [32 NT][TS] (forward: W[o][k] as it lies; backward: transposed, so that both directions are
//                       layer_fwd of mlp_kernels.h), every wave multiplies its own 32 x 32 input tile (prefetched one block ahead, raw and
//                       unconditional: rows past the end read the last row and are not stored) onto its NT accumulators.
//                       forward:  Y = relu(b + X0 W[:, c0 : c0 + k0]^T [+ X1 W[:, c1 : c1 + k1]^T]): the skip layer's two inputs are two segments of the one
//                                 weight matrix, no concat.  The accumulator starts at b, segment 0 then segment 1, k ascending in the pairs of layer_fwd.
//                       backward: dX[:, j] = sum_o (Y[:, o] > 0 ? G[:, o] : 0) W[o][c0 + j], from 0, o ascending the same way; `addprev`: prev + that sum.
//                       NARROW: the input is the encoded [N, C_in] matrix, whose rows are not 16-byte aligned: scalar loads, columns masked.
//   k_deform_heads_fwd  the three heads as ONE [10][W] matrix in LDS (absent heads: zero rows), one output tile.
//   k_deform_heads_bwd  dL/dH = sum_j g_j Wh[j][:], j = warp 0..2, rotation 0..3, scaling 0..2, one fmaf chain per element from 0 (vector pipe: K = 10).
//   k_deform_wgrad<MASK>  dW = G^T X, db = sum G: workgroup (row group, 64 output features); wave w owns the input tiles w and w + 4 of those 64 rows of dW
//                       (4 accumulator tiles, no sum across waves), reads G and X straight in fragment form (lane = feature, registers = 16 rows: one
//                       128-byte line per half wave and register, no LDS) one step ahead, walks the group's rows in ascending steps of 32 and stores its
//                       total to slot `row group` of the slab.  Every element of every slot is written.
//   k_deform_reduce     adds the slots in ascending order in double precision from 0.0 and rounds once (the form of k_mlp_det_reduce).
#include "mlp_kernels.h"

namespace {

#define DM_ROWS 128          // rows of a workgroup of the gemm / heads kernels: four waves x one 32-row tile

struct GemmArgs {
    int N, nseg;
    const float* x[2];       // input segments [N][ldx], kx columns each
    int ldx[2], kx[2], wcol[2];      // wcol: forward: the segment's first weight column; backward: [0] = the first weight column of the OUTPUT
    const float* y;          // backward: the layer's saved output [N][ldx[0]] (the ReLU mask of x[0] = dL/dY)
    const float* w;
    int ldw;
    const float* b;          // forward
    float* out;
    int ldo, nout, relu, addprev;
};

template <bool NARROW>
__device__ __forceinline__ f32x16 dm_load_x(const float* __restrict__ x, int ld, size_t row_c, int k0, int hh, int kx) {
    if constexpr (NARROW) {
        f32x16 t;
        const float* p = x + row_c * (size_t)ld;
#pragma unroll
        for (int v = 0; v < 16; v++) {
            const int f = k0 + 8 * (v >> 2) + 4 * hh + (v & 3);
            t[v] = p[f < kx ? f : 0];
        }
        return t;
    } else return load_tile_raw(x, (size_t)ld, row_c, k0, hh);
}

// The backward's weight block, transposed: dst[c][rr] = src[rr ld + col0 + c] for the 32 rows rr of the block and c < cols_pad = 32 NT.  Whole 16-byte
// pieces of a row, eight rows x eight pieces per wave: 128-byte runs on the global side, and the four dword stores of a lane land 2-way on the LDS
// banks (bank = 16 piece + 4 i + rr mod 32; one row per wave, as stage_matrix_t walks it, is 4-way).  Needs ld, col0, cols multiples of 4, 32 rows.
// Measured at 160 000 rows, W = 256: the seven dL/dh launches of a backward 3.08 -> 2.12 ms against stage_matrix_t's dword loop.
__device__ __forceinline__ void dm_stage_t4(float* __restrict__ dst, int stride, int cols_pad, const float* __restrict__ src, int ld, int col0, int cols) {
    const int total = 32 * (cols_pad >> 2);
    for (int idx = threadIdx.x; idx < total; idx += MLP_THREADS) {
        const int rr = (idx & 7) + 8 * ((idx >> 6) & 3), c = (((idx >> 3) & 7) + 8 * (idx >> 8)) << 2;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < cols) v = *(const float4*)(src + (size_t)rr * ld + col0 + c);
        dst[c * stride + rr] = v.x; dst[(c + 1) * stride + rr] = v.y; dst[(c + 2) * stride + rr] = v.z; dst[(c + 3) * stride + rr] = v.w;
    }
}

// one input segment: acc[to] += (block of weights) x (input tile), block after block of 32 summation indices
template <int NT, bool BWD, bool NARROW>
__device__ __forceinline__ void dm_segment(f32x16 (&acc)[NT], float* __restrict__ lds, const GemmArgs& a, int s, size_t row_c, int r, int hh) {
    const int kx = a.kx[s], nb = (kx + 31) >> 5;
    f32x16 xn = dm_load_x<NARROW>(a.x[s], a.ldx[s], row_c, 0, hh, kx), yn = xn;
    if constexpr (BWD) yn = load_tile_raw(a.y, (size_t)a.ldx[s], row_c, 0, hh);
    for (int kb = 0; kb < nb; kb++) {
        f32x16 xc[1] = {xn};
        const f32x16 yc = yn;
        const int k1 = 32 * (kb + 1 < nb ? kb + 1 : kb);          // the next block, unconditionally (the last one is loaded twice)
        xn = dm_load_x<NARROW>(a.x[s], a.ldx[s], row_c, k1, hh, kx);
        if constexpr (BWD) yn = load_tile_raw(a.y, (size_t)a.ldx[s], row_c, k1, hh);
        const int k0 = 32 * kb, kn = kx - k0 < 32 ? kx - k0 : 32;
        __syncthreads();          // the previous block's reads are done
        if constexpr (BWD) {
            if (kn == 32 && !((a.ldw | a.wcol[0] | a.nout) & 3) && !((uintptr_t)a.w & 15)) dm_stage_t4(lds, TS, 32 * NT, a.w + (size_t)k0 * a.ldw, a.ldw, a.wcol[0], a.nout);
            else stage_matrix_t(lds, TS, 32, 32 * NT, a.w + (size_t)k0 * a.ldw, a.ldw, a.wcol[0], kn, a.nout);
        }
        else stage_matrix(lds, TS, 32 * NT, 32, a.w, a.ldw, a.wcol[s] + k0, a.nout, kn);
        __syncthreads();
        if constexpr (NARROW) xc[0] = mask_tile(xc[0], true, k0, hh, kx);
        if constexpr (BWD) xc[0] = mask16(xc[0], yc);
        layer_fwd<1, NT>(acc, xc, lds, TS, 0, r, hh);
    }
}

// Two waves per SIMD (219 / 241 registers at NT = 8, no scratch): a workgroup waits at two barriers per block while the weights are staged, and only a
// second resident workgroup keeps the matrix pipe busy meanwhile.
template <int NT, bool BWD, bool NARROW>
__global__ void __launch_bounds__(MLP_THREADS) MLP_OCC(2) k_deform_gemm(GemmArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[32 * NT * TS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
    const size_t row = ((size_t)blockIdx.x * MLP_WAVES + wave) * 32 + r;
    const bool ok = row < (size_t)a.N;
    const size_t row_c = ok ? row : (size_t)a.N - 1;
    f32x16 acc[NT];
#pragma unroll
    for (int to = 0; to < NT; to++) {
        acc[to] = zero16();
        if constexpr (!BWD) {
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int f = 32 * to + 8 * (v >> 2) + 4 * hh + (v & 3);
                acc[to][v] = a.b[f < a.nout ? f : 0];          // (a column past nout is not stored)
            }
        }
    }
    dm_segment<NT, BWD, NARROW>(acc, lds, a, 0, row_c, r, hh);
    if constexpr (!BWD) {
        if (a.nseg > 1) dm_segment<NT, false, false>(acc, lds, a, 1, row_c, r, hh);
    }
    const bool vec = !a.addprev && !(a.ldo & 3) && !(a.nout & 3) && !((uintptr_t)a.out & 15);
#pragma unroll
    for (int to = 0; to < NT; to++) {
        f32x16 t = acc[to];
        if (a.relu) t = relu16(t);
        if (vec) store_tile(a.out, (size_t)a.ldo, row, ok, 32 * to, hh, t, a.nout);
        else if (ok) {
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int f = 32 * to + 8 * (v >> 2) + 4 * hh + (v & 3);
                if (f < a.nout) {
                    float* __restrict__ d = a.out + row * (size_t)a.ldo + f;
                    *d = a.addprev ? *d + t[v] : t[v];
                }
            }
        }
    }
}

// ---- heads ---------------------------------------------------------------------------------------------------------------------------------------
// rows of the stacked head matrix: warp 0..2 | rotation 3..6 | scaling 7..9
#define DM_HEAD_ROWS 10
struct HeadsArgs {
    int N, W;
    const float* h;          // [N][W]
    const float* w[3];       // [3][W], [4][W], [3][W]; NULL: the head is absent
    const float* b[3];
    float* out[3];           // forward: [N][3], [N][4], [N][3]
    const float* g[3];       // backward: dL/dout
    float* gh;               // backward: dL/dh [N][W]
};
__device__ __forceinline__ int dm_head_of(int o) { return o < 3 ? 0 : o < 7 ? 1 : 2; }
__device__ __forceinline__ int dm_head_first(int k) { return k == 0 ? 0 : k == 1 ? 3 : 7; }
__device__ __forceinline__ int dm_head_width(int k) { return k == 1 ? 4 : 3; }

// Wh[o][k] into LDS [rows_pad][stride] (rows >= 10 and absent heads: zero); the biases behind it at `bias` when asked for
__device__ __forceinline__ void dm_stage_heads(float* __restrict__ lds, int stride, int rows_pad, const HeadsArgs& a, float* __restrict__ bias) {
    for (int idx = threadIdx.x; idx < rows_pad * a.W; idx += MLP_THREADS) {
        const int o = idx / a.W, k = idx - o * a.W, hd = dm_head_of(o);
        const float* p = o < DM_HEAD_ROWS ? a.w[hd] : nullptr;
        lds[o * stride + k] = p ? p[(o - dm_head_first(hd)) * a.W + k] : 0.f;
    }
    if (bias)
        for (int o = threadIdx.x; o < 32; o += MLP_THREADS) {
            const int hd = dm_head_of(o);
            const float* p = o < DM_HEAD_ROWS ? a.b[hd] : nullptr;
            bias[o] = p ? p[o - dm_head_first(hd)] : 0.f;
        }
    __syncthreads();
}

__global__ void __launch_bounds__(MLP_THREADS) k_deform_heads_fwd(HeadsArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[32 * (256 + 4) + 32];
    const int stride = a.W + 4;          // 4 x odd: conflict-free ds_read_b128 across the rows
    float* bias = lds + 32 * stride;
    dm_stage_heads(lds, stride, 32, a, bias);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
    const size_t row = ((size_t)blockIdx.x * MLP_WAVES + wave) * 32 + r;
    const bool ok = row < (size_t)a.N;
    const size_t row_c = ok ? row : (size_t)a.N - 1;
    f32x16 acc[1] = {bias_tile(bias, 0, hh)};
    const int nb = a.W >> 5;
    f32x16 xn = load_tile_raw(a.h, (size_t)a.W, row_c, 0, hh);
    for (int kb = 0; kb < nb; kb++) {
        const f32x16 xc[1] = {xn};
        xn = load_tile_raw(a.h, (size_t)a.W, row_c, 32 * (kb + 1 < nb ? kb + 1 : kb), hh);
        layer_fwd<1, 1>(acc, xc, lds, stride, 32 * kb, r, hh);
    }
    if (!ok) return;
#pragma unroll
    for (int v = 0; v < 16; v++) {
        const int f = 8 * (v >> 2) + 4 * hh + (v & 3);
        if (f < DM_HEAD_ROWS) {
            const int hd = dm_head_of(f);
            if (a.out[hd] && a.w[hd]) a.out[hd][row * dm_head_width(hd) + (f - dm_head_first(hd))] = acc[0][v];
        }
    }
}

__global__ void __launch_bounds__(MLP_THREADS) k_deform_heads_bwd(HeadsArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[DM_HEAD_ROWS * 256];
    dm_stage_heads(lds, a.W, DM_HEAD_ROWS, a, nullptr);
    const size_t q = (size_t)(a.W >> 2), total = (size_t)a.N * q;
    for (size_t idx = (size_t)blockIdx.x * MLP_THREADS + threadIdx.x; idx < total; idx += (size_t)gridDim.x * MLP_THREADS) {
        const size_t n = idx / q;
        const int c = (int)(idx - n * q) << 2;
        float g[DM_HEAD_ROWS];
#pragma unroll
        for (int j = 0; j < DM_HEAD_ROWS; j++) {
            const int hd = dm_head_of(j);
            g[j] = (a.w[hd] && a.g[hd]) ? a.g[hd][n * dm_head_width(hd) + (j - dm_head_first(hd))] : 0.f;
        }
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < DM_HEAD_ROWS; j++) {
            const float4 w = *(const float4*)(lds + j * a.W + c);
            s.x = fmaf(g[j], w.x, s.x); s.y = fmaf(g[j], w.y, s.y); s.z = fmaf(g[j], w.z, s.z); s.w = fmaf(g[j], w.w, s.w);
        }
        *(float4*)(a.gh + n * (size_t)a.W + c) = s;
    }
}

// ---- weight gradients ----------------------------------------------------------------------------------------------------------------------------
struct WgradArgs {
    int N, group_rows, nsrc, nout;
    const float* g[3];       // dL/dY as up to three column blocks: source s holds output features o0[s] .. o0[s] + ng[s] - 1 in rows of ldg[s] floats
    int ldg[3], o0[3], ng[3];
    const float* y;          // MASK: the layer's saved output [N][ldy]
    int ldy;
    const float* x;          // the layer's input [N][ldx], kx <= 256 columns
    int ldx, kx;
    float* slab_w;           // slot g: [nout][kx]
    int pitch_w;
    float* slab_b;           // slot g: [nout]; NULL: not wanted (the second block of the skip layer's weight)
    int pitch_b;
};
struct WgradRaw { f32x16 g[2], y[2], x[2]; };

// Two waves per SIMD (254 registers with the mask, no scratch).  Measured at 160 000 rows, W = 256: 2.99 ms for the nine launches of a backward against 3.01 ms
// with one wave per SIMD and 353 registers -- inside the spread; kept for the smaller footprint.
template <bool MASK>
__global__ void __launch_bounds__(MLP_THREADS) MLP_OCC(2) k_deform_wgrad(WgradArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
    const int KT = (a.kx + 31) >> 5, ob = 64 * blockIdx.y;
    const float *gp[2], *yp[2], *xp[2];
    size_t gld[2];
    bool gok[2], kon[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int o = ob + 32 * t + r;
        gp[t] = a.g[0]; gld[t] = 0; gok[t] = false;
        for (int s = 0; s < a.nsrc; s++)
            if (a.g[s] && o >= a.o0[s] && o < a.o0[s] + a.ng[s]) { gp[t] = a.g[s] + (o - a.o0[s]); gld[t] = (size_t)a.ldg[s]; gok[t] = true; }
        yp[t] = MASK ? a.y + (gok[t] ? o : 0) : nullptr;
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int kt = wave + MLP_WAVES * j, k = 32 * kt + r;
        kon[j] = kt < KT;
        xp[j] = a.x + (k < a.kx ? k : 0);
    }
    const bool t1 = ob + 32 < a.nout;          // the block's second tile of output features exists
    const size_t row0 = (size_t)blockIdx.x * a.group_rows, N = (size_t)a.N;
    const size_t rend = row0 + a.group_rows < N ? row0 + a.group_rows : N;
    // fragment form: register s of lane half hh = row base + 16 hh + s (clamped, raw: masked where used)
    auto load = [&](size_t base) {
        WgradRaw w;
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const size_t row = base + 16 * hh + s, rc = row < N ? row : N - 1;
#pragma unroll
            for (int t = 0; t < 2; t++) {
                w.g[t][s] = gp[t][rc * gld[t]];
                w.y[t][s] = MASK ? yp[t][rc * (size_t)a.ldy] : 1.f;
            }
#pragma unroll
            for (int j = 0; j < 2; j++) w.x[j][s] = xp[j][rc * (size_t)a.ldx];
        }
        return w;
    };
    f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
    float dbp[2] = {0.f, 0.f};
    WgradRaw nx = load(row0);
    for (size_t base = row0; base < rend; base += 32) {
        // this step's operands out of the loads of the step before (the ReLU mask and the row bound applied HERE, where they are used), then the next
        // step's loads, then the products
        f32x16 gf[2], xf[2] = {nx.x[0], nx.x[1]};
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int s = 0; s < 16; s++) gf[t][s] = (gok[t] && base + 16 * hh + s < rend && nx.y[t][s] > 0.f) ? nx.g[t][s] : 0.f;
        nx = load(base + 32 < rend ? base + 32 : base);
        if (wave == 0) { dbp[0] += frag_sum(gf[0]); dbp[1] += frag_sum(gf[1]); }
#pragma unroll
        for (int j = 0; j < 2; j++)
            if (kon[j]) {
                acc[0][j] = outer_acc(acc[0][j], gf[0], xf[j]);
                if (t1) acc[1][j] = outer_acc(acc[1][j], gf[1], xf[j]);
            }
    }
    // accumulator tile D[o][k]: lane r = k, register v = o
    float* __restrict__ slot = a.slab_w + (size_t)blockIdx.x * a.pitch_w;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int k = 32 * (wave + MLP_WAVES * j) + r;
        if (!kon[j] || k >= a.kx) continue;
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int o = ob + 32 * t + 8 * (v >> 2) + 4 * hh + (v & 3);
                if (o < a.nout) slot[(size_t)o * a.kx + k] = acc[t][j][v];
            }
    }
    if (wave == 0 && a.slab_b) {          // lower half of the rows + upper half, in that order
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const float both = dbp[t] + __shfl_xor(dbp[t], 32);
            const int o = ob + 32 * t + r;
            if (hh == 0 && o < a.nout) a.slab_b[(size_t)blockIdx.x * a.pitch_b + o] = both;
        }
    }
}

#define DM_MAX_JOBS 6
struct ReduceJobs { EmdMlpDetJob job[DM_MAX_JOBS]; };
__global__ void __launch_bounds__(256) k_deform_reduce(ReduceJobs jobs) {
    const EmdMlpDetJob& j = jobs.job[blockIdx.y];
    const int total = j.rows * j.cols;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const float* __restrict__ p = j.slab + e;
        double acc = 0.0;
#pragma unroll 8
        for (int s = 0; s < j.groups; s++) acc += (double)p[(size_t)s * j.pitch];          // ascending: the loads may run ahead, the adds do not
        const int o = e / j.cols, i = e - o * j.cols;
        j.dst[(size_t)o * j.ld + j.col0 + i] = (float)acc;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------
size_t dm_round256(size_t b) { return (b + 255) & ~(size_t)255; }

int dm_layout(int n, int w, int in_dim, int num_cus, EmdDeformMlpLayout* out, const char* who) {
    if (n < 0 || w < 32 || w > 256 || (w & 31) || in_dim < 1 || in_dim > 256 || num_cus < 1) {
        emd_set_error("%s: bad sizes (num_points >= 0, width a multiple of 32 up to 256, in_dim 1..256, num_cus >= 1)", who);
        return EMD_ERR_INVALID;
    }
    EmdDeformMlpLayout L;
    memset(&L, 0, sizeof(L));
    if (n > 0) {
        const int64_t target = num_cus / 2 > 0 ? num_cus / 2 : 1;
        int64_t rows = ((int64_t)n + target - 1) / target;
        rows = rows < EMD_DEFORM_MLP_MIN_GROUP_ROWS ? EMD_DEFORM_MLP_MIN_GROUP_ROWS : rows;
        rows = (rows + 31) / 32 * 32;
        L.group_rows = (int32_t)rows;
        L.groups = (int32_t)(((int64_t)n + rows - 1) / rows);
        L.pitch_w = w * (w > in_dim ? w : in_dim);
        L.pitch_b = w;
        L.offset_w = 0;
        L.offset_b = dm_round256((size_t)L.groups * L.pitch_w * sizeof(float));
        L.bytes = L.offset_b + dm_round256((size_t)L.groups * L.pitch_b * sizeof(float));
    }
    *out = L;
    return EMD_OK;
}

int dm_check(const EmdDeformMlpArgs* a, const char* who, bool need_out) {
    if (!a) { emd_set_error("%s: null args", who); return EMD_ERR_INVALID; }
    if (a->width < 32 || a->width > 256 || (a->width & 31)) { emd_set_error("%s: width %d is not a multiple of 32 up to 256", who, a->width); return EMD_ERR_INVALID; }
    if (a->depth < 2 || a->depth > EMD_DEFORM_MLP_MAX_LAYERS) { emd_set_error("%s: depth %d outside 2..%d", who, a->depth, EMD_DEFORM_MLP_MAX_LAYERS); return EMD_ERR_INVALID; }
    if (a->skip == a->depth - 1) { emd_set_error("%s: skip %d is the last layer: the heads would see the concat", who, a->skip); return EMD_ERR_INVALID; }
    if (a->skip < -1 || a->skip > a->depth - 1) { emd_set_error("%s: skip %d outside -1..%d", who, a->skip, a->depth - 2); return EMD_ERR_INVALID; }
    if (a->num_points < 0 || a->in_dim < 1 || a->in_dim > 256 || a->embed_dim < 0 || a->embed_dim > 32 || a->embed_dim > a->in_dim || a->ld_x < a->in_dim ||
        a->num_cus < 1) {
        emd_set_error("%s: bad sizes (num_points >= 0, in_dim 1..256, embed_dim 0..min(32, in_dim), ld_x >= in_dim, num_cus >= 1)", who);
        return EMD_ERR_INVALID;
    }
    if (a->num_points == 0) return EMD_OK;
    if (!a->x || !a->w_head[0] || !a->b_head[0] || (need_out && !a->out[0])) { emd_set_error("%s: null pointer (x, the warp head or its output)", who); return EMD_ERR_INVALID; }
    for (int k = 1; k < 3; k++)
        if (a->w_head[k] && (!a->b_head[k] || (need_out && !a->out[k]))) { emd_set_error("%s: head %d has a weight but no bias or output", who, k); return EMD_ERR_INVALID; }
    for (int i = 0; i < a->depth; i++) {
        if (!a->w[i] || !a->b[i] || !a->h[i]) { emd_set_error("%s: null pointer (layer %d)", who, i); return EMD_ERR_INVALID; }
        if (((uintptr_t)a->h[i] & 15)) { emd_set_error("%s: h[%d] must be 16-byte aligned", who, i); return EMD_ERR_INVALID; }
    }
    return EMD_OK;
}

template <int NT, bool BWD, bool NARROW>
int dm_gemm_launch(const GemmArgs& g, hipStream_t st) {
    hipLaunchKernelGGL((k_deform_gemm<NT, BWD, NARROW>), dim3((unsigned)(((size_t)g.N + DM_ROWS - 1) / DM_ROWS)), dim3(MLP_THREADS), 0, st, g);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}
template <bool BWD, bool NARROW>
int dm_gemm(const GemmArgs& g, hipStream_t st) {
    const int nt = (g.nout + 31) / 32;
    if (nt <= 1) return dm_gemm_launch<1, BWD, NARROW>(g, st);
    if (nt <= 2) return dm_gemm_launch<2, BWD, NARROW>(g, st);
    if (nt <= 4) return dm_gemm_launch<4, BWD, NARROW>(g, st);
    return dm_gemm_launch<8, BWD, NARROW>(g, st);
}

HeadsArgs dm_heads(const EmdDeformMlpArgs* a) {
    HeadsArgs h;
    memset(&h, 0, sizeof(h));
    h.N = a->num_points; h.W = a->width; h.h = a->h[a->depth - 1];
    for (int k = 0; k < 3; k++) { h.w[k] = a->w_head[k]; h.b[k] = a->b_head[k]; h.out[k] = a->out[k]; }
    return h;
}

int dm_reduce(const EmdMlpDetJob* jobs, int n, hipStream_t st) {
    ReduceJobs table;
    memset(&table, 0, sizeof(table));
    int most = 0;
    for (int k = 0; k < n; k++) {
        table.job[k] = jobs[k];
        most = jobs[k].rows * jobs[k].cols > most ? jobs[k].rows * jobs[k].cols : most;
    }
    hipLaunchKernelGGL(k_deform_reduce, dim3((most + 255) / 256, n), dim3(256), 0, st, table);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

EmdMlpDetJob dm_job(const float* slab, int groups, int pitch, float* dst, int rows, int cols, int ld, int col0) {
    EmdMlpDetJob j;
    memset(&j, 0, sizeof(j));
    j.slab = slab; j.dst = dst; j.groups = groups; j.pitch = pitch; j.rows = rows; j.cols = cols; j.ld = ld; j.col0 = col0; j.scale = 1.0;
    return j;
}

template <bool MASK>
int dm_wgrad(const WgradArgs& w, int groups, hipStream_t st) {
    hipLaunchKernelGGL(k_deform_wgrad<MASK>, dim3(groups, (w.nout + 63) / 64), dim3(MLP_THREADS), 0, st, w);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

}  // namespace

extern "C" int emd_deform_mlp_workspace(int num_points, int width, int in_dim, int num_cus, EmdDeformMlpLayout* layout) {
    EmdDeformMlpLayout L;
    const int rc = dm_layout(num_points, width, in_dim, num_cus, &L, "deform_mlp_workspace");
    if (rc) return rc;
    if (layout) *layout = L;
    return EMD_OK;
}

extern "C" int emd_deform_mlp_forward(const EmdDeformMlpArgs* a, void* hip_stream) {
    int rc = dm_check(a, "deform_mlp_forward", true);
    if (rc || a->num_points == 0) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const int W = a->width, C = a->in_dim;
    for (int i = 0; i < a->depth; i++) {
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        g.N = a->num_points; g.w = a->w[i]; g.b = a->b[i]; g.out = a->h[i]; g.ldo = W; g.nout = W; g.relu = 1;
        const bool first = i == 0, skip = a->skip >= 0 && i == a->skip + 1;
        if (first || skip) { g.x[0] = a->x; g.ldx[0] = a->ld_x; g.kx[0] = C; g.wcol[0] = 0; g.nseg = 1; g.ldw = C; }
        if (skip) { g.x[1] = a->h[i - 1]; g.ldx[1] = W; g.kx[1] = W; g.wcol[1] = C; g.nseg = 2; g.ldw = C + W; }
        if (!first && !skip) { g.x[0] = a->h[i - 1]; g.ldx[0] = W; g.kx[0] = W; g.wcol[0] = 0; g.nseg = 1; g.ldw = W; }
        rc = (first || skip) ? dm_gemm<false, true>(g, st) : dm_gemm<false, false>(g, st);
        if (rc) return rc;
    }
    const HeadsArgs h = dm_heads(a);
    hipLaunchKernelGGL(k_deform_heads_fwd, dim3((unsigned)(((size_t)a->num_points + DM_ROWS - 1) / DM_ROWS)), dim3(MLP_THREADS), 0, st, h);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

extern "C" int emd_deform_mlp_backward(const EmdDeformMlpArgs* a, const EmdDeformMlpGrads* g, void* hip_stream) {
    const char* who = "deform_mlp_backward";
    int rc = dm_check(a, who, false);
    if (rc || a->num_points == 0) return rc;
    if (!g || !g->g_h[0] || !g->g_h[1] || g->g_h[0] == g->g_h[1] || ((uintptr_t)g->g_h[0] & 15) || ((uintptr_t)g->g_h[1] & 15)) {
        emd_set_error("%s: needs two distinct 16-byte aligned [N][width] buffers g_h", who); return EMD_ERR_INVALID;
    }
    for (int k = 0; k < 3; k++)
        if (a->w_head[k] && (!g->g_out[k] || !g->d_w_head[k] || !g->d_b_head[k])) { emd_set_error("%s: null gradient pointer (head %d)", who, k); return EMD_ERR_INVALID; }
    for (int i = 0; i < a->depth; i++)
        if (!g->d_w[i] || !g->d_b[i]) { emd_set_error("%s: null gradient pointer (layer %d)", who, i); return EMD_ERR_INVALID; }
    if (g->d_x && g->ld_dx < a->in_dim) { emd_set_error("%s: ld_dx < in_dim", who); return EMD_ERR_INVALID; }
    EmdDeformMlpLayout L;
    rc = dm_layout(a->num_points, a->width, a->in_dim, a->num_cus, &L, who);
    if (rc) return rc;
    if (!g->slab || ((uintptr_t)g->slab & 255) || g->slab_bytes < L.bytes) {
        emd_set_error("%s: the slab is missing, not 256-byte aligned or shorter than emd_deform_mlp_workspace reports (%zu < %zu)", who, g->slab ? g->slab_bytes : (size_t)0,
                      L.bytes);
        return EMD_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int N = a->num_points, W = a->width, C = a->in_dim, E = a->embed_dim, D = a->depth;
    float* slab_w = (float*)((char*)g->slab + L.offset_w);
    float* slab_b = (float*)((char*)g->slab + L.offset_b);
    const bool want_dx = g->d_x && E > 0;
    float* d_embed = want_dx ? g->d_x + (C - E) : nullptr;

    // the heads: dL/dh of the last layer, then their weight and bias gradients
    float *gcur = g->g_h[0], *gnext = g->g_h[1];
    {
        HeadsArgs h = dm_heads(a);
        for (int k = 0; k < 3; k++) h.g[k] = g->g_out[k];
        h.gh = gcur;
        const size_t work = ((size_t)N * (W / 4) + MLP_THREADS - 1) / MLP_THREADS;
        hipLaunchKernelGGL(k_deform_heads_bwd, dim3((unsigned)(work < 4096 ? work : 4096)), dim3(MLP_THREADS), 0, st, h);
        EMD_LAUNCH_CHECK();
        WgradArgs w;
        memset(&w, 0, sizeof(w));
        w.N = N; w.group_rows = L.group_rows; w.nsrc = 3; w.nout = DM_HEAD_ROWS;
        const int first[3] = {0, 3, 7}, wid[3] = {3, 4, 3};
        for (int k = 0; k < 3; k++) { w.g[k] = a->w_head[k] ? g->g_out[k] : nullptr; w.ldg[k] = wid[k]; w.o0[k] = first[k]; w.ng[k] = wid[k]; }
        w.x = a->h[D - 1]; w.ldx = W; w.kx = W;
        w.slab_w = slab_w; w.pitch_w = L.pitch_w; w.slab_b = slab_b; w.pitch_b = L.pitch_b;
        rc = dm_wgrad<false>(w, L.groups, st);
        if (rc) return rc;
        EmdMlpDetJob jobs[DM_MAX_JOBS];
        int nj = 0;
        for (int k = 0; k < 3; k++)
            if (a->w_head[k]) {
                jobs[nj++] = dm_job(slab_w + (size_t)first[k] * W, L.groups, L.pitch_w, g->d_w_head[k], wid[k], W, W, 0);
                jobs[nj++] = dm_job(slab_b + first[k], L.groups, L.pitch_b, g->d_b_head[k], 1, wid[k], wid[k], 0);
            }
        rc = dm_reduce(jobs, nj, st);
        if (rc) return rc;
    }
    for (int i = D - 1; i >= 0; i--) {
        const bool first = i == 0, skip = a->skip >= 0 && i == a->skip + 1;
        const int ldw = first ? C : skip ? C + W : W;
        // weight and bias gradients: one launch and one reduction per input block of the layer
        for (int part = 0; part < (skip ? 2 : 1); part++) {
            const bool from_x = first || (skip && part == 0);
            WgradArgs w;
            memset(&w, 0, sizeof(w));
            w.N = N; w.group_rows = L.group_rows; w.nsrc = 1; w.nout = W;
            w.g[0] = gcur; w.ldg[0] = W; w.o0[0] = 0; w.ng[0] = W;
            w.y = a->h[i]; w.ldy = W;
            w.x = from_x ? a->x : a->h[i - 1]; w.ldx = from_x ? a->ld_x : W; w.kx = from_x ? C : W;
            w.slab_w = slab_w; w.pitch_w = L.pitch_w; w.slab_b = part == 0 ? slab_b : nullptr; w.pitch_b = L.pitch_b;
            rc = dm_wgrad<true>(w, L.groups, st);
            if (rc) return rc;
            EmdMlpDetJob jobs[2];
            int nj = 0;
            jobs[nj++] = dm_job(slab_w, L.groups, L.pitch_w, g->d_w[i], W, w.kx, ldw, (skip && part == 1) ? C : 0);
            if (part == 0) jobs[nj++] = dm_job(slab_b, L.groups, L.pitch_b, g->d_b[i], 1, W, W, 0);
            rc = dm_reduce(jobs, nj, st);
            if (rc) return rc;
        }
        // data gradients
        GemmArgs d;
        memset(&d, 0, sizeof(d));
        d.N = N; d.nseg = 1; d.x[0] = gcur; d.ldx[0] = W; d.kx[0] = W; d.y = a->h[i]; d.w = a->w[i]; d.ldw = ldw;
        if (!first) {
            GemmArgs dh = d;
            dh.wcol[0] = skip ? C : 0; dh.out = gnext; dh.ldo = W; dh.nout = W;
            rc = dm_gemm<true, false>(dh, st);
            if (rc) return rc;
        }
        if ((first || skip) && want_dx) {
            // the embedding columns of dL/dx: the skip layer's launch (the earlier one) stores, layer 0's adds its own sum to what it finds
            GemmArgs dx = d;
            dx.wcol[0] = C - E; dx.out = d_embed; dx.ldo = g->ld_dx; dx.nout = E; dx.addprev = first && a->skip >= 0;
            rc = dm_gemm<true, false>(dx, st);
            if (rc) return rc;
        }
        float* t = gcur; gcur = gnext; gnext = t;
    }
    return EMD_OK;
}
