// mlp_kernels.h -- what mlp.hip (the default kernels: float atomics onto the caller's zero-filled gradients) and mlp_det.hip (the deterministic forms:
// one slab slot per workgroup) share: the tile / MFMA helpers, the LDS layouts, the flush policies, the argument checks and the host
// dispatch.  The BODIES of the head forward and of the three backward kernel families are one source text for both units as well, in mlp_*_body.inc:
// each unit includes them inside its own __global__ functions next to a flush policy `fl` -- FlushAtomic (one unsafeAtomicAdd per element, as ever) or
// FlushSlab (one plain store into slot blockIdx.x of a slab) -- and names its kernels to the dispatch through a `Kernels` struct, so the kernel symbols
// and the machine code of mlp.hip stay what they were (profiles/mlp_det_isa.txt).  The block comment of mlp.hip describes the kernels themselves.
#pragma once
#include <string.h>

#include <atomic>

#include "common.h"
#include "device_utils.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define MLP_W 64          // layer width
#define WS 68             // LDS row stride of a [.][64] weight matrix (floats): 4 x odd -> conflict-free ds_read_b128 across 16 rows
#define TS 36             // LDS row stride of a transposed 32 x 32 tile
#define MLP_THREADS 256
#define MLP_WAVES (MLP_THREADS / 64)
#define MLP_OCC(n) __attribute__((amdgpu_waves_per_eu(n, n)))
// Waves per SIMD of every kernel family, written HERE only: the kernel's MLP_OCC(...) and its launcher both read it (a workgroup is four waves, one per
// SIMD, so the value is also the number of persistent workgroups per CU: mlp_grid).  Two (<= 256 registers each) where the accumulators allow it: a
// single wave exposes every LDS / HBM wait to the MFMA pipe (measured: SQ_VALU_MFMA_BUSY_CYCLES = 45-59 % of the kernel time with one wave per SIMD).
// Measured round 3: k_mlp_branch_fwd<1,1> 228 -> 219 us, k_mlp_trunk_bwd<0> 504 -> 457 us at 2 M rows; the others spill at half the register file and
// lose.  The narrow heads' forward keeps two WITH the folded L1 sum as well (195 -> 182 us at 2 M rows; 152 without the sum).
// The trunk's forward and backward happen to agree today; they are two decisions about two kernels with different register needs, not one.
constexpr int branch_fwd_waves(int depth, int nto) { return depth == 1 && nto == 1 ? 2 : 1; }
constexpr int branch_bwd_waves = 1;
constexpr int trunk_fwd_waves(int kta) { return kta == 0 ? 2 : 1; }
constexpr int trunk_bwd_waves(int kta) { return kta == 0 ? 2 : 1; }
constexpr int embed_bwd_waves = 1;

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int v = 0; v < 16; v++) z[v] = 0.f;
    return z;
}
__device__ __forceinline__ f32x16 relu16(f32x16 t) {
#pragma unroll
    for (int v = 0; v < 16; v++) t[v] = fmaxf(t[v], 0.f);
    return t;
}
// g where y > 0, else 0
__device__ __forceinline__ f32x16 mask16(f32x16 g, f32x16 y) {
#pragma unroll
    for (int v = 0; v < 16; v++) g[v] = y[v] > 0.f ? g[v] : 0.f;
    return g;
}

// ---- global <-> tile (lane = (r = row, hh), register v = feature c0 + 8 (v / 4) + 4 hh + v % 4) -------------------------------------
// wide: ld and c0 multiples of 4, the whole 32-feature tile inside the row.
// STRAIGHT: rows past the end load row 0 and are zeroed afterwards instead of branching around the load.  A branch makes the compiler
// fall back to s_waitcnt vmcnt(0) at the join, which waits for the prefetch of the NEXT tile in every iteration (SQ_WAIT_ANY 15-25 %
// of the wave time): the forward kernels gain 12-15 % from the straight form.  (The backward kernels lost as much with it when this was written --
// the product behind the load put the wait AT the load -- and kept the branch until round 5: they now use load_tile_raw / mask_tile below.)
// `width` (a multiple of 4): columns >= width do not exist and read as 0 (the last tile of a narrow xa)
// Plain loads and stores (round 5, measured): the [N, 64..128] activation / gradient streams of these kernels are each far larger than the 256 MiB
// Infinity Cache and are touched once or twice per step, but nontemporal accesses on these 16-byte pieces of rows cost 1.1 ms of the fine-stage step
// (hexplane.hip keeps the hint for its whole-row streams).  ld4 is a plain forwarder and stays one: with the load spelt out in load_tile's guarded arm the
// compiler orders the backward kernels that use that arm (GO = 2, MULTI) differently.
__device__ __forceinline__ float4 ld4(const float* p) { return *(const float4*)p; }
template <bool STRAIGHT = false>
__device__ __forceinline__ f32x16 load_tile(const float* __restrict__ src, size_t ld, size_t row, bool ok, int c0, int hh, int width = 1 << 30) {
    f32x16 t;
    if (STRAIGHT) {
        const float* p = src + (ok ? row : 0) * ld;
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const int c = c0 + 8 * a + 4 * hh;
            const bool in = c < width;
            const float4 q = ld4(p + (in ? c : 0));
            const float keep = (ok && in) ? 1.f : 0.f;
            t[4 * a] = q.x * keep; t[4 * a + 1] = q.y * keep; t[4 * a + 2] = q.z * keep; t[4 * a + 3] = q.w * keep;
        }
    } else {
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const int c = c0 + 8 * a + 4 * hh;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok && c < width) q = ld4(src + row * ld + c);
            t[4 * a] = q.x; t[4 * a + 1] = q.y; t[4 * a + 2] = q.z; t[4 * a + 3] = q.w;
        }
    }
    return t;
}
// any width: features >= width read as 0
__device__ __forceinline__ f32x16 load_tile_narrow(const float* __restrict__ src, int width, size_t row, bool ok, int c0, int hh) {
    f32x16 t;
#pragma unroll
    for (int v = 0; v < 16; v++) {
        const int f = c0 + 8 * (v >> 2) + 4 * hh + (v & 3);
        t[v] = (ok && f < width) ? src[row * (size_t)width + f] : 0.f;
    }
    return t;
}
__device__ __forceinline__ void store_tile(float* __restrict__ dst, size_t ld, size_t row, bool ok, int c0, int hh, f32x16 t, int width = 1 << 30) {
    if (!ok) return;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int c = c0 + 8 * a + 4 * hh;
        if (c < width) *(float4*)(dst + row * ld + c) = make_float4(t[4 * a], t[4 * a + 1], t[4 * a + 2], t[4 * a + 3]);
    }
}
__device__ __forceinline__ void store_tile_narrow(float* __restrict__ dst, int width, size_t row, bool ok, int c0, int hh, f32x16 t) {
    if (!ok) return;
#pragma unroll
    for (int v = 0; v < 16; v++) {
        const int f = c0 + 8 * (v >> 2) + 4 * hh + (v & 3);
        if (f < width) dst[row * (size_t)width + f] = t[v];
    }
}

// RAW tile loads for the backward kernels' loop-carried prefetches (round 5).  A guarded load (a branch around it, or a select / product right behind
// it) makes the compiler wait for the load where it is issued -- with `s_waitcnt vmcnt(0)`, i.e. for every other load in flight too: the head
// kernels stalled for a full HBM round trip at the top of every tile.  So: the caller clamps the row, columns >= width read column 0, nothing is
// masked here; the values travel raw across the loop iteration and are masked (mask_tile) where they are used.
__device__ __forceinline__ f32x16 load_tile_raw(const float* __restrict__ src, size_t ld, size_t row_c, int c0, int hh, int width = 1 << 30) {
    f32x16 t;
    const float* p = src + row_c * ld;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int c = c0 + 8 * a + 4 * hh;
        const float4 q = ld4(p + (c < width ? c : 0));
        t[4 * a] = q.x; t[4 * a + 1] = q.y; t[4 * a + 2] = q.z; t[4 * a + 3] = q.w;
    }
    return t;
}
__device__ __forceinline__ f32x16 mask_tile(f32x16 t, bool ok, int c0, int hh, int width) {
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const float keep = (ok && c0 + 8 * a + 4 * hh < width) ? 1.f : 0.f;
        t[4 * a] *= keep; t[4 * a + 1] *= keep; t[4 * a + 2] *= keep; t[4 * a + 3] *= keep;
    }
    return t;
}

// bias as the initial accumulator: register v of lane half hh holds feature c0 + 8 (v / 4) + 4 hh + v % 4
__device__ __forceinline__ f32x16 bias_tile(const float* __restrict__ b_lds, int c0, int hh) {
    f32x16 t;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const float4 q = *(const float4*)(b_lds + c0 + 8 * a + 4 * hh);
        t[4 * a] = q.x; t[4 * a + 1] = q.y; t[4 * a + 2] = q.z; t[4 * a + 3] = q.w;
    }
    return t;
}

// out[to] += W[32 to + r][k] in[k]: KT input tiles, NT output tiles; W in LDS, row stride `stride`, first input column `k0`.
// NA < 4: only the first NA 8-feature chunks of an input tile are non-zero.
// The backward's data path is the same function on the TRANSPOSED weights (a second LDS image, [in][out]): reading W column-wise
// instead needs one ds_read_b32 per MFMA, which a wave with a full register file cannot prefetch -- the matrix pipe then waits for an
// LDS round trip per instruction (SQ_VALU_MFMA_BUSY_CYCLES was 53 % of the kernel time).
template <int KT, int NT, int NA = 4>
__device__ __forceinline__ void layer_fwd(f32x16 (&acc)[NT], const f32x16 (&in)[KT], const float* __restrict__ W, int stride, int k0, int r, int hh) {
#pragma unroll
    for (int kt = 0; kt < KT; kt++)
#pragma unroll
        for (int a = 0; a < NA; a++) {
            float4 w[NT];
#pragma unroll
            for (int to = 0; to < NT; to++) w[to] = *(const float4*)(W + (32 * to + r) * stride + k0 + 32 * kt + 8 * a + 4 * hh);
#pragma unroll
            for (int to = 0; to < NT; to++) {
                acc[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[to].x, in[kt][4 * a], acc[to], 0, 0, 0);
                acc[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[to].y, in[kt][4 * a + 1], acc[to], 0, 0, 0);
                acc[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[to].z, in[kt][4 * a + 2], acc[to], 0, 0, 0);
                acc[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[to].w, in[kt][4 * a + 3], acc[to], 0, 0, 0);
            }
        }
}

// ---- split-bf16 MFMA (round 4) ---------------------------------------------------------------------------------------------------------
// fp32 MFMA runs at 1/16 of the bf16 rate on gfx950.  A product of fp32 values is reproduced to fp32 accuracy from bf16 pieces:
//     x = x1 + x2 + x3 (three bf16 terms = 24 mantissa bits: exact), W x ~ W1 x1 + (W1 x2 + W2 x1) + (W1 x3 + W2 x2 + W3 x1)
// -- the six products above 2^-24 of the result; a bf16 x bf16 product is exact in fp32 and v_mfma_f32_32x32x16_bf16 accumulates in fp32.
// profiles/microbench_mfma_split_bf16.hip: the same error against float64 as the fp32 MFMA path (4.1e-7 of O(1) outputs after three
// layers) at 1.8x its rate, conversions included.  The data flow does not change: a tile's 16 registers of a lane are, in pairs of eight,
// exactly the eight consecutive k-positions the bf16 shape wants from that lane (k-block 0 = registers 0..7 of both lane halves = features
// {0-3, 8-11 | 4-7, 12-15} of the tile, k-block 1 = registers 8..15), so the accumulator of a layer is still the B operand of the next
// one after its registers have been split (5.5 vector instructions per value), and the weights are staged in LDS as ready-made A fragments:
//     image[term 0..2][out tile][k-block][lane] = uint4 of eight bf16 = term(M[32 tile + lane % 32][feature(k-block, lane / 32, 0..7)])
// Per kernel (mode bit 0: the layers' products W x on split bf16, bit 1: the weight gradients' outer products): chosen from measurements at 2 M
// rows (profiles/r04_mlp_split_variants.txt) -- the split costs 176 vector instructions per 32 x 32 tile, which a kernel with few MFMAs per
// tile does not earn back.  The heads' modes are branch_mode's table; the trunk's xa block (KTA > 0) runs its forward in mode 1 and its backward in
// mode 3 (TrunkLds), the embedding-only trunk (KTA = 0) stays on fp32.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
struct Split { uint4 t[3][2]; };          // [term][k-block of the tile]
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const bf16x2 r = __builtin_convertvector((f32x2){a, b}, bf16x2);        // v_cvt_pk_bf16_f32: round to nearest even
    return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ void split2(float x0, float x1, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
    p1 = pack_bf16(x0, x1);
    const float r0 = x0 - __uint_as_float(p1 << 16), r1 = x1 - __uint_as_float(p1 & 0xffff0000u);         // exact residuals
    p2 = pack_bf16(r0, r1);
    const float s0 = r0 - __uint_as_float(p2 << 16), s1 = r1 - __uint_as_float(p2 & 0xffff0000u);
    p3 = pack_bf16(s0, s1);
}
__device__ __forceinline__ Split split_tile(const f32x16& x) {
    Split s;
#pragma unroll
    for (int kb = 0; kb < 2; kb++) {
        uint32_t p[3][4];
#pragma unroll
        for (int q = 0; q < 4; q++) split2(x[8 * kb + 2 * q], x[8 * kb + 2 * q + 1], p[0][q], p[1][q], p[2][q]);
#pragma unroll
        for (int m = 0; m < 3; m++) s.t[m][kb] = make_uint4(p[m][0], p[m][1], p[m][2], p[m][3]);
    }
    return s;
}
__device__ __forceinline__ f32x16 mfma_bf16(uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// the six products of one k-block, smallest first
__device__ __forceinline__ f32x16 mfma_split(f32x16 c, uint4 a1, uint4 a2, uint4 a3, uint4 b1, uint4 b2, uint4 b3) {
    c = mfma_bf16(a3, b1, c); c = mfma_bf16(a2, b2, c); c = mfma_bf16(a1, b3, c);
    c = mfma_bf16(a2, b1, c); c = mfma_bf16(a1, b2, c);
    return mfma_bf16(a1, b1, c);
}
// floats (4-byte units) of the image of a [32 NT][16 KB] matrix
constexpr int split_floats(int nt, int kb) { return 3 * nt * kb * 64 * 4; }
// layer_fwd on an image: acc[to] += M[32 to + .][k] in[k], k-blocks kb0 .. of the image (NB = k-blocks of an input tile that are non-zero)
template <int KT, int NT, int NB = 2>
__device__ __forceinline__ void layer_fwd_s(f32x16 (&acc)[NT], const f32x16 (&in)[KT], const uint4* __restrict__ img, int nt_img, int kb_img, int kb0, int lane) {
#pragma unroll
    for (int kt = 0; kt < KT; kt++) {
        const Split x = split_tile(in[kt]);
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const int kb = kb0 + 2 * kt + b;
#pragma unroll
            for (int to = 0; to < NT; to++) {
                const uint4 w1 = img[((0 * nt_img + to) * kb_img + kb) * 64 + lane], w2 = img[((1 * nt_img + to) * kb_img + kb) * 64 + lane],
                            w3 = img[((2 * nt_img + to) * kb_img + kb) * 64 + lane];
                acc[to] = mfma_split(acc[to], w1, w2, w3, x.t[0][b], x.t[1][b], x.t[2][b]);
            }
        }
    }
}
// M[o][f] = src[o ld + col0 + f] (o < rows, f < cols), or transposed: M[o][f] = src[f ld + col0 + o] (f < rows, o < cols); zero elsewhere
__device__ __forceinline__ void stage_split(float* __restrict__ dst_f, int nt_img, int kb_img, const float* __restrict__ src, int ld, int col0, int rows, int cols,
                                            bool transposed) {
    uint4* dst = reinterpret_cast<uint4*>(dst_f);
    const int total = nt_img * kb_img * 64;
    for (int idx = threadIdx.x; idx < total; idx += MLP_THREADS) {
        const int ln = idx & 63, kb = (idx >> 6) % kb_img, to = (idx >> 6) / kb_img, hh = ln >> 5, o = 32 * to + (ln & 31);
        float w[8];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const int v = 8 * (kb & 1) + t, f = 32 * (kb >> 1) + 8 * (v >> 2) + 4 * hh + (v & 3);
            const bool in = src && (transposed ? (f < rows && o < cols) : (o < rows && f < cols));
            w[t] = in ? (transposed ? src[(size_t)f * ld + col0 + o] : src[(size_t)o * ld + col0 + f]) : 0.f;
        }
        uint32_t p[3][4];
#pragma unroll
        for (int q = 0; q < 4; q++) split2(w[2 * q], w[2 * q + 1], p[0][q], p[1][q], p[2][q]);
#pragma unroll
        for (int m = 0; m < 3; m++) dst[((m * nt_img + to) * kb_img + kb) * 64 + ln] = make_uint4(p[m][0], p[m][1], p[m][2], p[m][3]);
    }
}
// dW += gf (x) af over the 32 rows of the fragments (registers 0..7 / 8..15 of both lane halves = the two k-blocks), split the same way
__device__ __forceinline__ f32x16 outer_acc_s(f32x16 acc, const Split& g, const Split& a) {
#pragma unroll
    for (int b = 0; b < 2; b++) acc = mfma_split(acc, g.t[0][b], g.t[1][b], g.t[2][b], a.t[0][b], a.t[1][b], a.t[2][b]);
    return acc;
}

// ---- transposed fragments for the weight gradients -------------------------------------------------------------------------------
// tile (lane = row, registers = features) -> fragment (lane r = feature, registers = the 16 rows 16 hh .. 16 hh + 15) through the wave's
// private LDS scratch.  LDS serves the DS instructions of one wave in order, so the reads see the writes; the fences only pin the
// compiler's order.
__device__ __forceinline__ f32x16 transpose_tile(f32x16 t, float* __restrict__ T, int r, int hh) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int v = 0; v < 16; v++) T[(8 * (v >> 2) + 4 * hh + (v & 3)) * TS + r] = t[v];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    f32x16 f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float4 q = *(const float4*)(T + r * TS + 16 * hh + 4 * i);
        f[4 * i] = q.x; f[4 * i + 1] = q.y; f[4 * i + 2] = q.z; f[4 * i + 3] = q.w;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return f;
}
__device__ __forceinline__ float frag_sum(f32x16 f) {
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < 16; v++) s += f[v];
    return s;
}
// dW[32 to + o][32 ti + i] += sum_rows gf[o][row] af[i][row]: both operands as fragments; the k-step s pairs row s (lanes 0-31)
// with row 16 + s (lanes 32-63) on both sides
__device__ __forceinline__ f32x16 outer_acc(f32x16 acc, f32x16 gf, f32x16 af) {
#pragma unroll
    for (int s = 0; s < 16; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[s], af[s], acc, 0, 0, 0);
    return acc;
}
// accumulator tile D[o][i] (lane r = i, register v = o = 8 (v / 4) + 4 hh + v % 4) -> dW[(o0 + o) * ld + i0 + i], bounded
__device__ __forceinline__ void flush_dw(float* __restrict__ dW, int ld, int o0, int i0, int rows, int cols, f32x16 acc, int r, int hh) {
    if (!dW || i0 + r >= cols) return;
#pragma unroll
    for (int v = 0; v < 16; v++) {
        const int o = o0 + 8 * (v >> 2) + 4 * hh + (v & 3);
        if (o < rows) unsafeAtomicAdd(dW + (size_t)o * ld + i0 + r, acc[v]);
    }
}
// Sum an accumulator tile / a per-lane partial over the workgroup's waves through LDS (`buf`: (MLP_WAVES - 1) x 17 x 64 floats, the
// transpose scratch after the tile loop); the total is valid in wave 0, which alone issues the atomics: a quarter of the traffic onto
// the few thousand addresses every workgroup of the grid adds to at the same moment.
__device__ __forceinline__ f32x16 wg_sum16(f32x16 acc, float* __restrict__ buf, int wave, int lane) {
    __syncthreads();
    if (wave > 0) {
#pragma unroll
        for (int v = 0; v < 16; v++) buf[((wave - 1) * 17 + v) * 64 + lane] = acc[v];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 0; w < MLP_WAVES - 1; w++)
#pragma unroll
            for (int v = 0; v < 16; v++) acc[v] += buf[(w * 17 + v) * 64 + lane];
    }
    return acc;
}
__device__ __forceinline__ float wg_sum1(float x, float* __restrict__ buf, int wave, int lane) {
    __syncthreads();
    if (wave > 0) buf[((wave - 1) * 17 + 16) * 64 + lane] = x;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 0; w < MLP_WAVES - 1; w++) x += buf[(w * 17 + 16) * 64 + lane];
    }
    return x;
}

// per-lane bias-gradient partials (lane r = feature of the tile, both halves hold half of the rows) -> db[o0 + r]
__device__ __forceinline__ void flush_db(float* __restrict__ db, int o0, int rows, float part, int r) {
    if (db && o0 + r < rows) unsafeAtomicAdd(db + o0 + r, part);
}

// What becomes of a workgroup's total: the bodies (mlp_*_body.inc) call the `fl` object their kernel declares.
//   FlushAtomic  added onto the caller's zero-filled gradient with float atomics (mlp.hip): flush_dw / flush_db as they are.
//   FlushSlab    stored to slot blockIdx.x of the tensor's slab [gridDim.x][rows * cols] (mlp_det.hip; emd_mlp_det_reduce adds the slots in ascending
//                order).  The bounds are flush_dw's / flush_db's, so every workgroup writes every element of its slot, zeros included: the slab is never
//                cleared.  The destination pointer only says whether the gradient is wanted.
// `id`: the tensor's index in EmdMlpDetLayout (offset / pitch).
struct DetSlabs { float* p[EMD_MLP_DET_MAX_TENSORS]; };
struct FlushAtomic {
    __device__ __forceinline__ void dw(int, float* __restrict__ dW, int ld, int o0, int i0, int rows, int cols, f32x16 acc, int r, int hh) const {
        flush_dw(dW, ld, o0, i0, rows, cols, acc, r, hh);
    }
    __device__ __forceinline__ void db(int, float* __restrict__ db_, int o0, int rows, float part, int r) const { flush_db(db_, o0, rows, part, r); }
    // one element of a tensor (the embedding kernel's tail): `dst` its address in the gradient, `idx` / `pitch` its place in a slab slot
    __device__ __forceinline__ void one(int, float* dst, int, int, float s) const { unsafeAtomicAdd(dst, s); }
    // the workgroup's share of sum |out| (the head's forward)
    __device__ __forceinline__ void l1(float* l1_sum, float t, int num_points, int out_dim) const { atomicAdd(l1_sum, t / ((float)num_points * (float)out_dim)); }
};
struct FlushSlab {
    DetSlabs s;
    __device__ __forceinline__ void dw(int id, float* __restrict__ dW, int, int o0, int i0, int rows, int cols, f32x16 acc, int r, int hh) const {
        if (!dW || i0 + r >= cols) return;
        float* __restrict__ slot = s.p[id] + (size_t)blockIdx.x * rows * cols;
#pragma unroll
        for (int v = 0; v < 16; v++) {
            const int o = o0 + 8 * (v >> 2) + 4 * hh + (v & 3);
            if (o < rows) slot[o * cols + i0 + r] = acc[v];
        }
    }
    // (the two lane halves of wave 0 hold the two halves of the rows of feature r: the atomic flush adds both onto one address; here lanes 0-31 add
    //  the upper half's partial to their own -- a fixed order -- and store the sum.  Called by the whole of wave 0.)
    __device__ __forceinline__ void db(int id, float* __restrict__ db_, int o0, int rows, float part, int r) const {
        const float both = part + __shfl_xor(part, 32);
        if (db_ && o0 + r < rows && (threadIdx.x & 32) == 0) s.p[id][(size_t)blockIdx.x * rows + o0 + r] = both;
    }
    __device__ __forceinline__ void one(int id, float*, int idx, int pitch, float v) const { s.p[id][(size_t)blockIdx.x * pitch + idx] = v; }
    // (unscaled: the reduction multiplies the sum of the slots by 1 / (N out_dim) in double precision)
    __device__ __forceinline__ void l1(float*, float t, int, int) const { s.p[0][blockIdx.x] = t; }
};

// stage a [rows, cols] block of a row-major matrix (row stride ld, first column col0) into LDS [rows_pad][stride], zero padded.
// 16-byte pieces, four independent loads in flight per thread: the one-dword-at-a-time loop this replaces spent 30-50 us per launch
// on dependent load -> write round trips, 15 % of a forward kernel.
__device__ __forceinline__ void stage_matrix(float* __restrict__ dst, int stride, int rows_pad, int cols_pad, const float* __restrict__ src, int ld, int col0,
                                             int rows, int cols) {
    const bool vec = src && !(cols & 3) && !(ld & 3) && !(col0 & 3) && !(cols_pad & 3) && !(stride & 3) && !((uintptr_t)src & 15);
    if (vec) {
        const int q = cols_pad >> 2, total = rows_pad * q;
#pragma unroll 4
        for (int idx = threadIdx.x; idx < total; idx += MLP_THREADS) {
            const int rr = idx / q, c = (idx - rr * q) << 2;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rr < rows && c < cols) v = *(const float4*)(src + (size_t)rr * ld + col0 + c);
            *(float4*)(dst + rr * stride + c) = v;
        }
        return;
    }
#pragma unroll 4
    for (int idx = threadIdx.x; idx < rows_pad * cols_pad; idx += MLP_THREADS) {
        const int rr = idx / cols_pad, c = idx - rr * cols_pad;
        dst[rr * stride + c] = (src && rr < rows && c < cols) ? src[(size_t)rr * ld + col0 + c] : 0.f;
    }
}
// the transposed image: dst[c][rr] = src[rr][col0 + c] for rr < rows, c < cols; zero elsewhere in [cols_pad][rows_pad]
__device__ __forceinline__ void stage_matrix_t(float* __restrict__ dst, int stride, int rows_pad, int cols_pad, const float* __restrict__ src, int ld, int col0,
                                               int rows, int cols) {
#pragma unroll 4
    for (int idx = threadIdx.x; idx < rows_pad * cols_pad; idx += MLP_THREADS) {
        const int rr = idx / cols_pad, c = idx - rr * cols_pad;          // consecutive threads read consecutive source columns
        dst[c * stride + rr] = (src && rr < rows && c < cols) ? src[(size_t)rr * ld + col0 + c] : 0.f;
    }
}
__device__ __forceinline__ void stage_vector(float* __restrict__ dst, int n_pad, const float* __restrict__ src, int n) {
    for (int idx = threadIdx.x; idx < n_pad; idx += MLP_THREADS) dst[idx] = (src && idx < n) ? src[idx] : 0.f;
}

// The xb block is ONE k-chunk of 8: register j of lane half hh holds xb[row][4 hh + j].
// The heads that recompute h: the next tile's embedding values travel RAW across the loop iteration (clamped address, unconditional loads) and are
// masked where they are used -- masking at the load (a select, or a product) makes the compiler wait for the load right there, inside the tile loop.
__device__ __forceinline__ void load_xb_raw(const float* __restrict__ xb, int kb, size_t row, bool ok, int hh, float (&v)[4]) {
    const float* p = xb + (ok ? row : 0) * (size_t)kb;
#pragma unroll
    for (int j = 0; j < 4; j++) { const int c = 4 * hh + j; v[j] = p[c < kb ? c : 0]; }
}
__device__ __forceinline__ void mask_xb(const float (&raw)[4], int kb, bool ok, int hh, float (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = raw[j] * ((ok && 4 * hh + j < kb) ? 1.f : 0.f);
}
// h = b + Wb xb for one 32-row tile: the xb part of the trunk's forward (trunk_forward_tile with no xa block, the same MFMAs in the same order: the
// same bits), from the [64][12] image of Wb and the bias behind it -- used by the trunk kernel and by the heads that recompute h (EmdMlpBranch.xb)
__device__ __forceinline__ void embed_h(const float* __restrict__ wb, const float* __restrict__ b, int r, int hh, const float (&xb)[4], f32x16 (&h)[2], bool init = true) {
    if (init) { h[0] = bias_tile(b, 0, hh); h[1] = bias_tile(b, 32, hh); }
#pragma unroll
    for (int to = 0; to < 2; to++) {
        const float4 w = *(const float4*)(wb + (32 * to + r) * 12 + 4 * hh);
        h[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, xb[0], h[to], 0, 0, 0);
        h[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, xb[1], h[to], 0, 0, 0);
        h[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, xb[2], h[to], 0, 0, 0);
        h[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, xb[3], h[to], 0, 0, 0);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// branch: [relu] -> Linear(64, 64) -> relu [-> Linear(64, 64) -> relu] -> Linear(64, out_dim)
// ---------------------------------------------------------------------------------------------------------------------------------
// LDS (floats): W1 [64][WS] | W2 [64][WS] (DEPTH 2) | Wo [32 NTO][WS] | b1 [64] | b2 [64] | bo [64] | scratch [waves][32][TS] (backward)
// the split-bf16 mode of every head kernel (measurements: profiles/r04_mlp_split_variants.txt, docs/history/DESIGN_rounds_1-5.md)
constexpr int branch_mode(int depth, int nto, bool bwd) {
    // two hidden layers (the feature head): the forward runs both hidden layers on split bf16 (round 5, late); the BACKWARD keeps fp32 MFMA -- its six
    // images + transposes would need 167 KB of LDS, the forward has three images only
    if (depth != 1) return bwd ? 0 : 1;
    // one hidden layer, forward: products on split bf16 for one output tile (dx / do / feat heads) and for two (dshs).  One tile since round 5: with the
    // narrow output layer on the vector pipe the hidden layer is what is left on the matrix pipe, and there the split wins (fine stage 13.61 -> 13.46 ms;
    // before, the split cost more than it saved while a third of the MFMAs were a padded output tile)
    if (!bwd) return 1;
    // one hidden layer, backward: one output tile has the registers for split outer products too, two output tiles split the products only
    return nto == 1 ? 3 : 1;
}
template <int DEPTH, int NTO, int MODE = 0>
struct BranchLds {
    static constexpr bool SP = (MODE & 1) != 0;            // weights as split-bf16 images
    static constexpr bool SPO = (MODE & 2) != 0;           // outer products on split bf16
    static constexpr int W64 = SP ? split_floats(2, 4) : 64 * WS;                    // a 64 x 64 matrix
    static constexpr int w1 = 0;
    static constexpr int w2 = w1 + W64;
    static constexpr int wo = w2 + (DEPTH == 2 ? W64 : 0);
    static constexpr int b1 = wo + (SP ? split_floats(NTO, 4) : 32 * NTO * WS);
    static constexpr int b2 = b1 + 64;
    static constexpr int bo = b2 + 64;
    static constexpr int fwd_floats = bo + 64;
    // backward only: the transposed images W1^T [64][WS], W2^T, Wo^T [64][WOT] and one transpose tile per wave
    static constexpr int WOT = 32 * NTO + 4;
    static constexpr int w1t = fwd_floats;
    static constexpr int w2t = w1t + W64;
    static constexpr int wot = w2t + (DEPTH == 2 ? W64 : 0);
    static constexpr int scratch = wot + (SP ? split_floats(2, 2 * NTO) : 64 * WOT);
    static constexpr int bwd_floats = scratch + MLP_WAVES * 32 * TS;
    // RC kernels (the head recomputes h from the embedding): Win [64][12] | b_in [64] behind the kernel's other regions
    static constexpr int rc_floats = 64 * 12 + 64;
};

// one call for both weight forms: the fp32 path reads rows of a padded LDS matrix, the split path ready-made bf16 fragments
template <bool SP, int KT, int NT, int NA = 4>
__device__ __forceinline__ void mm(f32x16 (&acc)[NT], const f32x16 (&in)[KT], const float* __restrict__ W, int stride, int k0, int nt_img, int kb_img, int r, int hh,
                                   int lane) {
    if constexpr (SP) layer_fwd_s<KT, NT, (NA + 1) / 2>(acc, in, reinterpret_cast<const uint4*>(W), nt_img, kb_img, k0 / 16, lane);
    else layer_fwd<KT, NT, NA>(acc, in, W, stride, k0, r, hh);
}
// dW[t][i] += gf (x) af[i], i = 0 .. NI - 1 (the fragments are split once per call on the bf16 path)
template <bool SP, int NI>
__device__ __forceinline__ void outer_all(f32x16 (&dW)[NI], const f32x16& gf, const f32x16 (&af)[NI], const Split (&afs)[NI]) {
    if constexpr (SP) {
        const Split gs = split_tile(gf);
#pragma unroll
        for (int i = 0; i < NI; i++) dW[i] = outer_acc_s(dW[i], gs, afs[i]);
    } else {
#pragma unroll
        for (int i = 0; i < NI; i++) dW[i] = outer_acc(dW[i], gf, af[i]);
    }
}
template <bool SP, int NI>
__device__ __forceinline__ void split_all(Split (&afs)[NI], const f32x16 (&af)[NI]) {
    if constexpr (SP) {
#pragma unroll
        for (int i = 0; i < NI; i++) afs[i] = split_tile(af[i]);
    }
}

template <int DEPTH, int NTO, bool BWD, bool RC = false>
__device__ __forceinline__ void branch_stage(float* lds, const EmdMlpBranch& a) {
    typedef BranchLds<DEPTH, NTO, branch_mode(DEPTH, NTO, BWD)> L;
    if constexpr (RC) {      // the trunk's embedding block and bias, in the trunk kernel's own layout (trunk_stage)
        float* rc = lds + (BWD ? L::bwd_floats : L::fwd_floats);
        stage_matrix(rc, 12, 64, 8, a.w_in, a.ld_w_in, a.col_in, 64, a.kb_in);
        stage_vector(rc + 64 * 12, 64, a.b_in, 64);
    }
    if constexpr (L::SP) {
        if (BWD) {
            stage_split(lds + L::w1t, 2, 4, a.w_hidden[0], 64, 0, 64, 64, true);
            stage_split(lds + L::wot, 2, 2 * NTO, a.w_out, 64, 0, a.out_dim, 64, true);
        }
        stage_split(lds + L::w1, 2, 4, a.w_hidden[0], 64, 0, 64, 64, false);
        if (DEPTH == 2) stage_split(lds + L::w2, 2, 4, a.w_hidden[1], 64, 0, 64, 64, false);        // (forward only: branch_mode)
        // (a narrow output layer runs on the vector pipe in the forward and reads plain fp32 rows: they fit the image's allocation)
        if (!BWD && NTO == 1 && a.out_dim <= 4) stage_matrix(lds + L::wo, WS, 32, 64, a.w_out, 64, 0, a.out_dim, 64);
        else stage_split(lds + L::wo, NTO, 4, a.w_out, 64, 0, a.out_dim, 64, false);
    } else {
        if (BWD) {
            stage_matrix_t(lds + L::w1t, WS, 64, 64, a.w_hidden[0], 64, 0, 64, 64);
            if (DEPTH == 2) stage_matrix_t(lds + L::w2t, WS, 64, 64, a.w_hidden[1], 64, 0, 64, 64);
            stage_matrix_t(lds + L::wot, L::WOT, 32 * NTO, 64, a.w_out, 64, 0, a.out_dim, 64);
        }
        stage_matrix(lds + L::w1, WS, 64, 64, a.w_hidden[0], 64, 0, 64, 64);
        if (DEPTH == 2) stage_matrix(lds + L::w2, WS, 64, 64, a.w_hidden[1], 64, 0, 64, 64);
        stage_matrix(lds + L::wo, WS, 32 * NTO, 64, a.w_out, 64, 0, a.out_dim, 64);
    }
    stage_vector(lds + L::b1, 64, a.b_hidden[0], 64);
    stage_vector(lds + L::b2, 64, DEPTH == 2 ? a.b_hidden[1] : nullptr, 64);
    stage_vector(lds + L::bo, 64, a.b_out, a.out_dim);
    __syncthreads();
}

// L1: the head's regulariser mean |out| is formed beside the outputs (EmdMlpBranch.l1_sum); a separate instantiation keeps the registers of
// the usual kernels as they were
// RC: the head forms h = b_in + W_in xb itself (EmdMlpBranch.xb, a level without HexPlane features) instead of reading a [N,64] tensor
// (the body of the kernel: mlp_branch_fwd_body.inc, included by the kernels of mlp.hip and mlp_det.hip)

// GO: how dL/dout reaches the kernel.  0: at most four outputs (dx / do heads, NTO = 1): four raw values per row; 1: out_dim a multiple of 4
// (dshs: 48): raw 16-byte pieces, a partial tile masked by whole pieces; 2: any width (guarded loads, masked at the load: the old path)
// CHAIN (GO 0 / 1): g_h_in is present.  A runtime branch around a group of loads would do: but then the number of loads in flight differs between the
// paths, the compiler's wait for the PREVIOUS iteration's prefetch has to assume the smaller one, and that wait lands on the loads just issued.
// GO 0 / 1 therefore take every such decision at compile time (and need g_out; without it the launcher picks GO 2).
// (the body of the kernel: mlp_branch_bwd_body.inc, included by the kernels of mlp.hip and mlp_det.hip)

// ---------------------------------------------------------------------------------------------------------------------------------
// trunk: h = b + W[:, col_a : col_a + ka] xa + W[:, col_b : col_b + kb] xb           (ka = 32 KTA, kb <= 8)
// ---------------------------------------------------------------------------------------------------------------------------------
// LDS: Wa (split-bf16 image of [64][32 KTA]; nothing for KTA = 0) | Wb [64][12] | b [64] | scratch (backward)
// The xa block runs on split bf16 -- the products in both directions and the backward's outer products (profiles/r04_mlp_split_variants.txt) -- , the
// embedding block and the embedding-only trunk (KTA = 0) on fp32 MFMA.
template <int KTA>
struct TrunkLds {
    static constexpr int wa = 0;
    static constexpr int wb = wa + split_floats(2, 2 * KTA);
    static constexpr int b = wb + 64 * 12;
    static constexpr int fwd_floats = b + 64;
    // backward: only the transposed images Wa^T (split bf16), Wb^T [32][WS] (rows >= kb zero) and one transpose tile per wave
    static constexpr int wat = 0;
    static constexpr int wbt = wat + split_floats(KTA, 4);
    static constexpr int scratch = wbt + 32 * WS;
    static constexpr int bwd_floats = scratch + MLP_WAVES * 32 * TS;
};

template <int KTA>
__device__ __forceinline__ void trunk_stage(float* lds, const EmdMlpTrunk& a) {
    typedef TrunkLds<KTA> L;
    if (KTA) stage_split(lds + L::wa, 2, 2 * KTA, a.w, a.ld_w, a.col_a, 64, a.ka, false);
    stage_matrix(lds + L::wb, 12, 64, 8, a.kb > 0 ? a.w : nullptr, a.ld_w, a.col_b, 64, a.kb);
    stage_vector(lds + L::b, 64, a.b, 64);
    __syncthreads();
}

// this tile's xa / xb rows (already in registers) -> h
template <int KTA>
__device__ __forceinline__ void trunk_forward_tile(const float* lds, int r, int hh, const f32x16 (&xa)[KTA ? KTA : 1], const float (&xb)[4], f32x16 (&h)[2]) {
    typedef TrunkLds<KTA> L;
    h[0] = bias_tile(lds + L::b, 0, hh); h[1] = bias_tile(lds + L::b, 32, hh);
    if constexpr (KTA > 0) layer_fwd_s<KTA, 2>(h, xa, reinterpret_cast<const uint4*>(lds + L::wa), 2, 2 * KTA, 0, r + 32 * hh);
    embed_h(lds + L::wb, lds + L::b, r, hh, xb, h, false);
}

// raw rows for the forward's prefetch: clamped row, a column past the width reads column 0 (its weights are zero: the staged images are zero padded);
// nothing is masked -- the rows past the end are not stored
template <int KTA>
__device__ __forceinline__ void trunk_load_x_raw(const EmdMlpTrunk& a, size_t row_c, int hh, f32x16 (&xa)[KTA ? KTA : 1], float (&xb)[4]) {
    if (KTA) {
#pragma unroll
        for (int t = 0; t < KTA; t++) xa[t] = load_tile_raw(a.xa, a.ka, row_c, 32 * t, hh, a.ka);
    }
    if (a.kb > 0) {
#pragma unroll
        for (int j = 0; j < 4; j++) xb[j] = a.xb[row_c * (size_t)a.kb + (4 * hh + j < a.kb ? 4 * hh + j : 0)];
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) xb[j] = 0.f;
    }
}

// The loop's loads (round 5): dL/dh of the NEXT tile is the prefetch (32 registers; it is the first thing a tile needs), xa / xb of THIS tile are
// requested at the top of the iteration and first read after the dL/dxa product (96 MFMAs later) -- before, xa / xb of the next tile travelled (64
// registers) while dL/dh was loaded and waited for in place, a full HBM round trip per tile.  All of them raw and unconditional (load_tile_raw): rows
// past the end read row 0, and dL/dh is zeroed for them where it is used, which zeroes all they could add.  MULTI: more than one dL/dh tensor (a
// two-hidden-layer head keeps its own): the others are loaded inside the loop, guarded as before.
// (the body of the kernel: mlp_trunk_bwd_body.inc, included by the kernels of mlp.hip and mlp_det.hip)

// ---------------------------------------------------------------------------------------------------------------------------------
// trunk backward of a level WITHOUT HexPlane features (ka = 0, kb <= 4) on the vector pipe (round 5).  The MFMA form above pads the [64 x kb]
// weight gradient and the [kb]-wide dL/dxb to 32-column tiles: 64 fp32 MFMAs + three LDS transposes per 32 rows for 2 x 64 x kb x 32 useful
// multiply-adds, 244 us at 2 M rows while the kernel's only real traffic, the heads' dL/dh, is 512 MB.  Here a lane keeps the tile layout of its
// row (32 of the row's 64 features), forms its share of dL/dxb as kb x 32 multiply-adds against broadcast LDS rows (the halves meet in one
// cross-lane add) and keeps dWb[feature][c] += dL/dh[feature] xb[c] and db[feature] += dL/dh[feature] in 32 (kb + 1) per-lane accumulators that
// are summed over the lanes once, at the end: no MFMA, no transpose, bound by the read of dL/dh.
// ---------------------------------------------------------------------------------------------------------------------------------
// One wave per SIMD: the 512-entry register file holds the lane's 32 x kb weights (no LDS round trip in the tile loop), the 32 (kb + 1)
// accumulators and the next two tiles' registers (8 KB per wave and tile; the rotation's register copy waits for the nearer one).  Every load of
// the loop is unconditional (rows past the end read row 0 and are zeroed by load_tile's product; xb of such a row meets a zero dL/dh): a guarded load
// makes the compiler wait for ALL outstanding loads -- the prefetches too -- at the join.  MULTI: more than one dL/dh tensor (a two-hidden-layer head
// keeps its own): the others are added inside the loop.
// (the body of the kernel: mlp_embed_bwd_body.inc, included by the kernels of mlp.hip and mlp_det.hip)

unsigned mlp_grid(int num_points, int per_cu) {
    const size_t tiles = ((size_t)num_points + 31) / 32;
    const size_t wgs = (tiles + MLP_WAVES - 1) / MLP_WAVES, cap = (size_t)256 * per_cu;
    return (unsigned)(wgs < cap ? (wgs ? wgs : 1) : cap);          // persistent: `per_cu` workgroups per CU (their LDS holds the weights)
}

int check_branch(const EmdMlpBranch* a, const char* who) {
    if (!a) { emd_set_error("%s: null args", who); return EMD_ERR_INVALID; }
    if (a->num_points < 0 || (a->depth != 1 && a->depth != 2) || a->out_dim < 1 || a->out_dim > 64) {
        emd_set_error("%s: bad sizes (depth 1..2, out_dim 1..64)", who); return EMD_ERR_INVALID;
    }
    if (a->num_points == 0) return EMD_OK;
    if ((!a->h && !a->xb) || !a->w_hidden[0] || !a->b_hidden[0] || !a->w_out || !a->b_out || (a->depth == 2 && (!a->w_hidden[1] || !a->b_hidden[1]))) {
        emd_set_error("%s: null pointer", who); return EMD_ERR_INVALID;
    }
    if (a->xb) {          // the head recomputes h from the embedding (ABI 26)
        if (a->depth != 1) { emd_set_error("%s: xb (recomputed h) is served for depth 1 only", who); return EMD_ERR_INVALID; }
        if (!a->w_in || !a->b_in || a->kb_in < 1 || a->kb_in > 8 || a->col_in < 0 || a->ld_w_in < a->col_in + a->kb_in) {
            emd_set_error("%s: xb needs w_in, b_in, kb_in 1..8 and col_in + kb_in <= ld_w_in", who); return EMD_ERR_INVALID;
        }
    } else if (((uintptr_t)a->h & 15)) { emd_set_error("%s: h must be 16-byte aligned", who); return EMD_ERR_INVALID; }
    return EMD_OK;
}

int check_trunk(const EmdMlpTrunk* a, const char* who, bool need_h = true) {
    if (!a) { emd_set_error("%s: null args", who); return EMD_ERR_INVALID; }
    if (a->num_points < 0 || (a->ka < 0 || a->ka > 128 || (a->ka & 3)) || a->kb < 0 || a->kb > 8 || a->ka + a->kb == 0 || a->ld_w < a->ka + a->kb ||
        a->col_a < 0 || a->col_b < 0 || a->col_a + a->ka > a->ld_w || a->col_b + a->kb > a->ld_w) {
        emd_set_error("%s: bad sizes (ka a multiple of 4 up to 128, kb <= 8)", who); return EMD_ERR_INVALID;
    }
    if (a->num_points == 0) return EMD_OK;
    if (!a->w || !a->b || (need_h && !a->h) || (a->ka && !a->xa) || (a->kb && !a->xb)) { emd_set_error("%s: null pointer", who); return EMD_ERR_INVALID; }
    if ((need_h && ((uintptr_t)a->h & 15)) || (a->ka && ((uintptr_t)a->xa & 15))) { emd_set_error("%s: xa / h must be 16-byte aligned", who); return EMD_ERR_INVALID; }
    return EMD_OK;
}

template <auto kernel, int PER_CU, typename... Args>
int mlp_launch(int floats, int num_points, hipStream_t st, Args... args) {
    const size_t bytes = (size_t)floats * sizeof(float);
    if (bytes > 64 * 1024) {
        // once per kernel (this function template is instantiated per kernel: the kernel is its template argument): not a stream operation, so it is kept
        // out of the per-launch path and out of any stream capture after the first call
        // (the attribute is per DEVICE: one flag per device ordinal; an unsynchronised double set by two threads is harmless)
        static std::atomic<bool> raised[64];
        int dev = 0;
        EMD_HIP_CHECK(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64 || !raised[dev].load(std::memory_order_acquire)) {
            EMD_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
            if (dev >= 0 && dev < 64) raised[dev].store(true, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(kernel, dim3(mlp_grid(num_points, PER_CU)), dim3(MLP_THREADS), bytes, st, args...);
    EMD_LAUNCH_CHECK();
    return EMD_OK;
}

// ---- the refusals and the dispatch of the entry points: ONE function each for mlp.hip and mlp_det.hip ---------------------------------------
// A dispatch turns the runtime shape of a call into the kernel's template arguments (with_bool / with_int: common.h); the LDS floats, the recomputed-h
// addend and the workgroups per CU follow from those arguments.  A combination the checks refuse or the rules never choose is pruned with
// `if constexpr`: no kernel is instantiated for it.  `K` names the unit's kernels as constexpr pointers -- K::branch_fwd<DEPTH, NTO, L1, RC>,
// K::branch_bwd<DEPTH, NTO, L1, RC, GO, CHAIN>, K::trunk_bwd<KTA, MULTI>, K::embed_bwd<KB, MULTI> --, `extra` is what they take behind the default
// kernels' arguments (nothing; the slab pointers).
int check_branch_forward(const EmdMlpBranch* a, const char* who) {
    int rc = check_branch(a, who);
    if (rc || a->num_points == 0) return rc;
    if (!a->out) { emd_set_error("%s: null output", who); return EMD_ERR_INVALID; }
    return EMD_OK;
}

int check_branch_backward(const EmdMlpBranch* a, const EmdMlpBranchGrads* g, const char* who) {
    int rc = check_branch(a, who);
    if (rc || a->num_points == 0) return rc;
    if (!g || (!g->g_out && !g->l1_grad) || !g->g_h) { emd_set_error("%s: null gradient pointer", who); return EMD_ERR_INVALID; }
    if (g->g_h_in && a->depth != 1) { emd_set_error("%s: g_h_in is served for depth 1 only", who); return EMD_ERR_INVALID; }
    if (g->g_h_in && ((uintptr_t)g->g_h_in & 15)) { emd_set_error("%s: g_h_in must be 16-byte aligned", who); return EMD_ERR_INVALID; }
    if (g->l1_grad && !g->out) { emd_set_error("%s: l1_grad needs the forward's output tensor", who); return EMD_ERR_INVALID; }
    if (((uintptr_t)g->g_h & 15)) { emd_set_error("%s: g_h must be 16-byte aligned", who); return EMD_ERR_INVALID; }
    if (!(a->out_dim & 3) && (((uintptr_t)g->g_out & 15) || ((uintptr_t)g->out & 15))) {
        emd_set_error("%s: g_out / out must be 16-byte aligned when out_dim is a multiple of 4", who); return EMD_ERR_INVALID;
    }
    return EMD_OK;
}

int check_trunk_backward(const EmdMlpTrunk* a, const EmdMlpTrunkGrads* g, const char* who) {
    int rc = check_trunk(a, who, false);          // (the backward reads xa, xb and the heads' dL/dh, not h)
    if (rc || a->num_points == 0) return rc;
    if (!g || g->num_gh < 1 || g->num_gh > EMD_MLP_MAX_BRANCHES) { emd_set_error("%s: 1..%d gradient contributions", who, EMD_MLP_MAX_BRANCHES); return EMD_ERR_INVALID; }
    for (int k = 0; k < g->num_gh; k++)
        if (!g->g_h[k] || ((uintptr_t)g->g_h[k] & 15)) { emd_set_error("%s: g_h[%d] null or unaligned", who, k); return EMD_ERR_INVALID; }
    if (g->d_xa && ((uintptr_t)g->d_xa & 15)) { emd_set_error("%s: d_xa must be 16-byte aligned", who); return EMD_ERR_INVALID; }
    return EMD_OK;
}

// the embedding alone, at the reference's width and in whole 16-byte rows: its own kernel (static LDS)
bool trunk_backward_is_embed(const EmdMlpTrunk* a, const EmdMlpTrunkGrads* g) {
    return a->ka == 0 && a->kb == 4 && !((uintptr_t)a->xb & 15) && !((uintptr_t)g->d_xb & 15);
}
// workgroups per CU of the kernel a call is served by (-> mlp_grid: the number of slab slots of the deterministic forms)
int branch_forward_per_cu(const EmdMlpBranch* a) { return branch_fwd_waves(a->depth, a->out_dim > 32 ? 2 : 1); }
int trunk_backward_per_cu(const EmdMlpTrunk* a, const EmdMlpTrunkGrads* g) {
    return trunk_backward_is_embed(a, g) ? embed_bwd_waves : trunk_bwd_waves((a->ka + 31) / 32);
}

// (checked by the caller: check_branch_forward; L1_ONLY: the unit has the L1 forms only)
template <class K, bool L1_ONLY, typename... Extra>
int branch_forward_dispatch(const EmdMlpBranch* a, hipStream_t st, Extra... extra) {
    return with_int<1, 2>(a->depth, [&](auto d) { return with_int<1, 2>(a->out_dim > 32 ? 2 : 1, [&](auto t) {
        return with_bool(L1_ONLY || a->l1_sum != nullptr, [&](auto l) { return with_bool(a->xb != nullptr, [&](auto r) -> int {
            constexpr int DEPTH = decltype(d)::value, NTO = decltype(t)::value;
            constexpr bool L1 = decltype(l)::value, RC = decltype(r)::value;
            if constexpr ((DEPTH == 2 && RC) || (L1_ONLY && !L1)) return EMD_ERR_INVALID;          // recomputed h: one hidden layer (check_branch)
            else {
                typedef BranchLds<DEPTH, NTO, branch_mode(DEPTH, NTO, false)> L;
                return mlp_launch<K::template branch_fwd<DEPTH, NTO, L1, RC>, branch_fwd_waves(DEPTH, NTO)>(L::fwd_floats + (RC ? L::rc_floats : 0), a->num_points, st, *a,
                                                                                                             extra...);
            }
        }); });
    }); });
}

// (checked by the caller: check_branch_backward)
template <class K, typename... Extra>
int branch_backward_dispatch(const EmdMlpBranch* a, const EmdMlpBranchGrads* g, hipStream_t st, Extra... extra) {
    const int nto = a->out_dim > 32 ? 2 : 1;
    // THE rule for k_mlp_branch_bwd's GO / CHAIN.  GO, the form dL/dout is loaded in: 0 for at most four outputs in one tile, 1 for out_dim a multiple of
    // 4, 2 (guarded loads) otherwise or without g_out.  CHAIN, the chained dL/dh as a template argument: the raw-load forms only (GO 2 tests g_h_in itself).
    const int go = !g->g_out ? 2 : (nto == 1 && a->out_dim <= 4) ? 0 : (a->out_dim & 3) == 0 ? 1 : 2;
    const bool chain = g->g_h_in != nullptr && go != 2;
    return with_int<1, 2>(a->depth, [&](auto d) { return with_int<1, 2>(nto, [&](auto t) { return with_bool(g->l1_grad != nullptr, [&](auto l) {
        return with_bool(a->xb != nullptr, [&](auto r) { return with_int<0, 2>(go, [&](auto f) { return with_bool(chain, [&](auto c) -> int {
            constexpr int DEPTH = decltype(d)::value, NTO = decltype(t)::value, GO = decltype(f)::value;
            constexpr bool L1 = decltype(l)::value, RC = decltype(r)::value, CHAIN = decltype(c)::value;
            // two hidden layers: neither recomputed h (check_branch) nor g_h_in (above); GO 0 is one tile; GO 2 has no CHAIN form
            if constexpr ((DEPTH == 2 && (RC || CHAIN)) || (GO == 0 && NTO == 2) || (GO == 2 && CHAIN)) return EMD_ERR_INVALID;
            else {
                typedef BranchLds<DEPTH, NTO, branch_mode(DEPTH, NTO, true)> L;
                return mlp_launch<K::template branch_bwd<DEPTH, NTO, L1, RC, GO, CHAIN>, branch_bwd_waves>(L::bwd_floats + (RC ? L::rc_floats : 0), a->num_points, st, *a, *g,
                                                                                                              extra...);
            }
        }); }); });
    }); }); });
}

// (checked by the caller: check_trunk_backward)
template <class K, typename... Extra>
int trunk_backward_dispatch(const EmdMlpTrunk* a, const EmdMlpTrunkGrads* g, hipStream_t st, Extra... extra) {
    const bool embed = trunk_backward_is_embed(a, g);
    return with_bool(g->num_gh != 1, [&](auto m) {
        constexpr bool MULTI = decltype(m)::value;
        if (embed) return mlp_launch<K::template embed_bwd<4, MULTI>, embed_bwd_waves>(0, a->num_points, st, *a, *g, extra...);
        return with_int<0, 4>((a->ka + 31) / 32, [&](auto k) {
            constexpr int KTA = decltype(k)::value;
            return mlp_launch<K::template trunk_bwd<KTA, MULTI>, trunk_bwd_waves(KTA)>(TrunkLds<KTA>::bwd_floats, a->num_points, st, *a, *g, extra...);
        });
    });
}

}  // namespace
