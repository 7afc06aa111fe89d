// mlp.hip -- the width-64 MLPs of the EMD deformation network as fused fp32-MFMA kernels.
//
//   trunk   h = b + W[:, a-block] xa + W[:, b-block] xb                 S3Gaussian/scene/deformation.py:100-112,254-296 (feature_out,
//           (xa = HexPlane features [N,128] or nothing, xb = the per-Gaussian embedding [N,4]; the temporal row is the same for
//           every Gaussian and arrives folded into b)                   defor_depth = 1: one Linear)
//   branch  out = W_o act(W_2 act(W_1 in + b_1) + b_2) + b_o             :113-185,298-337 (pos / scales / rotations / opacity / shs
//           in = relu(h) for the deformation heads (one hidden layer),    heads: nn.Sequential(ReLU, Linear, ReLU, Linear); dino_head:
//           in = h for the feature head (two hidden layers)               Linear, ReLU, Linear, ReLU, Linear on the un-rectified h)
//
// The reference runs these as ~12 cuBLAS GEMMs per level plus one element-wise launch per bias / ReLU / slice, forward and backward;
// over 2 M Gaussians the [N, 64..192] intermediates cross HBM ~40 times per step.  Here a wave owns 32 Gaussians and keeps every
// intermediate in registers:
//   * `v_mfma_f32_32x32x2_f32` (exact fp32: a k-ordered fmaf chain) with the DATA ROWS on the N dimension: A = weights [out feature x k]
//     from LDS (one ds_read_b128 per four MFMAs, row stride 68 = 4 x odd floats: conflict-free), B = activations [k x row].  The
//     accumulator tile of a layer (lane = row, registers = features 8(v/4) + 4(lane/32) + v%4) IS the B operand of the next layer, register v
//     for k-step v -- the contraction order is free, so the weights are simply read in the same permuted k order: no lane movement,
//     no LDS round trip between layers.  The backward's data path (W^T g) reads the same LDS weights column-wise.
//   * weight gradients dW[o][i] = sum_rows g[o][row] act[i][row] contract over the rows, i.e. over the LANE index of both tiles: each
//     tile takes one wave-private trip through LDS (16 ds_write_b32, 4 ds_read_b128) that leaves it with lane = feature and its 16
//     registers = the data rows 16(lane/32) .. +15, which is an MFMA operand again; dW accumulates in registers over all tiles of the
//     wave and is added to HBM once per wave with float atomics.  Bias gradients are the row sums of the same fragments.
//   * the ReLU masks, bias adds and the sum over the heads' contributions to dL/dh ride in registers.
// HBM traffic per Gaussian and level: x (528 B) + h (256 B) + outputs forward; h, g_out, one g_h per branch, g_x backward.
// Bound: fp32 MFMA (157 TFLOP/s); no kernel here waits on HBM.
// The helpers, the argument checks and the dispatch live in mlp_kernels.h and the kernels' bodies in mlp_*_body.inc, shared with the deterministic forms of
// mlp_det.hip; the kernels of THIS unit flush a workgroup's totals with float atomics (FlushAtomic) and keep the symbols and the
// machine code they always had.
#include "mlp_kernels.h"

namespace {

// (what the template arguments mean: beside the bodies' places in mlp_kernels.h)
template <int DEPTH, int NTO, bool L1 = false, bool RC = false>
__global__ void __launch_bounds__(MLP_THREADS) MLP_OCC(branch_fwd_waves(DEPTH, NTO)) k_mlp_branch_fwd(EmdMlpBranch a) {
    const FlushAtomic fl{};
#include "mlp_branch_fwd_body.inc"
}

template <int DEPTH, int NTO, bool L1 = false, bool RC = false, int GO = 2, bool CHAIN = false>
__global__ void __launch_bounds__(MLP_THREADS) MLP_OCC(branch_bwd_waves) k_mlp_branch_bwd(EmdMlpBranch a, EmdMlpBranchGrads g) {
    const FlushAtomic fl{};
#include "mlp_branch_bwd_body.inc"
}

template <int KTA>
__global__ void __launch_bounds__(MLP_THREADS) MLP_OCC(trunk_fwd_waves(KTA)) k_mlp_trunk_fwd(EmdMlpTrunk a) {
    extern __shared__ float lds[];
    trunk_stage<KTA>(lds, a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
    const size_t N = (size_t)a.num_points, tiles = (N + 31) / 32;
    const size_t tile0 = (size_t)blockIdx.x * MLP_WAVES + wave, tstep = (size_t)gridDim.x * MLP_WAVES;
    // the next tile's rows are loaded while this tile computes (one wave per SIMD: nothing else hides the HBM latency)
    f32x16 nxa[KTA ? KTA : 1];
    float nxb[4];
    trunk_load_x_raw<KTA>(a, tile0 * 32 + r < N ? tile0 * 32 + r : 0, hh, nxa, nxb);
    for (size_t tile = tile0; tile < tiles; tile += tstep) {
        const size_t row = tile * 32 + r;
        const bool ok = row < N;
        f32x16 xa[KTA ? KTA : 1], h[2];
        float xb[4];
#pragma unroll
        for (int t = 0; t < (KTA ? KTA : 1); t++) xa[t] = nxa[t];
#pragma unroll
        for (int j = 0; j < 4; j++) xb[j] = nxb[j];
        {
            const size_t nrow = (tile + tstep) * 32 + r;
            trunk_load_x_raw<KTA>(a, nrow < N ? nrow : 0, hh, nxa, nxb);
        }
        trunk_forward_tile<KTA>(lds, r, hh, xa, xb, h);
        store_tile(a.h, 64, row, ok, 0, hh, h[0]);
        store_tile(a.h, 64, row, ok, 32, hh, h[1]);
    }
}

template <int KTA, bool MULTI = false>
__global__ void __launch_bounds__(MLP_THREADS) MLP_OCC(trunk_bwd_waves(KTA)) k_mlp_trunk_bwd(EmdMlpTrunk a, EmdMlpTrunkGrads g) {
    const FlushAtomic fl{};
#include "mlp_trunk_bwd_body.inc"
}

template <int KB, bool MULTI>          // KB = kb = 4
__global__ void __launch_bounds__(MLP_THREADS) MLP_OCC(embed_bwd_waves) k_mlp_embed_bwd(EmdMlpTrunk a, EmdMlpTrunkGrads g) {
    const FlushAtomic fl{};
#include "mlp_embed_bwd_body.inc"
}

// this unit's kernels, as the shared dispatch names them
struct Kernels {
    template <int DEPTH, int NTO, bool L1, bool RC> static constexpr auto branch_fwd = &k_mlp_branch_fwd<DEPTH, NTO, L1, RC>;
    template <int DEPTH, int NTO, bool L1, bool RC, int GO, bool CHAIN> static constexpr auto branch_bwd = &k_mlp_branch_bwd<DEPTH, NTO, L1, RC, GO, CHAIN>;
    template <int KTA, bool MULTI> static constexpr auto trunk_bwd = &k_mlp_trunk_bwd<KTA, MULTI>;
    template <int KB, bool MULTI> static constexpr auto embed_bwd = &k_mlp_embed_bwd<KB, MULTI>;
};

}  // namespace

extern "C" int emd_mlp_branch_forward(const EmdMlpBranch* a, void* hip_stream) {
    int rc = check_branch_forward(a, "mlp_branch_forward");
    if (rc || a->num_points == 0) return rc;
    return branch_forward_dispatch<Kernels, false>(a, (hipStream_t)hip_stream);
}

extern "C" int emd_mlp_branch_backward(const EmdMlpBranch* a, const EmdMlpBranchGrads* g, void* hip_stream) {
    int rc = check_branch_backward(a, g, "mlp_branch_backward");
    if (rc || a->num_points == 0) return rc;
    return branch_backward_dispatch<Kernels>(a, g, (hipStream_t)hip_stream);
}

extern "C" int emd_mlp_trunk_forward(const EmdMlpTrunk* a, void* hip_stream) {
    int rc = check_trunk(a, "mlp_trunk_forward");
    if (rc || a->num_points == 0) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    return with_int<0, 4>((a->ka + 31) / 32, [&](auto k) {            // input tiles of 32 columns (the last one zero-padded)
        constexpr int KTA = decltype(k)::value;
        return mlp_launch<k_mlp_trunk_fwd<KTA>, trunk_fwd_waves(KTA)>(TrunkLds<KTA>::fwd_floats, a->num_points, st, *a);
    });
}

extern "C" int emd_mlp_trunk_backward(const EmdMlpTrunk* a, const EmdMlpTrunkGrads* g, void* hip_stream) {
    int rc = check_trunk_backward(a, g, "mlp_trunk_backward");
    if (rc || a->num_points == 0) return rc;
    return trunk_backward_dispatch<Kernels>(a, g, (hipStream_t)hip_stream);
}
