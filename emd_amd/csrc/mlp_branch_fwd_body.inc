// mlp_branch_fwd_body.inc -- the BODY of the head forward (k_mlp_branch_fwd[_det]): expects the kernel's `a` (EmdMlpBranch), DEPTH, NTO, L1, RC and a flush policy `fl`.
// Included textually inside the __global__ function of each unit (mlp.hip: FlushAtomic, mlp_det.hip: FlushSlab), not called: routed through a
// function, the default kernels came out with another register allocation (profiles/mlp_det_isa.txt pins them instruction for instruction).
    typedef BranchLds<DEPTH, NTO, branch_mode(DEPTH, NTO, false)> L;
    extern __shared__ float lds[];
    branch_stage<DEPTH, NTO, false, RC>(lds, a);
    const float* rc = lds + L::fwd_floats;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
    const size_t N = (size_t)a.num_points, tiles = (N + 31) / 32;
    const bool wide_out = (a.out_dim & 3) == 0;
    const bool narrow_out = a.out_dim <= 4;
    float l1_acc = 0.f;
    const size_t tile0 = (size_t)blockIdx.x * MLP_WAVES + wave, tstep = (size_t)gridDim.x * MLP_WAVES;
    // the next tile's rows are loaded while this tile computes: one wave per SIMD has nothing else to hide the HBM latency behind
    f32x16 nx[2];
    float nxb[4];
    // (h travels raw: a row past the end reads row 0 and its outputs are neither stored nor counted -- a product or select behind the load puts the
    //  wait for the prefetch AT the load)
    auto hrow = [&](size_t row_) -> size_t { return row_ < N ? row_ : 0; };
    if constexpr (RC) load_xb_raw(a.xb, a.kb_in, tile0 * 32 + r, tile0 * 32 + r < N, hh, nxb);
    else { nx[0] = load_tile_raw(a.h, 64, hrow(tile0 * 32 + r), 0, hh); nx[1] = load_tile_raw(a.h, 64, hrow(tile0 * 32 + r), 32, hh); }
    for (size_t tile = tile0; tile < tiles; tile += tstep) {
        const size_t row = tile * 32 + r;
        const bool ok = row < N;
        f32x16 x[2];
        const size_t nrow = (tile + tstep) * 32 + r;
        if constexpr (RC) {
            float xb[4];
            mask_xb(nxb, a.kb_in, ok, hh, xb);
            load_xb_raw(a.xb, a.kb_in, nrow, nrow < N, hh, nxb);
            embed_h(rc, rc + 64 * 12, r, hh, xb, x);
        } else {
            x[0] = nx[0]; x[1] = nx[1];
            nx[0] = load_tile_raw(a.h, 64, hrow(nrow), 0, hh); nx[1] = load_tile_raw(a.h, 64, hrow(nrow), 32, hh);
        }
        if (a.relu_input) { x[0] = relu16(x[0]); x[1] = relu16(x[1]); }
        f32x16 m[2] = {bias_tile(lds + L::b1, 0, hh), bias_tile(lds + L::b1, 32, hh)};
        mm<L::SP, 2, 2>(m, x, lds + L::w1, WS, 0, 2, 4, r, hh, lane);
        m[0] = relu16(m[0]); m[1] = relu16(m[1]);
        if (DEPTH == 2) {
            f32x16 m2[2] = {bias_tile(lds + L::b2, 0, hh), bias_tile(lds + L::b2, 32, hh)};
            mm<L::SP, 2, 2>(m2, m, lds + L::w2, WS, 0, 2, 4, r, hh, lane);
            m[0] = relu16(m2[0]); m[1] = relu16(m2[1]);
        }
        if constexpr (NTO == 1) {
            // Round 5: an output layer of at most four features (dx: 3, do: 1) on the VECTOR pipe.  As an MFMA tile it is padded to 32 output rows --
            // 32 of the kernel's 96 MFMAs per 32-row tile for 3 or 1 useful rows -- while the contraction itself is 64 multiply-adds per output and
            // row: a lane holds 32 of its row's 64 activations (the two lane halves hold the two feature halves), so it forms 4 x 32 products
            // against weight rows read as broadcast ds_read_b128 and the halves meet in one cross-lane add.  (Summation order differs from the MFMA's
            // k-ordered chain: fp32 rounding only.)
            if (narrow_out) {
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < 2; t++)
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const int f0 = 32 * t + 8 * c + 4 * hh;
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const float4 w = *(const float4*)(lds + L::wo + q * WS + f0);           // (rows >= out_dim of the staged matrix are zero)
                            acc[q] = fmaf(w.x, m[t][4 * c], acc[q]); acc[q] = fmaf(w.y, m[t][4 * c + 1], acc[q]);
                            acc[q] = fmaf(w.z, m[t][4 * c + 2], acc[q]); acc[q] = fmaf(w.w, m[t][4 * c + 3], acc[q]);
                        }
                    }
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = acc[q] + __shfl_xor(acc[q], 32) + lds[L::bo + q];
                if (hh == 0 && ok) {
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (q < a.out_dim) {
                            a.out[row * (size_t)a.out_dim + q] = acc[q];
                            if (L1 && a.l1_sum) l1_acc += fabsf(acc[q]);
                        }
                }
                continue;
            }
        }
        f32x16 o[NTO];
#pragma unroll
        for (int t = 0; t < NTO; t++) o[t] = bias_tile(lds + L::bo, 32 * t, hh);
        mm<L::SP, 2, NTO>(o, m, lds + L::wo, WS, 0, NTO, 4, r, hh, lane);
        if (L1 && a.l1_sum && ok) {                   // the head's L1 regulariser, formed while the outputs are in registers
#pragma unroll
            for (int t = 0; t < NTO; t++)
#pragma unroll
                for (int v = 0; v < 16; v++)
                    if (32 * t + 8 * (v >> 2) + 4 * hh + (v & 3) < a.out_dim) l1_acc += fabsf(o[t][v]);
        }
#pragma unroll
        for (int t = 0; t < NTO; t++) {
            // (a wide tile may still hang over the row's end: out_dim = 48 -> the second tile holds features 32..47: whole 16-byte pieces, bounded by the width)
            if (wide_out) store_tile(a.out, a.out_dim, row, ok, 32 * t, hh, o[t], a.out_dim);
            else store_tile_narrow(a.out, a.out_dim, row, ok, 32 * t, hh, o[t]);
        }
    }
    if (L1 && a.l1_sum) {                             // mean |out| over the N x out_dim outputs: ONE atomic per workgroup (a float atomic per wave was
        __shared__ float s_l1[MLP_WAVES];             // 1 024 - 2 048 atomics on one address at the very end of the kernel, served one after the other: ~40 us)
        const float s = wave_reduce_to_lane63(l1_acc);
        if (lane == 63) s_l1[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < MLP_WAVES; w++) t += s_l1[w];
            fl.l1(a.l1_sum, t, a.num_points, a.out_dim);
        }
    }
