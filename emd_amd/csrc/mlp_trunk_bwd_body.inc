// mlp_trunk_bwd_body.inc -- the BODY of the trunk backward (k_mlp_trunk_bwd[_det]): expects `a` (EmdMlpTrunk), `g` (EmdMlpTrunkGrads), KTA, MULTI and a flush policy `fl`;
// tensor ids of the flush: 0 the xa block of d_w, 1 its xb block, 2 d_b.
// Included textually inside the __global__ function of each unit (mlp.hip: FlushAtomic, mlp_det.hip: FlushSlab), not called: routed through a
// function, the default kernels came out with another register allocation (profiles/mlp_det_isa.txt pins them instruction for instruction).
    typedef TrunkLds<KTA> L;
    extern __shared__ float lds[];
    if (KTA) stage_split(lds + L::wat, KTA, 4, a.w, a.ld_w, a.col_a, 64, a.ka, true);
    stage_matrix_t(lds + L::wbt, WS, 64, 32, a.kb > 0 ? a.w : nullptr, a.ld_w, a.col_b, 64, a.kb);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
    float* T = lds + L::scratch + wave * 32 * TS;
    const size_t N = (size_t)a.num_points, tiles = (N + 31) / 32;
    f32x16 dWa[2][KTA ? KTA : 1], dWb[2];
    float db[2] = {0.f, 0.f};
#pragma unroll
    for (int to = 0; to < 2; to++) {
        dWb[to] = zero16();
#pragma unroll
        for (int t = 0; t < (KTA ? KTA : 1); t++) dWa[to][t] = zero16();
    }
    const size_t tile0 = (size_t)blockIdx.x * MLP_WAVES + wave, tstep = (size_t)gridDim.x * MLP_WAVES;
    auto rowc = [&](size_t row_) -> size_t { return row_ < N ? row_ : 0; };
    f32x16 ngh[2] = {load_tile_raw(g.g_h[0], 64, rowc(tile0 * 32 + r), 0, hh), load_tile_raw(g.g_h[0], 64, rowc(tile0 * 32 + r), 32, hh)};
    for (size_t tile = tile0; tile < tiles; tile += tstep) {
        const size_t row = tile * 32 + r;
        const bool ok = row < N;
        // dL/dh: the sum of the branches' contributions
        f32x16 gh[2] = {mask_tile(ngh[0], ok, 0, hh, 64), mask_tile(ngh[1], ok, 32, hh, 64)};
        f32x16 xa[KTA ? KTA : 1];
        float xb[4];
        if (KTA) {
#pragma unroll
            for (int t = 0; t < KTA; t++) xa[t] = load_tile_raw(a.xa, a.ka, rowc(row), 32 * t, hh, a.ka);
        }
        if (a.kb > 0) {                                  // (kernel-uniform, the same loads every iteration)
#pragma unroll
            for (int j = 0; j < 4; j++) xb[j] = a.xb[rowc(row) * (size_t)a.kb + (4 * hh + j < a.kb ? 4 * hh + j : 0)];
        }
        {
            const size_t nrow = rowc((tile + tstep) * 32 + r);
            ngh[0] = load_tile_raw(g.g_h[0], 64, nrow, 0, hh); ngh[1] = load_tile_raw(g.g_h[0], 64, nrow, 32, hh);
        }
        if constexpr (MULTI) {
            for (int k = 1; k < g.num_gh; k++) {
                const f32x16 p0 = load_tile(g.g_h[k], 64, row, ok, 0, hh), p1 = load_tile(g.g_h[k], 64, row, ok, 32, hh);
#pragma unroll
                for (int v = 0; v < 16; v++) { gh[0][v] += p0[v]; gh[1][v] += p1[v]; }
            }
        }
        const f32x16 gf[2] = {transpose_tile(gh[0], T, r, hh), transpose_tile(gh[1], T, r, hh)};
        db[0] += frag_sum(gf[0]); db[1] += frag_sum(gf[1]);
        if constexpr (KTA > 0) {
            if (g.d_xa) {
                f32x16 gx[KTA];
#pragma unroll
                for (int t = 0; t < KTA; t++) gx[t] = zero16();
                layer_fwd_s<2, KTA>(gx, gh, reinterpret_cast<const uint4*>(lds + L::wat), KTA, 4, 0, lane);
#pragma unroll
                for (int t = 0; t < KTA; t++) store_tile(g.d_xa, a.ka, row, ok, 32 * t, hh, gx[t], a.ka);
            }
            const Split gs[2] = {split_tile(gf[0]), split_tile(gf[1])};
#pragma unroll
            for (int t = 0; t < KTA; t++) {
                const Split as = split_tile(transpose_tile(xa[t], T, r, hh));
                dWa[0][t] = outer_acc_s(dWa[0][t], gs[0], as);
                dWa[1][t] = outer_acc_s(dWa[1][t], gs[1], as);
            }
        }
        if (a.kb > 0) {
            // xb as a tile: feature c = 8 (v / 4) + 4 hh + v % 4 < kb <= 8 lives in registers 0..3 (columns >= kb were read from column 0: zeroed here)
            f32x16 xt = zero16();
#pragma unroll
            for (int j = 0; j < 4; j++) xt[j] = xb[j] * ((4 * hh + j < a.kb) ? 1.f : 0.f);
            const f32x16 af = transpose_tile(xt, T, r, hh);
            dWb[0] = outer_acc(dWb[0], gf[0], af);
            dWb[1] = outer_acc(dWb[1], gf[1], af);
            if (g.d_xb) {
                // d xb[c] = sum_k Wb[k][c] gh[k]: one tile whose features c >= kb are zero (the rows of Wb^T beyond kb are zero)
                f32x16 gx1[1] = {zero16()};
                layer_fwd<2, 1>(gx1, gh, lds + L::wbt, WS, 0, r, hh);
                const f32x16 gx = gx1[0];
                if (ok) {
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int c = 4 * hh + j;
                        if (c < a.kb) g.d_xb[row * (size_t)a.kb + c] = gx[j];
                    }
                }
            }
        }
    }
    float* red = lds + L::scratch;
#pragma unroll
    for (int to = 0; to < 2; to++) {
        if (KTA) {
#pragma unroll
            for (int t = 0; t < KTA; t++) {
                const f32x16 sa = wg_sum16(dWa[to][t], red, wave, lane);
                if (wave == 0) fl.dw(0, g.d_w ? g.d_w + a.col_a : nullptr, a.ld_w, 32 * to, 32 * t, 64, a.ka, sa, r, hh);
            }
        }
        if (a.kb > 0) {
            const f32x16 sb = wg_sum16(dWb[to], red, wave, lane);
            if (wave == 0) fl.dw(1, g.d_w ? g.d_w + a.col_b : nullptr, a.ld_w, 32 * to, 0, 64, a.kb, sb, r, hh);
        }
        const float bs = wg_sum1(db[to], red, wave, lane);
        if (wave == 0) fl.db(2, g.d_b, 32 * to, 64, bs, r);
    }
