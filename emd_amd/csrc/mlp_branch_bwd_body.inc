// mlp_branch_bwd_body.inc -- the BODY of the head backward (k_mlp_branch_bwd[_det]): expects `a` (EmdMlpBranch), `g` (EmdMlpBranchGrads), DEPTH, NTO, L1, RC, GO, CHAIN and a flush policy `fl`;
// tensor ids of the flush: 0 / 1 d_w_hidden[0] / d_b_hidden[0], 2 / 3 the second hidden layer's, 4 / 5 d_w_out / d_b_out.
// Included textually inside the __global__ function of each unit (mlp.hip: FlushAtomic, mlp_det.hip: FlushSlab), not called: routed through a
// function, the default kernels came out with another register allocation (profiles/mlp_det_isa.txt pins them instruction for instruction).
    typedef BranchLds<DEPTH, NTO, branch_mode(DEPTH, NTO, true)> L;
    extern __shared__ float lds[];
    branch_stage<DEPTH, NTO, true, RC>(lds, a);
    const float* rc = lds + L::bwd_floats;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
    float* T = lds + L::scratch + wave * 32 * TS;
    const size_t N = (size_t)a.num_points, tiles = (N + 31) / 32;
    const bool wide_out = (a.out_dim & 3) == 0;
    f32x16 dW1[2][2], dW2[2][2], dWo[NTO][2];
    float db1[2] = {0.f, 0.f}, db2[2] = {0.f, 0.f}, dbo[NTO];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) { dW1[i][j] = zero16(); dW2[i][j] = zero16(); }
#pragma unroll
    for (int t = 0; t < NTO; t++) { dWo[t][0] = zero16(); dWo[t][1] = zero16(); dbo[t] = 0.f; }

    const size_t tile0 = (size_t)blockIdx.x * MLP_WAVES + wave, tstep = (size_t)gridDim.x * MLP_WAVES;
    // g.l1_grad: the gradient of the head's L1 regulariser (mean |out|, EmdMlpBranch.l1_sum) joins dL/dout while it is loaded:
    // + sign(out) l1_grad / (N out_dim); g_out itself may then be absent
    const float l1_s = (L1 && g.l1_grad) ? g.l1_grad[0] / ((float)a.num_points * (float)a.out_dim) : 0.f;
    auto load_go = [&](size_t row_, bool ok_, int t) -> f32x16 {
        const bool wide = wide_out && 32 * t + 32 <= a.out_dim;
        f32x16 v = (L1 && !g.g_out) ? zero16() : (wide ? load_tile(g.g_out, a.out_dim, row_, ok_, 32 * t, hh) : load_tile_narrow(g.g_out, a.out_dim, row_, ok_, 32 * t, hh));
        if (L1 && g.l1_grad) {
            const f32x16 o = wide ? load_tile(g.out, a.out_dim, row_, ok_, 32 * t, hh) : load_tile_narrow(g.out, a.out_dim, row_, ok_, 32 * t, hh);
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] += o[k] > 0.f ? l1_s : (o[k] < 0.f ? -l1_s : 0.f);      // (rows / features past the end read 0: no term)
        }
        return v;
    };
    // the next tile's h and g_out are loaded while this tile computes (one wave per SIMD: nothing else hides the HBM latency).  Every load of the
    // loop is unconditional and raw (see load_tile_raw); rows past the end read row 0 and their dL/dout is masked to zero where it is used, which
    // zeroes everything they could contribute (their h needs no mask: a finite activation times a zero gradient).
    auto rowc = [&](size_t row_) -> size_t { return row_ < N ? row_ : 0; };
    f32x16 nh[2];
    float nxb[4];
    f32x16 ngo[NTO];
    float ngn[4] = {0.f, 0.f, 0.f, 0.f};
    auto fetch = [&](size_t row_) {                      // h (or the embedding) and dL/dout of one tile
        const size_t rcl = rowc(row_);
        if constexpr (RC) load_xb_raw(a.xb, a.kb_in, row_, row_ < N, hh, nxb);
        else { nh[0] = load_tile_raw(a.h, 64, rcl, 0, hh); nh[1] = load_tile_raw(a.h, 64, rcl, 32, hh); }
        if constexpr (GO == 0) {
#pragma unroll
            for (int j = 0; j < 4; j++) ngn[j] = g.g_out[rcl * (size_t)a.out_dim + (j < a.out_dim ? j : 0)];
        } else if constexpr (GO == 1) {
#pragma unroll
            for (int t = 0; t < NTO; t++) ngo[t] = load_tile_raw(g.g_out, a.out_dim, rcl, 32 * t, hh, a.out_dim);
        } else {
#pragma unroll
            for (int t = 0; t < NTO; t++) ngo[t] = load_go(row_, row_ < N, t);
        }
    };
    fetch(tile0 * 32 + r);
    for (size_t tile = tile0; tile < tiles; tile += tstep) {
        const size_t row = tile * 32 + r;
        const bool ok = row < N;
        // ---- recompute the forward
        f32x16 hin[2];
        f32x16 go[NTO];
        float gn[4];
        if constexpr (GO == 0) {
#pragma unroll
            for (int j = 0; j < 4; j++) gn[j] = ngn[j];
        } else {
#pragma unroll
            for (int t = 0; t < NTO; t++) go[t] = ngo[t];
        }
        float xbm[4];
        if constexpr (RC) mask_xb(nxb, a.kb_in, ok, hh, xbm);
        else { hin[0] = nh[0]; hin[1] = nh[1]; }
        // this tile's forward outputs (the L1 term's sign) and the earlier heads' dL/dh (EmdMlpBranchGrads.g_h_in, added before the store) are
        // requested first -- older than the prefetches behind them, so waiting for them later does not wait for those
        f32x16 oraw[NTO];
        float on[4];
        if constexpr (L1 && GO == 0) {                    // (an L1 kernel is launched with l1_grad and the forward's outputs present)
#pragma unroll
            for (int j = 0; j < 4; j++) on[j] = g.out[rowc(row) * (size_t)a.out_dim + (j < a.out_dim ? j : 0)];
        } else if constexpr (L1 && GO == 1) {
#pragma unroll
            for (int t = 0; t < NTO; t++) oraw[t] = load_tile_raw(g.out, a.out_dim, rowc(row), 32 * t, hh, a.out_dim);
        }
        f32x16 gin[2] = {zero16(), zero16()};
        if constexpr (GO == 2) {
            if (DEPTH == 1 && g.g_h_in) { gin[0] = load_tile(g.g_h_in, 64, row, ok, 0, hh); gin[1] = load_tile(g.g_h_in, 64, row, ok, 32, hh); }
        } else if constexpr (CHAIN) { gin[0] = load_tile_raw(g.g_h_in, 64, rowc(row), 0, hh); gin[1] = load_tile_raw(g.g_h_in, 64, rowc(row), 32, hh); }
        fetch((tile + tstep) * 32 + r);
        if constexpr (RC) embed_h(rc, rc + 64 * 12, r, hh, xbm, hin);
        f32x16 x[2] = {hin[0], hin[1]};
        if (a.relu_input) { x[0] = relu16(x[0]); x[1] = relu16(x[1]); }
        f32x16 m1[2] = {bias_tile(lds + L::b1, 0, hh), bias_tile(lds + L::b1, 32, hh)};
        mm<L::SP, 2, 2>(m1, x, lds + L::w1, WS, 0, 2, 4, r, hh, lane);
        m1[0] = relu16(m1[0]); m1[1] = relu16(m1[1]);
        f32x16 m2[2];
        if (DEPTH == 2) {
            m2[0] = bias_tile(lds + L::b2, 0, hh); m2[1] = bias_tile(lds + L::b2, 32, hh);
            layer_fwd<2, 2>(m2, m1, lds + L::w2, WS, 0, r, hh);
            m2[0] = relu16(m2[0]); m2[1] = relu16(m2[1]);
        }
        f32x16 (&last)[2] = DEPTH == 2 ? m2 : m1;          // the activation that feeds the output layer
        // ---- dL/dout of this tile from its raw pieces: masked here, after the forward's MFMAs, where it is first needed
        if constexpr (GO == 0) {
            go[0] = zero16();
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float v = gn[j];
                if constexpr (L1) v += on[j] > 0.f ? l1_s : (on[j] < 0.f ? -l1_s : 0.f);
                go[0][j] = v * ((ok && hh == 0 && j < a.out_dim) ? 1.f : 0.f);
            }
        } else if constexpr (GO == 1) {
#pragma unroll
            for (int t = 0; t < NTO; t++) {
                if constexpr (L1) {
#pragma unroll
                    for (int k = 0; k < 16; k++) go[t][k] += oraw[t][k] > 0.f ? l1_s : (oraw[t][k] < 0.f ? -l1_s : 0.f);
                }
                go[t] = mask_tile(go[t], ok, 32 * t, hh, a.out_dim);
            }
        }
        // ---- output layer
        f32x16 gl[2] = {zero16(), zero16()};
        if (NTO == 1 && a.out_dim <= 8) mm<L::SP, NTO, 2, 1>(gl, go, lds + L::wot, L::WOT, 0, 2, 2 * NTO, r, hh, lane);  // dx / do / feat: one 8-feature chunk carries everything
        else if (NTO == 2 && a.out_dim <= 48) {       // dshs (48 outputs): the second tile's upper two 8-feature chunks are padding
            const f32x16 g0[1] = {go[0]}, g1[1] = {go[NTO - 1]};
            mm<L::SP, 1, 2>(gl, g0, lds + L::wot, L::WOT, 0, 2, 2 * NTO, r, hh, lane);
            mm<L::SP, 1, 2, 2>(gl, g1, lds + L::wot, L::WOT, 32, 2, 2 * NTO, r, hh, lane);
        } else mm<L::SP, NTO, 2>(gl, go, lds + L::wot, L::WOT, 0, 2, 2 * NTO, r, hh, lane);
        gl[0] = mask16(gl[0], last[0]); gl[1] = mask16(gl[1], last[1]);
        {   // dWo += go (x) last, dbo += rowsum(go)
            const f32x16 af[2] = {transpose_tile(last[0], T, r, hh), transpose_tile(last[1], T, r, hh)};
            Split afs[2];
            split_all<L::SPO, 2>(afs, af);
#pragma unroll
            for (int t = 0; t < NTO; t++) {
                const f32x16 gf = transpose_tile(go[t], T, r, hh);
                dbo[t] += frag_sum(gf);
                outer_all<L::SPO, 2>(dWo[t], gf, af, afs);
            }
        }
        // ---- second hidden layer (feature head)
        f32x16 g1[2];
        if (DEPTH == 2) {
            g1[0] = zero16(); g1[1] = zero16();
            layer_fwd<2, 2>(g1, gl, lds + L::w2t, WS, 0, r, hh);
            g1[0] = mask16(g1[0], m1[0]); g1[1] = mask16(g1[1], m1[1]);
            f32x16 af[2] = {transpose_tile(m1[0], T, r, hh), transpose_tile(m1[1], T, r, hh)};
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const f32x16 gf = transpose_tile(gl[t], T, r, hh);
                db2[t] += frag_sum(gf);
                dW2[t][0] = outer_acc(dW2[t][0], gf, af[0]);
                dW2[t][1] = outer_acc(dW2[t][1], gf, af[1]);
            }
        } else {
            g1[0] = gl[0]; g1[1] = gl[1];
        }
        // ---- first hidden layer
        f32x16 gx[2] = {zero16(), zero16()};
        mm<L::SP, 2, 2>(gx, g1, lds + L::w1t, WS, 0, 2, 4, r, hh, lane);
        if (a.relu_input) { gx[0] = mask16(gx[0], hin[0]); gx[1] = mask16(gx[1], hin[1]); }
        if ((GO == 2 && DEPTH == 1 && g.g_h_in) || (GO != 2 && CHAIN)) { gx[0] += gin[0]; gx[1] += gin[1]; }     // (one-hidden-layer heads only: the other kernel has no registers left)
        store_tile(g.g_h, 64, row, ok, 0, hh, gx[0]);
        store_tile(g.g_h, 64, row, ok, 32, hh, gx[1]);
        {
            const f32x16 af[2] = {transpose_tile(x[0], T, r, hh), transpose_tile(x[1], T, r, hh)};
            Split afs[2];
            split_all<L::SPO, 2>(afs, af);
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const f32x16 gf = transpose_tile(g1[t], T, r, hh);
                db1[t] += frag_sum(gf);
                outer_all<L::SPO, 2>(dW1[t], gf, af, afs);
            }
        }
    }
    // ---- workgroup sums, then one atomic add per accumulator element and workgroup
    float* red = lds + L::scratch;
#pragma unroll
    for (int to = 0; to < 2; to++) {
#pragma unroll
        for (int ti = 0; ti < 2; ti++) {
            const f32x16 t1 = wg_sum16(dW1[to][ti], red, wave, lane);
            if (wave == 0) fl.dw(0, g.d_w_hidden[0], 64, 32 * to, 32 * ti, 64, 64, t1, r, hh);
            if (DEPTH == 2) {
                const f32x16 t2 = wg_sum16(dW2[to][ti], red, wave, lane);
                if (wave == 0) fl.dw(2, g.d_w_hidden[1], 64, 32 * to, 32 * ti, 64, 64, t2, r, hh);
            }
        }
        const float b1s = wg_sum1(db1[to], red, wave, lane);
        if (wave == 0) fl.db(1, g.d_b_hidden[0], 32 * to, 64, b1s, r);
        if (DEPTH == 2) {
            const float b2s = wg_sum1(db2[to], red, wave, lane);
            if (wave == 0) fl.db(3, g.d_b_hidden[1], 32 * to, 64, b2s, r);
        }
    }
#pragma unroll
    for (int t = 0; t < NTO; t++) {
        const f32x16 o0 = wg_sum16(dWo[t][0], red, wave, lane), o1 = wg_sum16(dWo[t][1], red, wave, lane);
        const float bos = wg_sum1(dbo[t], red, wave, lane);
        if (wave == 0) {
            fl.dw(4, g.d_w_out, 64, 32 * t, 0, a.out_dim, 64, o0, r, hh);
            fl.dw(4, g.d_w_out, 64, 32 * t, 32, a.out_dim, 64, o1, r, hh);
            fl.db(5, g.d_b_out, 32 * t, a.out_dim, bos, r);
        }
    }
