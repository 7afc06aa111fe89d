// mlp_embed_bwd_body.inc -- the BODY of the embedding-only trunk backward (k_mlp_embed_bwd[_det]): expects `a` (EmdMlpTrunk), `g` (EmdMlpTrunkGrads), KB, MULTI and a flush policy `fl`;
// tensor ids of the flush as the trunk's: 1 the xb block of d_w, 2 d_b.
// Included textually inside the __global__ function of each unit (mlp.hip: FlushAtomic, mlp_det.hip: FlushSlab), not called: routed through a
// function, the default kernels came out with another register allocation (profiles/mlp_det_isa.txt pins them instruction for instruction).
    __shared__ float wt[KB][64];                                  // Wb^T: wt[c][feature]
    __shared__ float red[MLP_WAVES][2][32][KB + 1];
    for (int idx = threadIdx.x; idx < KB * 64; idx += MLP_THREADS) {
        const int c = idx >> 6, k = idx & 63;
        wt[c][k] = a.w[(size_t)k * a.ld_w + a.col_b + c];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
    const size_t N = (size_t)a.num_points, tiles = (N + 31) / 32;
    float4 wreg[KB][2][4];
#pragma unroll
    for (int c = 0; c < KB; c++)
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int q = 0; q < 4; q++) wreg[c][t][q] = *(const float4*)&wt[c][32 * t + 8 * q + 4 * hh];
    float accw[2][16][KB], accb[2][16];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int v = 0; v < 16; v++) {
            accb[t][v] = 0.f;
#pragma unroll
            for (int c = 0; c < KB; c++) accw[t][v][c] = 0.f;
        }
    const size_t tile0 = (size_t)blockIdx.x * MLP_WAVES + wave, tstep = (size_t)gridDim.x * MLP_WAVES;
    auto load_x = [&](size_t row_) -> float4 { return *(const float4*)(a.xb + (row_ < N ? row_ : 0) * 4); };
    // (measured: three buffers in rotation with the loop unrolled by three -- no register copy of a travelling tile -- spill at 512 registers: 143 -> 358 us)
    f32x16 n1[2], n2[2];
    float4 x1, x2;
    {
        const size_t r1 = tile0 * 32 + r, r2 = (tile0 + tstep) * 32 + r;
        n1[0] = load_tile<true>(g.g_h[0], 64, r1, r1 < N, 0, hh); n1[1] = load_tile<true>(g.g_h[0], 64, r1, r1 < N, 32, hh); x1 = load_x(r1);
        n2[0] = load_tile<true>(g.g_h[0], 64, r2, r2 < N, 0, hh); n2[1] = load_tile<true>(g.g_h[0], 64, r2, r2 < N, 32, hh); x2 = load_x(r2);
    }
    for (size_t tile = tile0; tile < tiles; tile += tstep) {
        const size_t row = tile * 32 + r;
        const bool ok = row < N;
        f32x16 gh[2] = {n1[0], n1[1]};                            // dL/dh (rows past the end: zero)
        const float xb[KB] = {x1.x, x1.y, x1.z, x1.w};
        n1[0] = n2[0]; n1[1] = n2[1]; x1 = x2;
        {
            const size_t nrow = (tile + 2 * tstep) * 32 + r;
            n2[0] = load_tile<true>(g.g_h[0], 64, nrow, nrow < N, 0, hh); n2[1] = load_tile<true>(g.g_h[0], 64, nrow, nrow < N, 32, hh); x2 = load_x(nrow);
        }
        if constexpr (MULTI) {
            for (int k = 1; k < g.num_gh; k++) {
                const f32x16 p0 = load_tile<true>(g.g_h[k], 64, row, ok, 0, hh), p1 = load_tile<true>(g.g_h[k], 64, row, ok, 32, hh);
#pragma unroll
                for (int v = 0; v < 16; v++) { gh[0][v] += p0[v]; gh[1][v] += p1[v]; }
            }
        }
        if (g.d_xb) {
            float d[KB];
#pragma unroll
            for (int c = 0; c < KB; c++) {
                float acc = 0.f;
#pragma unroll
                for (int t = 0; t < 2; t++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const float4 w = wreg[c][t][q];
                        acc = fmaf(w.x, gh[t][4 * q], acc); acc = fmaf(w.y, gh[t][4 * q + 1], acc);
                        acc = fmaf(w.z, gh[t][4 * q + 2], acc); acc = fmaf(w.w, gh[t][4 * q + 3], acc);
                    }
                d[c] = acc + __shfl_xor(acc, 32);
            }
            if (hh == 0 && ok) *(float4*)(g.d_xb + row * 4) = make_float4(d[0], d[1], d[2], d[3]);       // whole 16-byte rows: 512 contiguous bytes per instruction
        }
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int v = 0; v < 16; v++) {
                accb[t][v] += gh[t][v];
#pragma unroll
                for (int c = 0; c < KB; c++) accw[t][v][c] = fmaf(gh[t][v], xb[c], accw[t][v][c]);
            }
    }
    // ---- sums over the 32 rows of a lane half (xor shuffles stay inside the half), the waves, then one atomic per element and workgroup
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int v = 0; v < 16; v++) {
            float s[KB + 1];
#pragma unroll
            for (int c = 0; c < KB; c++) s[c] = accw[t][v][c];
            s[KB] = accb[t][v];
#pragma unroll
            for (int c = 0; c <= KB; c++) {
#pragma unroll
                for (int m = 1; m < 32; m <<= 1) s[c] += __shfl_xor(s[c], m);
            }
            if (r == 0) {
#pragma unroll
                for (int c = 0; c <= KB; c++) red[wave][t][8 * (v >> 2) + 4 * hh + (v & 3)][c] = s[c];
            }
        }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 64 * (KB + 1); idx += MLP_THREADS) {
        const int k = idx / (KB + 1), c = idx - k * (KB + 1);
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < MLP_WAVES; w++) s += red[w][k >> 5][k & 31][c];
        if (c < KB) { if (g.d_w) fl.one(1, g.d_w + (size_t)k * a.ld_w + a.col_b + c, k * KB + c, 64 * KB, s); }
        else if (g.d_b) fl.one(2, g.d_b + k, k, 64, s);
    }
