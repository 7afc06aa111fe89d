// embed_det.hip -- emd_temporal_embed_backward_det: the backward of the temporal embedding row (embed.hip, k_temporal_embed<true>) without atomics
// (DESIGN.md section 8.14).  A unit of its own: embed.hip's kernels are pinned instruction for instruction (profiles/mlp_det_isa.txt), and a further
// kernel inside that unit changed the code of its neighbours.  What the units share is shared as text: the sampling set-up is temporal_sample.h, the
// gather-form accumulation te_gather_body.inc (also track_det.hip's).  One pair stays written twice, the dL/dt column walk below and in
// k_temporal_embed<true>: that kernel's set-up is written out in place because it came out with other registers when taken from the helpers, so
// a text both could include would change its instructions (profiles/shared_source_isa.txt).
#include "common.h"
#include "temporal_sample.h"

namespace {

// The backward of k_temporal_embed without atomics, in gather form.  k_temporal_embed<true> adds onto addresses that collide
// between lanes (lane j's x1 is lane j + 1's x0; ha and hb of the two resized rows can coincide), and every table adds onto one g_t.  Here the at most
// four touched table rows are slots q = 2 r + (0: ha, 1: hb); the lane of (q, column c) owns element (row[q], c) when no earlier slot names the same
// row, and adds ITS contributions in the default kernel's issue order -- j ascending, then te_gather_body.inc's --, in double precision
// from 0.0, rounded once and WRITTEN (rows no sample touches keep the caller's zeros).
// dL/dt: wave 0 walks the columns as the default kernel does, the fixed xor tree follows; one table adds onto g_t itself, several leave one partial
// each in `dt_part` for k_temporal_dt_sum.
#define TE_DET_THREADS 256
__global__ void __launch_bounds__(TE_DET_THREADS) k_temporal_embed_bwd_det(const float* __restrict__ weight, int rows, int dim, int k,
                                                                            const float* __restrict__ t_ptr, const float* __restrict__ g_out,
                                                                            float* __restrict__ g_weight, float* __restrict__ g_t,
                                                                            float* __restrict__ dt_part) {
#pragma clang fp contract(off)
    weight += (size_t)blockIdx.x * rows * dim;
    g_out += (size_t)blockIdx.x * dim;
    const TeSample s = te_rows(t_ptr[0], k, rows);
    if (g_weight) {
        float* __restrict__ G = g_weight + (size_t)blockIdx.x * rows * dim;
        const int row_of[4] = {s.ha[0], s.hb[0], s.ha[1], s.hb[1]};
        for (int idx = threadIdx.x; idx < 4 * dim; idx += TE_DET_THREADS) {
            const int q = idx / dim, c = idx - q * dim;
            if (q >= 2 && !s.in1) continue;                      // the row past the end contributes nothing: its slots name no row
            const int R = row_of[q];
            bool owner = true;
            for (int p = 0; p < q; p++) owner = owner && row_of[p] != R;
            if (!owner) continue;
            double acc = 0.0;
            for (int j = 0; j < dim; j++) {
                const TeCol col = te_col(j, dim);
                const bool m0 = col.x0 == c, m1 = col.inx1 && col.x1 == c;
                if (!m0 && !m1) continue;
                const float g = g_out[j], wx0 = col.wx0, wx1 = col.wx1;
#include "te_gather_body.inc"
            }
            G[(size_t)R * dim + c] = (float)acc;
        }
    }
    if (g_t && threadIdx.x < EMD_WAVE) {
        float my;
        reflect_coord((t_ptr[0] - 0.5f) * 2.f, k, &my);
        float dt_acc = 0.f;
        for (int j = threadIdx.x; j < dim; j += EMD_WAVE) {
            const TeCol col = te_col(j, dim);
            float wv[2][4], v[2][2];
            te_taps(weight, dim, s, col, wv);
#pragma unroll
            for (int r = 0; r < 2; r++) {
                v[r][0] = s.la[r] * wv[r][0] + s.lb[r] * wv[r][1];
                v[r][1] = col.inx1 ? s.la[r] * wv[r][2] + s.lb[r] * wv[r][3] : 0.f;
            }
            if (!s.in1) v[1][0] = v[1][1] = 0.f;
            dt_acc += g_out[j] * ((v[1][0] - v[0][0]) * col.wx0 + (v[1][1] - v[0][1]) * col.wx1);
        }
        for (int off = 32; off; off >>= 1) dt_acc += __shfl_xor(dt_acc, off);
        if (threadIdx.x == 0) {
            const float d = dt_acc * my * 2.f;                   // y = (t - 0.5) * 2
            if (dt_part) dt_part[blockIdx.x] = d;
            else g_t[0] += d;
        }
    }
}

// the tables' dL/dt partials, added in ascending order onto g_t by one thread
__global__ void k_temporal_dt_sum(const float* __restrict__ dt_part, int tables, float* __restrict__ g_t) {
    if (blockIdx.x || threadIdx.x) return;
    float s = g_t[0];
    for (int b = 0; b < tables; b++) s += dt_part[b];
    g_t[0] = s;
}

}  // namespace

extern "C" int emd_temporal_embed_backward_det(const float* weight, int tables, int rows, int dim, int k, const float* t, const float* dL_dout,
                                               float* dL_dweight, float* dL_dt, float* dt_partials, void* hip_stream) {
    int rc = check_te(weight, tables, rows, dim, k, t, "temporal_embed_backward_det");
    if (rc) return rc;
    if (!dL_dout) { emd_set_error("temporal_embed_backward_det: null gradient"); return EMD_ERR_INVALID; }
    const bool parts = dL_dt && tables > 1;
    if (parts && !dt_partials) { emd_set_error("temporal_embed_backward_det: dL_dt of %d tables needs dt_partials", tables); return EMD_ERR_WORKSPACE; }
    hipLaunchKernelGGL(k_temporal_embed_bwd_det, dim3(tables), dim3(TE_DET_THREADS), 0, (hipStream_t)hip_stream, weight, rows, dim, k, t, dL_dout,
                       dL_dweight, dL_dt, parts ? dt_partials : (float*)nullptr);
    EMD_LAUNCH_CHECK();
    if (parts) {
        hipLaunchKernelGGL(k_temporal_dt_sum, dim3(1), dim3(1), 0, (hipStream_t)hip_stream, (const float*)dt_partials, tables, dL_dt);
        EMD_LAUNCH_CHECK();
    }
    return EMD_OK;
}
