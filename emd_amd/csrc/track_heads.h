// track_heads.h -- the per-actor helpers of the actor chain that hold no atomic (temporal blend, wave sum, the eight head rows) and the argument checks
// of its entry points: shared by embed.hip and track_det.hip (the chain without atomics).  The text is embed.hip's own, moved
// here unchanged and in its order.  te_scatter and heads_backward call atomicAdd and stay in embed.hip: nothing that holds an atomic may enter a file
// a deterministic unit includes (tests/test_track_det_cpu.py reads this file for the word).
#pragma once
#include "common.h"
#include "temporal_sample.h"

namespace {

// the bilinear blend of a sample's eight taps.  ONE function without contraction for every caller: the one-launch actor chain (te_column2) and the
// three-launch path (te_column) must produce the same bits (tests/test_motion_sh_gpu.py), and with contraction left to the compiler the two
// inlined copies were fused differently.
__device__ __forceinline__ float te_eval(const TeSample& s, const float (&wv)[2][4], const TeCol& c) {
#pragma clang fp contract(off)
    float out = 0.f;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const float wy = r ? s.wy1 : s.wy0;
        const float v0 = s.la[r] * wv[r][0] + s.lb[r] * wv[r][1];
        const float v1 = c.inx1 ? s.la[r] * wv[r][2] + s.lb[r] * wv[r][3] : 0.f;
        const float term = v0 * (c.wx0 * wy) + v1 * (c.wx1 * wy);
        out = (r == 1 && !s.in1) ? out : out + term;
    }
    return out;
}

// column j of the sampled row
__device__ __forceinline__ float te_column(const float* __restrict__ weight, int dim, const TeSample& s, int j) {
    const TeCol c = te_col(j, dim);
    float wv[2][4];
    te_taps(weight, dim, s, c, wv);
    return te_eval(s, wv, c);
}

// two samples of the same table column (the coarse and the fine level of an actor's table): all sixteen taps are requested before either is evaluated
__device__ __forceinline__ void te_column2(const float* __restrict__ weight, int dim, const TeSample& sa, const TeSample& sb, int j, float* oa, float* ob) {
    const TeCol c = te_col(j, dim);
    float wa[2][4], wb[2][4];
    te_taps(weight, dim, sa, c, wa);
    te_taps(weight, dim, sb, c, wb);
    *oa = te_eval(sa, wa, c);
    *ob = te_eval(sb, wb, c);
}

__device__ __forceinline__ float wave_sum_all(float v) {
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the eight head rows: o = 0-2 trans_c, 3-5 trans_f, 6 rot_c, 7 rot_f -> head tensor, its row, and whether it reads h_c or h_f
__device__ __forceinline__ constexpr int head_of(int o) { return o < 3 ? 0 : o < 6 ? 1 : o - 4; }
__device__ __forceinline__ constexpr int head_row(int o) { return o < 3 ? o : o < 6 ? o - 3 : 0; }
__device__ __forceinline__ constexpr bool head_coarse(int o) { return o < 3 || o == 6; }

// The heads of one actor by one wave, for k_track_heads and k_tracked_pose alike (contraction is the unit's default in both).  Every lane holds its
// column of the eight head rows (wrow: zero past the width) and of h_c / h_f; out[] and the rotation (ow, 0, 0, oz) come out wave-uniform.
__device__ __forceinline__ void heads_eval(const float (&wrow)[8], const float (&hbias)[8], float hc, float hf, float (&out)[8], float* ow, float* oz) {
#pragma unroll
    for (int o = 0; o < 8; o++) out[o] = wave_sum_all(wrow[o] * (head_coarse(o) ? hc : hf)) + hbias[o];
    const float cc = cosf(out[6]), scn = sinf(out[6]), cf = cosf(out[7]), sfn = sinf(out[7]);
    // quaternion_raw_multiply of two rotations about z: ow = cc cf - scn sfn, oz = cc sfn + scn cf.  Which product of each pair is fused is written
    // out: left to the compiler, the copy inlined into k_tracked_pose was packed with the quaternion product behind it and fused the other product
    // of oz than k_track_heads' copy (one ulp in the pose table).  This is the form both kernels had before they shared this function.
    *ow = fmaf(cc, cf, -(scn * sfn)); *oz = fmaf(scn, cf, cc * sfn);
}

int check_track(const EmdTrackArgs* a, const char* who) {
    if (!a) { emd_set_error("%s: null args", who); return EMD_ERR_INVALID; }
    if (a->num_actors < 0 || a->rows < 1 || a->dim < 1 || a->embed_dim < 0 || a->dim + a->embed_dim > EMD_WAVE || a->k_coarse < 1 || a->k_fine < 1 ||
        a->num_points < 0) { emd_set_error("%s: bad sizes (dim + embed_dim <= 64)", who); return EMD_ERR_INVALID; }
    if (a->num_actors == 0) return EMD_OK;
    if (!a->weight || !a->count || !a->emb_sum || (a->embed_dim > 0 && a->num_points > 0 && (!a->embeddings || !a->point_ids))) {
        emd_set_error("%s: null pointer", who); return EMD_ERR_INVALID;
    }
    for (int h = 0; h < 4; h++) if (!a->head_w[h] || !a->head_b[h]) { emd_set_error("%s: null head parameter %d", who, h); return EMD_ERR_INVALID; }
    return EMD_OK;
}

int check_tracked(const EmdTrackedPoseArgs* p, const char* who) {
    if (!p) { emd_set_error("%s: null args", who); return EMD_ERR_INVALID; }
    int rc = check_track(&p->track, who);
    if (rc) return rc;
    const EmdTrackArgs& a = p->track;
    if (a.num_actors == 0) return EMD_OK;
    if (!a.segment_start || a.embed_dim > 8) { emd_set_error("%s: needs segment_start (points sorted by actor) and embed_dim <= 8", who); return EMD_ERR_INVALID; }
    if (!p->q_all || !p->t_all || p->num_frames < 1 || (!p->frame_dev && (p->frame < 0 || p->frame >= p->num_frames))) {
        emd_set_error("%s: bad pose tables / frame", who); return EMD_ERR_INVALID;
    }
    return EMD_OK;
}

}  // namespace

// d_emb[i] = d_mean[ids[i]] / count[ids[i]] per point (k_track_embed_bwd, embed.hip: no reduction), launched for emd_track_heads_backward and
// emd_track_heads_backward_det alike
int emd_launch_track_embed_bwd(int n, int E, const int32_t* ids, const float* count, const float* d_mean, float* d_emb, hipStream_t st);
