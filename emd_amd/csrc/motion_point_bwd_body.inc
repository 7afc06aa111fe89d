// motion_point_bwd_body.inc -- the per-point half of the stand-alone motion backward, included textually inside k_motion_backward and
// k_motion_backward_det (standalone_ops.hip): one text, hence the same bits in d_means, d_quats, d_opac, d_rdx and d_rdq of both
// (tests/test_motion_det_gpu.py).  The includer has the kernels' common parameters in scope: n, means, quats, opac, mo, g_wm, g_wq, g_wo, d_means,
// d_quats, d_opac, d_rdx, d_rdq.  The text writes the per-point outputs and leaves `i` (the lane's point), `a_id` (its actor, -1: static or past the
// end) and pose_g[12] (its share of the actor's pose gradient; zeros for a static point), which each kernel reduces its own way.
    const int i = blockIdx.x * EMD_BLOCK + threadIdx.x;
    int a_id = -1;
    float pose_g[12];
#pragma unroll
    for (int k = 0; k < 12; k++) pose_g[k] = 0.f;
    if (i < n) {
        float dm[3] = {0.f, 0.f, 0.f}, dq[4] = {0.f, 0.f, 0.f, 0.f}, dop = 0.f;
        if (g_wm) { dm[0] = g_wm[3 * i]; dm[1] = g_wm[3 * i + 1]; dm[2] = g_wm[3 * i + 2]; }
        if (g_wq) { const float4 t = *(const float4*)(g_wq + 4 * i); dq[0] = t.x; dq[1] = t.y; dq[2] = t.z; dq[3] = t.w; }
        if (g_wo) dop = g_wo[i];
        a_id = mo.actor_id ? mo.actor_id[i] : -1;
        float dl[3] = {dm[0], dm[1], dm[2]}, dql[4] = {dq[0], dq[1], dq[2], dq[3]}, dopl = dop;
        if (a_id >= 0) motion_point_backward(i, a_id, means, quats, opac, mo, dm, dq, dop, dl, dql, &dopl, pose_g);
        if (d_means) { d_means[3 * i] = dl[0]; d_means[3 * i + 1] = dl[1]; d_means[3 * i + 2] = dl[2]; }
        if (d_rdx) { d_rdx[3 * i] = dl[0]; d_rdx[3 * i + 1] = dl[1]; d_rdx[3 * i + 2] = dl[2]; }
        if (d_quats) *(float4*)(d_quats + 4 * i) = make_float4(dql[0], dql[1], dql[2], dql[3]);
        if (d_rdq) *(float4*)(d_rdq + 4 * i) = a_id >= 0 ? make_float4(dql[0], dql[1], dql[2], dql[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (d_opac) d_opac[i] = dopl;
    }
