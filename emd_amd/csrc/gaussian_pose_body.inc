// gaussian_pose_body.inc -- part 1 of the projection backward for one visible Gaussian `i`: its loads and its world pose, included textually inside
// k_preprocess_backward (preprocess.hip) and k_camera_backward (camera_grad.hip): one text, hence the same fp32 intermediates in both.  (As functions
// of projection_math.h these lines moved K8's machine code: profiles/projection_shared_isa.txt.)
// EVERY load whose address depends on the index alone is issued back to back, before any of them is used -- the parameters, the accumulated gradient
// row, the colour Jacobian --, then the actor's pose rows (the one dependent address).  Optional inputs are read through a pointer that is valid either
// way (the Gaussian's own gradient row stands in for an absent array) and selected where they are used: a branch around a load would put it back
// behind a wait.  Then the world pose: motion_point's arithmetic on these values.  (K1 keeps a twin of its own in preprocess.hip: it has no gradient row.)
// The includer has in scope: a (PreBwdArgs), i, raw, z4c, the kernel-uniform motion, has_ids, has_rot, has_rdx, has_rdq, and
//   constexpr bool consume_row   K8: true.  false (the camera kernel, which runs before K8): the opacity is neither loaded nor formed and the
//                                gradient row is not handed back clean.
// and has declared what the text assigns: int a_id; float mloc[3], m[3], q[4], op, op_raw, q_norm; float4 q_raw, rdq, pr0, pr1, pr2.  The text also
// leaves the loaded s0..s2 (scales), g0..g2 (gradient row), j0..j2 (Jacobian rows) and `safe`, the stand-in pointer.
        const int aid_raw = *(has_ids ? a.motion.actor_id + i : a.radii + i);
        a_id = has_ids ? aid_raw : -1;
        float4* gr = (float4*)(a.grad_rec + (size_t)i * a.bwd_stride);
        const float* safe = (const float*)gr;                                          // 48 readable, 16-byte aligned bytes
        const float* mp = a.means3D + 3 * (size_t)i;
        const float* xp = has_rdx ? a.motion.residual_dx + 3 * (size_t)i : safe;
        const float* sp = a.cov3D_precomp ? safe : a.scales + 3 * (size_t)i;
        const float4* jr = a.colors_precomp ? (const float4*)gr : a.g.shjac + (size_t)i * 3;
        const float m0 = mp[0], m1 = mp[1], m2 = mp[2];
        const float x0 = xp[0], x1 = xp[1], x2 = xp[2];
        const float4 qq = *(const float4*)(has_rot ? a.rotations + 4 * (size_t)i : safe);
        const float4 dqq = *(const float4*)(has_rdq ? a.motion.residual_dq + 4 * (size_t)i : safe);
        const float opv = consume_row ? a.opacities[i] : 0.f;
        const float s0 = sp[0], s1 = sp[1], s2 = sp[2];
        const float4 g0 = gr[0], g1 = gr[1], g2 = gr[2];
        const float4 j0 = jr[0], j1 = jr[1], j2 = jr[2];
        if (a_id >= 0) {                              // the one dependent address
            const float4* Pp = (const float4*)(a.motion.actor_pose + (size_t)a_id * EMD_ACTOR_STRIDE);
            pr0 = Pp[0]; pr1 = Pp[1]; pr2 = Pp[2];
        }
        if (consume_row && (a.flags & EMD_FLAG_BWD_WS_CLEAN)) {          // the row is handed back clean: the next backward needs no zero fill
            gr[0] = z4c; gr[1] = z4c; gr[2] = z4c;
        }
        // ---- the Gaussian's world pose (motion_point's arithmetic on the values above)
        mloc[0] = has_rdx ? m0 + x0 : m0; mloc[1] = has_rdx ? m1 + x1 : m1; mloc[2] = has_rdx ? m2 + x2 : m2;
        q_raw = qq; rdq = dqq; op_raw = opv;
        if (motion) motion_apply(mloc, a_id, has_rot, q_raw, has_rdq, rdq, consume_row, op_raw, pr0, pr1, pr2, raw, m, q, &op);
        else {
            if (consume_row) op = raw ? sigmoidf_(op_raw) : op_raw;
            m[0] = m0; m[1] = m1; m[2] = m2;
            if (has_rot) { q[0] = qq.x; q[1] = qq.y; q[2] = qq.z; q[3] = qq.w; }
        }
        if (raw && a_id < 0 && has_rot) {   // static point: q is the raw quaternion (no-motion path) or already unit (motion path)
            const float qr[4] = {qq.x, qq.y, qq.z, qq.w};
            q_norm = fmaxf(quat_norm(qr), 1e-12f);
            q[0] = qr[0] / q_norm; q[1] = qr[1] / q_norm; q[2] = qr[2] / q_norm; q[3] = qr[3] / q_norm;
        }
