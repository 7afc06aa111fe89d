// sh_dir_grad_body.inc -- the SH colour's gradient with respect to the view direction, included textually inside k_preprocess_backward
// (preprocess.hip) and k_camera_backward (camera_grad.hip): one text, hence the same fp32 intermediates in both.  (As functions of projection_math.h
// these lines moved K8's machine code: profiles/projection_shared_isa.txt.)  The includer has in scope: S, the world mean m, the Jacobian rows j0, j1,
// j2 that K1 stored and the accumulated gcol[3].  The text leaves d = (m - campos) / n, gc = dL/d colour under the clamp bits, gd = J^T gc (no second
// pass over the 192 B of coefficients) and dot = d . gd: dL/dm = -dL/d campos = (gd - d dot) / n.
            float d0[3] = {m[0] - S.campos[0], m[1] - S.campos[1], m[2] - S.campos[2]};
            float n = sqrtf((d0[0] * d0[0] + d0[1] * d0[1]) + d0[2] * d0[2]);
            float d[3] = {d0[0] / n, d0[1] / n, d0[2] / n};
            const uint32_t bits = __float_as_uint(j0.w);        // (the clamp bits K1 left in the row's spare word)
            float gc[3];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) gc[ch] = ((bits >> ch) & 1u) ? 0.f : gcol[ch];
            float gd[3];
            gd[0] = (j0.x * gc[0] + j1.x * gc[1]) + j2.x * gc[2];
            gd[1] = (j0.y * gc[0] + j1.y * gc[1]) + j2.y * gc[2];
            gd[2] = (j0.z * gc[0] + j1.z * gc[1]) + j2.z * gc[2];
            float dot = (d[0] * gd[0] + d[1] * gd[1]) + d[2] * gd[2];
