// cov2d_bwd_body.inc -- cov2D -> M = J W -> J -> the camera-space mean in the projection backward; included, and in its own file, as
// conic_bwd_body.inc is (K8 forms dL/dSigma between the two, and its machine code follows the order of the text).  The includer has in scope: Proj p,
// V, fx, fy, (da, db, dc) and g_depth.  The text leaves dM0[k], dM1[k] = dL/d(rows of M) and dt[3] = dL/dt: through J (a clamped x/z, y/z is a
// constant) and the depth image.
        float dM0[3], dM1[3], dJ00 = 0.f, dJ02 = 0.f, dJ11 = 0.f, dJ12 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            dM0[k] = 2.f * da * p.T0[k] + db * p.T1[k];
            dM1[k] = 2.f * dc * p.T1[k] + db * p.T0[k];
            dJ00 += dM0[k] * V[4 * k + 0]; dJ02 += dM0[k] * V[4 * k + 2];
            dJ11 += dM1[k] * V[4 * k + 1]; dJ12 += dM1[k] * V[4 * k + 2];
        }
        float tz2 = 1.f / (p.tz * p.tz), tz3 = tz2 / p.tz;
        float dt[3];
        dt[0] = p.clx ? 0.f : -fx * tz2 * dJ02;
        dt[1] = p.cly ? 0.f : -fy * tz2 * dJ12;
        dt[2] = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + 2.f * fx * p.cx * tz3 * dJ02 + 2.f * fy * p.cy * tz3 * dJ12;
        dt[2] += g_depth;
