// conic_bwd_body.inc -- conic -> cov2D in the projection backward, included textually inside k_preprocess_backward (preprocess.hip) and
// k_camera_backward (camera_grad.hip): one text, hence the same fp32 intermediates in both.  (As a function of projection_math.h these lines moved
// K8's machine code: profiles/projection_shared_isa.txt.)  The includer has in scope: Proj p after project_cov2d and the accumulated gA, gB, gC.  The
// text leaves (da, db, dc) = dL/d(a, b, c).
        float da = 0.f, db = 0.f, dc = 0.f;
        if (p.det != 0.f) {
            float i2 = 1.f / (p.det * p.det);
            da = (-p.c * p.c * gA + p.b * p.c * gB - p.b * p.b * gC) * i2;
            db = (2.f * p.b * p.c * gA - (p.a * p.c + p.b * p.b) * gB + 2.f * p.a * p.b * gC) * i2;
            dc = (-p.b * p.b * gA + p.a * p.b * gB - p.a * p.a * gC) * i2;
        }
