// sky_pixel_bwd_body.inc -- the per-pixel half of the sky cube-map backward, included textually inside k_sky_backward (sky.hip) and k_sky_det_rows
// (sky_det.hip): one text, hence the same expressions in the same order and the same bits in dL_dfg and dL_dacc (tests/test_sky_det_gpu.py).  It is an
// include and not a function: with the statements behind a function the default kernel's registers were allocated differently, and that kernel keeps
// its instructions (profiles/shared_source_isa.txt).
// The includer has in scope: `b` (EmdSkyBwdArgs), `a` (= b.f), `P` (pixels), `p` (the lane's pixel), `px`, `py` (its column and row), `valid` (the lane
// has a pixel), `res` (= a.resolution).  The text writes dL_dfg and dL_dacc of the pixel and leaves what the cube-map gradient is made of: `sampled`,
// the taps `tp` (set only when sampled) and gs[c] = dL/d(sky colour c) behind the clamp (tap k adds tp.w[k] * gs[c] to its texel); `acc`, `il`, `pcl`,
// `blend` and the *_raw inputs are declared here too.
    float acc = 0.f, gs[3] = {0.f, 0.f, 0.f};
    bool sampled = false;
    Tap tp;
    const bool il = (a.flags & EMD_SKY_INTERLEAVED) != 0;
    // the pixel's inputs first, unconditionally (an absent input reads the cube map's first texel and is not used; a pixel outside the image reads
    // pixel 0): with the loads inside the branches that use them the thread made a trip to memory per input, one after the other
    const size_t pcl = valid ? p : 0;
    const bool blend = b.dL_dout && a.fg;
    const float acc_raw = *(a.acc ? a.acc + pcl : a.cube);
    float gsky_raw[3], gout_raw[3], fg_raw[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const size_t q = il ? 3 * pcl + c : (size_t)c * P + pcl;
        gsky_raw[c] = *(b.dL_dsky ? b.dL_dsky + q : a.cube);
        gout_raw[c] = *(blend ? b.dL_dout + q : a.cube);
        fg_raw[c] = *(blend ? a.fg + q : a.cube);
    }
    if (valid) {
        acc = a.acc ? acc_raw : 0.f;
        sampled = !(a.acc && a.mask_threshold >= 0.f) || (1.f - acc) > a.mask_threshold;
        float s[3] = {a.fill, a.fill, a.fill};
        bool pass[3] = {false, false, false};
        if (sampled) {
            float dx, dy, dz;
            pixel_ray(a, px, py, p, dx, dy, dz);
            cube_taps(dx, dy, dz, res, tp);
            s[0] = s[1] = s[2] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float* t = a.cube + (size_t)tp.idx[k] * 3;
                s[0] += tp.w[k] * t[0]; s[1] += tp.w[k] * t[1]; s[2] += tp.w[k] * t[2];
            }
#pragma unroll
            for (int c = 0; c < 3; c++) pass[c] = !(a.flags & EMD_SKY_CLAMP01) || (s[c] >= 0.f && s[c] <= 1.f);   // torch.clamp backward
        }
        if (a.flags & EMD_SKY_CLAMP01) {
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] = fminf(fmaxf(s[c], 0.f), 1.f);
        }
        float dacc = 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const size_t q = il ? 3 * p + c : (size_t)c * P + p;
            gs[c] = b.dL_dsky ? gsky_raw[c] : 0.f;
            if (blend) {
                const float g = gout_raw[c], f = fg_raw[c];
                gs[c] += g * (1.f - acc);
                if (a.flags & EMD_SKY_BLEND_S3G) { dacc += g * (f - s[c]); if (b.dL_dfg) b.dL_dfg[q] = g * acc; }
                else { dacc -= g * s[c]; if (b.dL_dfg) b.dL_dfg[q] = g; }
            }
            if (!pass[c]) gs[c] = 0.f;
        }
        if (b.dL_dacc) b.dL_dacc[p] = dacc;
    }
