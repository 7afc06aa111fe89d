// te_gather_body.inc -- the table gradient of the temporal embedding in gather form, included textually inside k_temporal_embed_bwd_det
// (embed_det.hip) and k_track_chain_bwd_det (track_det.hip), the two backwards without atomics: what the gradient `g` of one column of sample `s` adds
// to element (R, c) of the table.  The includer has in scope: `acc` (double, the element's sum), `s` (TeSample), `wx0`, `wx1` (the column's weights),
// `m0`, `m1` (the column's x0 / its x1 is c), `g`, `R`.  The products are formed as the default kernels' scatter forms them (embed.hip, te_scatter) and
// added in its issue order -- r = 0, 1, then (ha, x0), (hb, x0), (ha, x1), (hb, x1) -- in double precision, without contraction.
// An include and not a function of temporal_sample.h: behind a __forceinline__ function k_temporal_embed_bwd_det came out with other instructions
// and 1.5 % slower at 32 tables of 32 columns (profiles/shared_source_isa.txt); with the text included both kernels kept theirs.
{
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (r == 1 && !s.in1) continue;
        const float wy = r ? s.wy1 : s.wy0;
        if (m0) {
            if (s.ha[r] == R) acc += (double)(g * wx0 * wy * s.la[r]);
            if (s.hb[r] == R) acc += (double)(g * wx0 * wy * s.lb[r]);
        }
        if (m1) {
            if (s.ha[r] == R) acc += (double)(g * wx1 * wy * s.la[r]);
            if (s.hb[r] == R) acc += (double)(g * wx1 * wy * s.lb[r]);
        }
    }
}
