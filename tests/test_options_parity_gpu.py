"""-m gpu: the rasterizer options the main parity suite leaves at their defaults, each against the CPU oracle.

  - a loss on the normal image (K7 with NORMAL=true: six per-pixel LDS planes instead of four), across absgrad and 0 / 1 / 2 extra
    colour sets -- every non-diagnostic instantiation of k_render_backward_q and k_render_forward_q;
  - scale_modifier (K1 scales the covariance with it, K8 chains dL/dscales through it);
  - RasterOptions.clamp_rgb01 (the clamp bits K1 records and K8 / the SH factor read), with aux_stream and factored_sh_grad;
  - RasterOptions.near_plane (the cull, and the offset of the three-pass depth-sort keys).
Bars: tests/helpers.py's, unchanged (compare_forward: keys / ids / images bit-exact; compare_backward: render backward, projection
backward on the kernel's own render gradients, end to end).  Every case asserts that the option actually changed something.

Which case reaches which render kernel (test_render_instantiations_against_the_oracle[normal-absgrad-extraX]):
  k_render_forward_q<false, X>           no-normal-image-*-extraX                   (compute_normal off)
  k_render_forward_q<true, X>            normal-image-*-extraX, normal-loss-*-extraX
  k_render_backward_q<false, false, X>   no-normal-image-noabs-extraX, normal-image-noabs-extraX
  k_render_backward_q<false, true, X>    no-normal-image-absgrad-extraX, normal-image-absgrad-extraX
  k_render_backward_q<true, false, X>    normal-loss-noabs-extraX (+ the normal-only and deep-list tests for X = 0)
  k_render_backward_q<true, true, X>     normal-loss-absgrad-extraX
for X in {0, 1, 2}."""
import numpy as np
import pytest
import torch

from oracle import cpu_oracle as co
from tests.helpers import (IMAGE_TOL, assert_grad_close, boost_dc, clamp_counts, compare_backward, compare_forward, make_case,
                           place_in_depth_band, raw_params_parity, run_hip, run_oracle, run_oracle_extra_sets)

pytestmark = pytest.mark.gpu


def _parity(case, **kw):
    orc = run_oracle(case, backward=True)
    hip = run_hip(case, backward=True, **kw)
    compare_forward(hip, orc, tol=IMAGE_TOL)
    checked = compare_backward(hip, orc)
    assert "means3D" in checked and "opacities" in checked
    return hip, orc


def _visible(orc):
    return int((orc["pre"]["radii"] > 0).sum())


# ---- the normal image's gradient: every K7 instantiation ---------------------------------------------------------------------

def _extra_set_losses(case, n_extra, disjoint, seed):
    """Colour sets and their image gradients.  With `disjoint` every pixel carries the loss of ONE colour set only (main: colour,
    depth, alpha and normal; extra set k: its image): then each pixel's gradient is that of a single pass, and the absgrad sums of
    the one call equal the sum of the separate passes' (|a + b| = |a| + |b| when one of them is zero)."""
    g = torch.Generator().manual_seed(seed)
    H, W = case["H"], case["W"]
    feats = [torch.rand(case["N"], 3, generator=g) for _ in range(n_extra)]
    dX = [torch.randn(3, H, W, generator=g).numpy() for _ in range(n_extra)]
    if disjoint:
        owner = (np.arange(H)[:, None] + np.arange(W)[None, :]) % (1 + n_extra)
        case = dict(case)
        for k in ("dL_dcolor", "dL_ddepth", "dL_dalpha", "dL_dnormal"):
            if case[k] is not None:
                case[k] = (case[k] * (owner == 0)[None]).astype(np.float32)
        dX = [(d * (owner == 1 + k)[None]).astype(np.float32) for k, d in enumerate(dX)]
    return case, feats, dX


@pytest.mark.parametrize("n_extra", [0, 1, 2], ids=lambda v: f"extra{v}")
@pytest.mark.parametrize("absgrad", [False, True], ids=["noabs", "absgrad"])
@pytest.mark.parametrize("normal", ["no-normal-image", "normal-image", "normal-loss"])
def test_render_instantiations_against_the_oracle(normal, absgrad, n_extra):
    """k_render_forward_q<NORMAL, NX> and k_render_backward_q<NORMAL, ABS, NX>: NORMAL of the forward is the normal image
    (RasterOptions.compute_normal), NORMAL of the backward a gradient on it.  Extra colour sets: the reference is the main oracle pass
    plus one colors_precomp pass per set, gradients of the shared inputs summed."""
    case = make_case(n=3000, H=64, W=96, seed=101 + n_extra, normal_loss=(normal == "normal-loss"))
    if normal == "no-normal-image":
        case["flags"] &= ~co.F_NORMAL
    case, feats, dX = _extra_set_losses(case, n_extra, disjoint=absgrad, seed=7 + n_extra)
    if n_extra:
        orc = run_oracle_extra_sets(case, feats, dX)
    else:
        orc = run_oracle(case, backward=True)
    hip = run_hip(case, backward=True, absgrad=absgrad, colors_extra=feats or None, dL_dextra=dX or None)
    compare_forward(hip, orc, tol=IMAGE_TOL)
    names = None if absgrad else ("means3D", "means2D", "shs", "opacities", "scales", "rotations")
    checked = compare_backward(hip, orc, names=names)
    assert ("means2D_abs" in checked) == absgrad
    for k, of in enumerate(orc.get("extra", [])):
        nz = int((hip["extra"][k].view(np.uint32) != of["img"]["color"].view(np.uint32)).sum())
        assert nz == 0, f"extra image {k}: {nz} values differ from the oracle's"
        assert_grad_close(hip["render_grads"][f"rgb_extra{k}"], of["grads"]["render_grads"]["rgb"], f"render:rgb_extra{k}")
        assert_grad_close(hip["grads"]["colors_extra"][k], of["grads"]["colors"], f"colors_extra[{k}]")
    if normal == "no-normal-image":
        assert not hip["normal"].any()
    else:
        assert np.abs(hip["normal"]).max() > 0.1
    if absgrad:
        assert np.abs(hip["grads"]["means2D_abs"]).max() > 0


def test_normal_only_loss_moves_opacity_and_pixel_means():
    """dL/dcolor = dL/ddepth = dL/dalpha = 0: every gradient comes from the normal image (the dN term of K7's per-pixel g).  The
    images of the call are those of the same call without the normal loss, bit for bit."""
    case = make_case(n=3000, H=64, W=96, seed=111, normal_loss=True)
    for k in ("dL_dcolor", "dL_ddepth", "dL_dalpha"):
        case[k] = np.zeros_like(case[k])
    hip, orc = _parity(case)
    for k in ("opacities", "means2D"):
        assert np.abs(orc["grads"][k]).max() > 0 and np.abs(hip["grads"][k]).max() > 0, k
    assert np.abs(hip["render_grads"]["conic"]).max() > 0
    plain = run_hip(dict(case, dL_dnormal=None), backward=True)
    for k in ("color", "depth", "alpha", "normal"):
        np.testing.assert_array_equal(hip[k].view(np.uint32), plain[k].view(np.uint32), err_msg=k)
    assert not np.abs(plain["grads"]["opacities"]).any()        # (without the normal loss this case has no loss at all)


def test_normal_loss_on_deep_tile_lists_and_with_every_pair_kept():
    """Deep lists (thousands of entries per tile, many 64-entry batches) with NORMAL=true: PB = 6 changes the staging of every
    batch.  keep_all_pairs=True (upstream's full list) gives the same images and gradients to the bar."""
    case = make_case(n=80000, H=96, W=128, seed=9, scale_mult=1.0, normal_loss=True)
    hip, orc = _parity(case)
    assert int(np.diff(orc["bin"]["ranges"].astype(np.int64), axis=1).max()) > 1000
    full = run_hip(case, backward=True, keep_all_pairs=True)
    compare_forward(full, orc, tol=IMAGE_TOL)
    assert full["status"]["num_rendered"] == orc["bin"]["D"] >= hip["status"]["num_rendered"]
    for k in ("color", "depth", "alpha", "normal", "radii"):
        np.testing.assert_array_equal(full[k], hip[k], err_msg=k)
    compare_backward(full, orc)


# ---- scale_modifier ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mod", [0.5, 1.7])
@pytest.mark.parametrize("scene", ["static", "motion-residual"])
def test_scale_modifier(scene, mod):
    kw = dict(motion=True, residual=True) if scene == "motion-residual" else {}
    case = make_case(n=3000, H=64, W=96, seed=121, scale_modifier=mod, **kw)
    hip, orc = _parity(case)
    ref = run_oracle(dict(case, scale_modifier=1.0))
    assert not np.array_equal(orc["pre"]["radii"], ref["pre"]["radii"])          # the modifier changes the footprints


@pytest.mark.parametrize("mod", [0.5, 1.7])
@pytest.mark.parametrize("motion", [False, True], ids=["static", "motion"])
def test_scale_modifier_with_fused_activations(motion, mod):
    case = make_case(n=3000, H=64, W=96, seed=131, motion=motion, scale_modifier=mod)
    g = torch.Generator().manual_seed(5)
    log_s = torch.log(case["scales"])
    raw_q = case["rotations"] * (0.5 + torch.rand(case["N"], 1, generator=g))
    logit = torch.logit(case["opacities"].clamp(1e-4, 1 - 1e-4))
    res = raw_params_parity(case, log_s, raw_q, logit)
    assert res["V"] > 1000


def test_scale_modifier_does_not_touch_a_precomputed_covariance():
    """With cov3Ds_precomp the modifier has nothing to scale: the projection, the list and the images are those of the 1.0 call bit
    for bit.  (The gradients are float-atomic sums, whose order differs from call to call: they meet the bar against the oracle,
    which gives the 1.0 and the 1.7 call the same gradients bit for bit.)"""
    case = make_case(n=3000, H=64, W=96, seed=141, cov_precomp=True)
    one = run_hip(case, backward=True)
    case_m = dict(case, scale_modifier=1.7)
    mod = run_hip(case_m, backward=True)
    orc, orc_m = run_oracle(case, backward=True), run_oracle(case_m, backward=True)
    for k in ("means3D", "means2D", "opacities", "cov3D"):
        np.testing.assert_array_equal(orc_m["grads"][k], orc["grads"][k], err_msg="oracle " + k)
    compare_forward(mod, orc_m, tol=IMAGE_TOL)
    compare_backward(mod, orc_m)
    for k in ("color", "depth", "alpha", "normal", "radii", "keys", "ids", "ranges"):
        np.testing.assert_array_equal(mod[k], one[k], err_msg=k)
    for k, v in one["geo"].items():
        if v is not None:
            np.testing.assert_array_equal(mod["geo"][k], v, err_msg="projection: " + k)


def test_scale_modifier_through_the_device_settings_call_site():
    """The reference's call site: camera settings as device tensors (one device block, EmdFwdArgs.settings_dev) and no_sync.  The
    modifier travels in the settings copy of the call, not in the block: the kernels must read it from there."""
    case = make_case(n=3000, H=64, W=96, seed=151, scale_modifier=1.7)
    run_hip(case, backward=False)                          # a synchronising call sizes the binning workspace for the no_sync one
    hip = run_hip(case, backward=True, no_sync=True)
    assert hip["call"].num_rendered == -1 and hip["call"].settings_dev is not None
    orc = run_oracle(case, backward=True)
    compare_forward(hip, orc, tol=IMAGE_TOL)
    compare_backward(hip, orc)


# ---- clamp_rgb01 ------------------------------------------------------------------------------------------------------------

def _clamp_case(seed, **kw):
    case = make_case(n=3000, H=64, W=96, seed=seed, clamp01=True, **kw)
    boost_dc(case, seed=seed)
    return case


def _assert_clamps(orc):
    above, below = clamp_counts(orc)
    assert above >= 0.1 * 3 * _visible(orc) and below > 0, (above, below, _visible(orc))


@pytest.mark.parametrize("aux_stream", [False, True], ids=["one-stream", "aux-stream"])
@pytest.mark.parametrize("motion", [False, True], ids=["static", "motion"])
def test_clamp_rgb01(motion, aux_stream):
    case = _clamp_case(161, motion=motion)
    hip, orc = _parity(case, aux_stream=aux_stream)
    _assert_clamps(orc)
    # the clamp is the option's doing: without it the same scene renders other colours
    assert not np.array_equal(run_oracle(dict(case, flags=case["flags"] & ~co.F_CLAMP01))["img"]["color"], hip["color"])


def test_clamp_rgb01_with_the_factored_sh_gradient():
    """factored_sh_grad: the backward publishes the clamp-masked [N,3] colour factor (k_sh_factor reads the clamp bits K1 left in the
    record); the dense dL/dshs rebuilt from it must be the oracle's."""
    from emd_amd import dp
    case = _clamp_case(171)
    orc = run_oracle(case, backward=True)
    _assert_clamps(orc)
    out = run_hip(case, backward=True, factored_sh_grad=True)
    assert out["grads"]["shs"] is None
    dev = torch.device("cuda", 0)
    campos = torch.as_tensor(case["cam"].camera_center, dtype=torch.float32).reshape(1, 3).to(dev)
    got = dp.sh_grad_from_factors(case["means3D"].to(dev), campos, out["call"].sh_color_grad.clone()[None], case["sh_degree"], 16,
                                  scale=1.0).cpu().numpy()
    assert_grad_close(got, orc["grads"]["shs"], "shs rebuilt from the factor")


def test_clamp_rgb01_leaves_precomputed_colours_alone():
    """The clamp belongs to the SH colour (raster_oracle.c: only the SH path clamps): colors_precomp outside [0, 1] are used as given."""
    case = make_case(n=3000, H=64, W=96, seed=181, colors_precomp=True, clamp01=True)
    case["colors_precomp"] = case["colors_precomp"] * 2.0 - 0.5
    hip, orc = _parity(case)
    vis = orc["pre"]["radii"] > 0
    assert (orc["pre"]["rgb"][vis] > 1.0).sum() > 100 and (orc["pre"]["rgb"][vis] < 0.0).sum() > 100


# ---- near_plane -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("near,band", [(0.05, (0.05, 0.2)), (1.0, (0.2, 1.0))], ids=["near0.05", "near1.0"])
def test_near_plane_culls_the_band(near, band):
    case = make_case(n=3000, H=64, W=96, seed=191, near_plane=near)
    place_in_depth_band(case, np.arange(180, 780), *band, seed=191)
    hip, orc = _parity(case)
    v, v0 = _visible(orc), _visible(run_oracle(dict(case, near_plane=0.2)))
    assert hip["status"]["num_visible"] == v and abs(v - v0) > 100, (v, v0)


def _far_case(seed, depth, H, W):
    case = make_case(n=3000, H=H, W=W, seed=seed, near_plane=0.01)
    place_in_depth_band(case, np.arange(60, 90), 0.01, 0.2, seed=seed)      # some Gaussians between the near plane and 0.2 as well
    z = place_in_depth_band(case, np.arange(90, 92), depth, depth + 1.0, seed=seed + 1)
    case["scales"][90:92] = 2.0
    return case, z


@pytest.mark.parametrize("depth,wide", [(600.0, False), (700.0, True)], ids=["600m-narrow", "700m-wide"])
def test_three_pass_depth_range_at_a_small_near_plane(depth, wide):
    """At near = 0.01 the three-pass depth sort covers 65 536 x 0.01 = 655 m: a visible Gaussian at 600 m stays on it, one at 700 m
    makes the call fall back to the four-pass sort.  Either way keys, ids and images are the oracle's."""
    from emd_amd import rasterizer
    case, _ = _far_case(201, depth, 64 + 16 * wide, 96)
    key = (0, case["H"], case["W"])
    rasterizer._wide_depth.discard(key)
    try:
        orc = run_oracle(case, backward=True)
        assert (orc["pre"]["radii"][90:92] > 0).all() and (orc["pre"]["depths"][90:92] > depth).all()
        assert (orc["pre"]["radii"][60:90] > 0).sum() > 10
        hip = run_hip(case, backward=True)
        assert (key in rasterizer._wide_depth) == wide
        compare_forward(hip, orc, tol=IMAGE_TOL)
        compare_backward(hip, orc)
        full = run_hip(case, backward=False, keep_all_pairs=True)
        compare_forward(full, orc, tol=IMAGE_TOL)
    finally:
        rasterizer._wide_depth.discard(key)


@pytest.mark.parametrize("near", [0.0, -0.1])
def test_near_plane_at_or_below_zero_takes_the_wide_sort(near):
    """A near plane <= 0 puts every depth beyond the three-pass range (the keys are offset by max(near, 0)): the binding renders
    through the four-pass sort, and the result is the oracle's."""
    from emd_amd import rasterizer
    case = make_case(n=3000, H=48, W=80, seed=211, near_plane=near)
    place_in_depth_band(case, np.arange(60, 360), 0.0, 0.2, seed=211)
    key = (0, case["H"], case["W"])
    rasterizer._wide_depth.discard(key)
    try:
        hip, orc = _parity(case)
        assert key in rasterizer._wide_depth
        assert _visible(orc) - _visible(run_oracle(dict(case, near_plane=0.2))) > 100
    finally:
        rasterizer._wide_depth.discard(key)
