"""-m gpu: the SH colour beside the rasterizer -- k_sh_forward, k_sh_backward, k_sh_grad_from_factors (csrc/standalone_ops.hip) and the callers
that reach them -- against the fp64 restatement of tests/sh_ref.py at every degree, with 16 coefficient rows and with exactly (degree + 1)^2, at
row counts on both sides of a 256-lane block and of the 128-row halves of the staged row store.  The bar is the project's criterion
(DESIGN.md section 5), which the same formula in plain fp32 meets with an order of magnitude to spare (tests/test_sh_paths_cpu.py, where the
conditions on the inputs are asserted too); zeros and untouched rows are compared by bit pattern.  Groups, as the printed lines are tagged:
  a  forward and backward through gsplat_api.spherical_harmonics        d  argument checks of the C entry points
  b  rows the degree does not use never reach a result                  e  dp.sh_grad_from_factors against the sum over views
  c  every output element is written, nothing past row N                f  the degree ramp through nodes.rigid_gaussians, model.pre_compute_colors"""
import ctypes as C

import pytest
import torch

from emd_amd import _lib as L
from emd_amd import dp, gsplat_api
from emd_amd.rasterizer import _fill_motion
from tests import sh_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def _run_sh(deg, dirs, coeffs, g, dirs_grad=True):
    """-> colour, dL/dcoeffs, dL/ddirs (None when the directions are detached: the kernel gets d_dirs == NULL)."""
    d = dirs.detach().clone().requires_grad_(dirs_grad)
    c = coeffs.detach().clone().requires_grad_(True)
    out = gsplat_api.spherical_harmonics(deg, d, c)
    (out * g).sum().backward()
    return out.detach(), c.grad, d.grad


def _on_device(case, *keys):
    return [None if case[k] is None else case[k].to(DEV) for k in keys]


# ---- a ----

@pytest.mark.parametrize("deg,M,N", R.SH_CASES)
def test_a_forward_and_backward_match_the_reference(deg, M, N):
    case, ref = R.sh_case(deg, M, N), R.sh_reference(deg, M, N)
    dirs, coeffs, g = _on_device(case, "dirs", "coeffs", "g")
    colour, d_coeffs, d_dirs = _run_sh(deg, dirs, coeffs, g)
    tag = f"a: deg {deg} M {M} N {N}"
    R.criterion(colour, ref["colour"], tag + " colour")
    R.criterion(d_coeffs, ref["d_coeffs"], tag + " dL/dcoeffs")
    R.criterion(d_dirs, ref["d_dirs"], tag + " dL/ddirs")
    assert d_coeffs.shape == (N, M, 3)
    assert bool((_bits(d_coeffs[:, case["K"]:]) == 0).all()), "rows >= (deg + 1)^2 of dL/dcoeffs are +0"
    if deg == 0:
        assert bool((_bits(d_dirs) == 0).all()), "dL/ddirs at degree 0 is +0"
    colour2, d_coeffs2, none = _run_sh(deg, dirs, coeffs, g, dirs_grad=False)
    assert none is None
    assert _same_bits(colour2, colour) and _same_bits(d_coeffs2, d_coeffs), "d_dirs == NULL changes nothing else"


def test_a_batched_leading_dims_and_a_strided_view_equal_the_flat_call():
    deg, M, N = 2, 16, 257
    case = R.sh_case(deg, M, 1000)
    dirs, coeffs, g = (t[:2 * N] for t in _on_device(case, "dirs", "coeffs", "g"))
    flat = _run_sh(deg, dirs, coeffs, g)
    strided = coeffs.reshape(2, N, M, 3).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not strided.is_contiguous() and torch.equal(strided.reshape(2 * N, M, 3), coeffs)
    got = _run_sh(deg, dirs.reshape(2, N, 3), strided, g.reshape(2, N, 3))
    assert got[0].shape == (2, N, 3) and got[1].shape == (2, N, M, 3) and got[2].shape == (2, N, 3)
    for a, b, what in zip(got, flat, ("colour", "dL/dcoeffs", "dL/ddirs")):
        assert _same_bits(a.reshape(b.shape), b), what
    R.criterion(flat[0], R.sh_reference(deg, M, 1000)["colour"][:2 * N], "a: batched call, colour")


# ---- b ----

@pytest.mark.parametrize("deg", [0, 1, 2])
@pytest.mark.parametrize("fill", [float("nan"), float("inf")])
def test_b_unused_rows_are_not_read_into_the_result(deg, fill):
    case = R.sh_case(deg, 16, 257)
    dirs, coeffs, g = _on_device(case, "dirs", "coeffs", "g")
    clean = _run_sh(deg, dirs, coeffs, g)
    dirty = coeffs.clone()
    dirty[:, case["K"]:] = fill
    got = _run_sh(deg, dirs, dirty, g)
    for a, b, what in zip(got, clean, ("colour", "dL/dcoeffs", "dL/ddirs")):
        assert bool(torch.isfinite(a).all()), what
        assert _same_bits(a, b), what


# ---- c ----

@pytest.mark.parametrize("deg,M", [(1, 16), (2, 9)])
def test_c_every_output_element_is_written_and_nothing_past_row_n(deg, M):
    N = 257
    lib, case, ref = L.load(), R.sh_case(deg, M, N), R.sh_reference(deg, M, N)
    dirs, coeffs, g = _on_device(case, "dirs", "coeffs", "g")
    rgb, d_coeffs, d_dirs = _nan(N + 1, 3), _nan(N + 1, M, 3), _nan(N + 1, 3)
    assert lib.emd_sh_forward(N, deg, M, dirs.data_ptr(), coeffs.data_ptr(), rgb.data_ptr(), L.stream()) == L.EMD_OK
    assert lib.emd_sh_backward(N, deg, M, dirs.data_ptr(), coeffs.data_ptr(), g.data_ptr(), d_coeffs.data_ptr(), d_dirs.data_ptr(), L.stream()) == L.EMD_OK
    for buf, key in ((rgb, "colour"), (d_coeffs, "d_coeffs"), (d_dirs, "d_dirs")):
        assert not bool(torch.isnan(buf[:N]).any()), key
        assert bool(torch.isnan(buf[N]).all()), key + ": the row past N is untouched"
        R.criterion(buf[:N], ref[key], f"c: deg {deg} M {M} N {N} {key} through the C entry")


# ---- d ----

def test_d_argument_checks_refuse_and_launch_nothing():
    lib, deg, M, N = L.load(), 1, 16, 257
    case = R.sh_case(deg, M, N)
    dirs, coeffs, g = _on_device(case, "dirs", "coeffs", "g")
    rgb, d_coeffs, d_dirs = _nan(N, 3), _nan(N, M, 3), _nan(N, 3)
    p = lambda t: t.data_ptr()
    fwd = lambda n=N, d=deg, m=M, a=p(dirs), b=p(coeffs), c=p(rgb): lib.emd_sh_forward(n, d, m, a, b, c, L.stream())
    bwd = lambda n=N, d=deg, m=M, a=p(dirs), b=p(coeffs), c=p(g): lib.emd_sh_backward(n, d, m, a, b, c, p(d_coeffs), p(d_dirs), L.stream())
    for call in (fwd, bwd):
        assert call(d=-1) == L.EMD_ERR_INVALID
        assert call(d=4) == L.EMD_ERR_INVALID
        assert call(d=1, m=3) == L.EMD_ERR_INVALID and call(d=2, m=8) == L.EMD_ERR_INVALID and call(d=3, m=15) == L.EMD_ERR_INVALID
        assert call(a=None) == L.EMD_ERR_INVALID and call(b=None) == L.EMD_ERR_INVALID and call(c=None) == L.EMD_ERR_INVALID
    torch.cuda.synchronize()
    for buf in (rgb, d_coeffs, d_dirs):
        assert bool(torch.isnan(buf).all()), "a refused call writes nothing"
    assert fwd() == L.EMD_OK and bwd() == L.EMD_OK                      # the same arguments, unbroken, are accepted
    assert not bool(torch.isnan(rgb).any() | torch.isnan(d_coeffs).any() | torch.isnan(d_dirs).any())
    with pytest.raises(ValueError, match="fewer than"):
        gsplat_api.spherical_harmonics(2, dirs, coeffs[:, :8])
    with pytest.raises(ValueError, match="mismatch"):
        gsplat_api.spherical_harmonics(1, dirs[:-1], coeffs)
    with pytest.raises(ValueError, match="mismatch"):
        gsplat_api.spherical_harmonics(1, dirs, coeffs[..., :2])


def _factors_c(case, deg, rows, scale, out):
    """emd_sh_grad_from_factors into a buffer of the caller (dp.sh_grad_from_factors allocates its own)."""
    means, campos, factors, ids, pose, rdx = _on_device(case, "means", "campos", "factors", "ids", "pose", "rdx")
    ids = None if ids is None else ids.to(torch.int32)
    per_view = pose is not None and pose.dim() == 3
    mo = L.EmdMotion()
    _fill_motion(mo, ids, pose if not per_view else pose[0], rdx, None)
    if per_view:
        mo.actor_pose = pose.data_ptr()
    rc = L.load().emd_sh_grad_from_factors(case["N"], case["V"], deg, rows, means.data_ptr(), C.byref(mo), 1 if per_view else 0, campos.data_ptr(),
                                           factors.data_ptr(), float(scale), out.data_ptr(), L.stream())
    torch.cuda.synchronize()                                            # (the device copies above live until the launch has run)
    return rc


def test_d_dense_gradient_needs_sixteen_rows():
    """The staged row store of k_sh_grad_from_factors writes 192-byte rows: 4 rows at degree 1 are refused, not mis-strided."""
    case = R.factor_case(1, 2, 257, "shared")
    out = _nan(257, 4, 3)
    assert _factors_c(case, 1, 4, 1.0, out) == L.EMD_ERR_INVALID
    assert bool(torch.isnan(out).all())
    means, campos, factors, ids, pose = _on_device(case, "means", "campos", "factors", "ids", "pose")
    with pytest.raises(L.EmdError, match="sh_coeffs == 16"):
        dp.sh_grad_from_factors(means, campos, factors, 1, 4, actor_ids=ids, actor_pose=pose)
    assert _factors_c(case, 1, 3, 1.0, out) == L.EMD_ERR_INVALID and _factors_c(case, 1, 17, 1.0, _nan(257, 17, 3)) == L.EMD_ERR_INVALID
    assert _factors_c(case, 4, 16, 1.0, _nan(257, 16, 3)) == L.EMD_ERR_INVALID and _factors_c(case, -1, 16, 1.0, _nan(257, 16, 3)) == L.EMD_ERR_INVALID


# ---- e ----

def _check_factors(deg, V, N, form, scale):
    case, ref = R.factor_case(deg, V, N, form), R.factor_reference(deg, V, N, form, scale)
    means, campos, factors, ids, pose, rdx = _on_device(case, "means", "campos", "factors", "ids", "pose", "rdx")
    got = dp.sh_grad_from_factors(means, campos, factors, deg, 16, actor_ids=ids, actor_pose=pose, residual_dx=rdx, scale=scale)
    assert got.shape == (N, 16, 3)
    R.criterion(got, ref, f"e: deg {deg} V {V} N {N} {form} scale {scale:.3f}")
    assert bool((_bits(got[:, case["K"]:]) == 0).all()), "rows >= (deg + 1)^2 are +0"
    unseen = case["zero"].all(0).to(DEV)
    assert bool((got[unseen] == 0).all()), "a Gaussian whose factor is zero in every view gets a zero row"
    out = _nan(N + 1, 16, 3)
    assert _factors_c(case, deg, 16, scale, out) == L.EMD_OK
    assert not bool(torch.isnan(out[:N]).any()) and bool(torch.isnan(out[N]).all())
    assert _same_bits(out[:N], got)


@pytest.mark.parametrize("deg,V,N", R.FACTOR_SWEEP)
def test_e_dense_gradient_from_factors_sweep(deg, V, N):
    _check_factors(deg, V, N, "shared", 1.0 / V)


@pytest.mark.parametrize("deg,V,N,form,scale", R.FACTOR_FORM_CASES)
def test_e_dense_gradient_from_factors_forms(deg, V, N, form, scale):
    _check_factors(deg, V, N, form, scale)


# ---- f ----

_NODE_KEYS = ("_means", "_opacities", "_rgbs", "_scales", "_quats")


def _run_nodes(case, colour_gradient):
    from emd_amd.nodes import rigid_gaussians
    names = ("means", "quats", "opacity_logits", "log_scales", "features_dc", "features_rest")
    leaf = {k: case[k].to(DEV).requires_grad_(True) for k in names}
    gs = rigid_gaussians(leaf["means"], leaf["quats"], leaf["opacity_logits"], leaf["log_scales"], leaf["features_dc"], leaf["features_rest"],
                         case["point_ids"].to(DEV), case["actor_pose"].to(DEV), case["camera_center"].to(DEV), sh_degree=case["sh_degree"],
                         step=case["step"], sh_degree_interval=R.NODE_INTERVAL)
    up = {k: case["g" + k].to(DEV) for k in _NODE_KEYS}
    if not colour_gradient:
        up["_rgbs"] = torch.zeros_like(up["_rgbs"])
    sum((gs[k] * up[k]).sum() for k in _NODE_KEYS).backward()
    return gs, leaf


@pytest.mark.parametrize("sh_degree,step", R.NODE_CASES)
def test_f_degree_ramp_through_rigid_gaussians(sh_degree, step):
    case, ref = R.node_case(sh_degree, step), R.node_reference(sh_degree, step)
    gs, leaf = _run_nodes(case, True)
    tag = f"f: nodes sh_degree {sh_degree} step {step} (n = {case['n']}, {case['features_rest'].shape[1] + 1} rows)"
    R.criterion(gs["_rgbs"], ref["colour"], tag + " _rgbs")
    R.criterion(leaf["features_dc"].grad, ref["d_features_dc"], tag + " dL/dfeatures_dc")
    R.criterion(leaf["features_rest"].grad, ref["d_features_rest"], tag + " dL/dfeatures_rest")
    K = (case["n"] + 1) ** 2
    assert bool((leaf["features_rest"].grad[:, K - 1:] == 0).all()), "rows the degree does not use take no gradient"
    _, dark = _run_nodes(case, False)
    assert float(leaf["means"].grad.abs().max()) > 0
    assert _same_bits(leaf["means"].grad, dark["means"].grad), "the colour sends nothing to the means (detached view directions)"
    assert bool((dark["features_dc"].grad == 0).all()) and bool((dark["features_rest"].grad == 0).all())


@pytest.mark.parametrize("deg", R.PRECOMPUTE_DEGREES)
def test_f_pre_compute_colors_with_a_gradient_to_xyz(deg):
    from emd_amd.model import pre_compute_colors
    case, ref = R.precompute_case(deg), R.precompute_reference(deg)
    shs, xyz = case["shs"].to(DEV).requires_grad_(True), case["xyz"].to(DEV).requires_grad_(True)
    colours = pre_compute_colors(shs, xyz, case["camera_center"], deg)
    (colours * case["g"].to(DEV)).sum().backward()
    tag = f"f: pre_compute_colors degree {deg}"
    R.criterion(colours, ref["colour"], tag + " colours")
    R.criterion(shs.grad, ref["d_coeffs"], tag + " dL/dshs")
    R.criterion(xyz.grad, ref["d_dirs"], tag + " dL/dxyz")
    assert bool((shs.grad[:, case["K"]:] == 0).all()), "rows the degree does not use take no gradient"
    if deg == 0:
        assert bool((xyz.grad == 0).all())
