"""-m gpu: the accumulator rows of the render backward at their 64-byte pitch (one aligned line per Gaussian), the lane mapping of K7's flush
(16 lanes per row, four rows per atomic instruction), and the call without depth / alpha-image gradients against the same call fed zeros.

Reference: the CPU oracle's render backward (tests/helpers.compare_render_grads: GRAD_RTOL / GRAD_ATOL_FRAC / GRAD_REL_L2).  Two runs of the
same backward differ by the order of K7's float atomics only: their rows are compared under that same per-kernel bar, the first run as the
reference (outputs of the projection chain behind the rows: the end-to-end floor of tests/helpers.py).  Pad floats of a row are written by nobody: exact zeros."""
import ctypes as C

import numpy as np
import pytest
import torch

from emd_amd import GaussianRasterizationSettings, GaussianRasterizer
from emd_amd import _lib as L
from emd_amd import rasterizer as rz
from oracle import cpu_oracle as co
from tests.helpers import (END2END_ATOL_FRAC, END2END_REL_L2, assert_grad_close, compare_render_grads, hip_render_grads, make_case, run_hip, run_oracle, run_oracle_extra_sets)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pad_is_zero(call, num_extra):
    rows = call.render_grads
    pay = L.BWD_PAYLOAD + 4 * num_extra
    assert rows.shape[1] == L.bwd_stride(num_extra) and rows.is_contiguous() and rows.data_ptr() % 64 == 0
    assert int(torch.count_nonzero(rows[:, pay:])) == 0, "a pad float of an accumulator row was written"
    for k in range(num_extra):
        assert int(torch.count_nonzero(rows[:, L.BWD_PAYLOAD + 4 * k + 3])) == 0       # the unused fourth float of an extra set


# ---- rows against the oracle: 0, 1, 2 extra colour sets, both small image sizes --------------------------------------------------------

@pytest.mark.parametrize("H, W", [(64, 96), (272, 272)], ids=["64x96", "272x272"])
@pytest.mark.parametrize("n_extra", [0, 1, 2], ids=lambda v: f"extra{v}")
def test_rows_match_the_oracle_and_the_pad_stays_zero(n_extra, H, W):
    case = make_case(n=600, H=H, W=W, seed=300 + n_extra)
    g = torch.Generator().manual_seed(17 + n_extra)
    feats = [torch.rand(case["N"], 3, generator=g) for _ in range(n_extra)]
    dX = [torch.randn(3, H, W, generator=g).numpy() for _ in range(n_extra)]
    orc = run_oracle_extra_sets(case, feats, dX) if n_extra else run_oracle(case, backward=True)
    hip = run_hip(case, backward=True, colors_extra=feats or None, dL_dextra=dX or None)
    compare_render_grads(hip["render_grads"], orc["grads"]["render_grads"])
    for k, of in enumerate(orc.get("extra", [])):
        assert_grad_close(hip["render_grads"][f"rgb_extra{k}"], of["grads"]["render_grads"]["rgb"], f"render:rgb_extra{k}")
    assert np.abs(hip["render_grads"]["conic"]).max() > 0
    _pad_is_zero(hip["call"], n_extra)


# ---- the seams of the lane mapping: the deepest batch of a quadrant's walk holds 1, 31, 32, 33, 63 rows ----------------------------------

def _stack_case(n, seed=5):
    """n wide, faint Gaussians on the optical axis of a one-tile image: every one of them reaches every pixel of all four quadrants with
    alpha >= 1/255 and the transmittance never runs out, so every quadrant's walk is n entries long -- full batches of 64 and a deepest
    batch of n % 64 rows."""
    H = W = 16
    case = make_case(n=n, H=H, W=W, seed=seed, sh_degree=0)
    cam = case["cam"]
    V, c = cam.world_view_transform.float(), cam.camera_center.float()
    g = torch.Generator().manual_seed(seed)
    z = 2.0 + 2.0 * (torch.randperm(n, generator=g).float() + 0.5) / n                     # distinct depths in (2, 4)
    off = 0.02 * (torch.rand(n, 2, generator=g) - 0.5) * z[:, None]
    case["means3D"] = (c[None] + z[:, None] * V[:3, 2][None] + off[:, :1] * V[:3, 0][None] + off[:, 1:] * V[:3, 1][None]).contiguous()
    case["scales"] = (z[:, None] * (0.9 + 0.3 * torch.rand(n, 3, generator=g))).contiguous()    # sigma ~ 17 px z / z: far wider than the tile
    case["rotations"] = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1)
    case["opacities"] = (0.012 + 0.006 * torch.rand(n, 1, generator=g)).contiguous()
    case["shs"] = torch.rand(n, 1, 3, generator=g)
    return case


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64 + 1, 64 + 31, 64 + 32, 64 + 33, 64 + 63])
def test_last_flush_batch_of_every_seam_size(n):
    case = _stack_case(n)
    orc = run_oracle(case, backward=True)
    # the construction holds on the reference: one tile with n entries, every pixel still open behind the last of them
    assert orc["bin"]["ranges"].reshape(-1, 2).tolist() == [[0, n]]
    assert float(orc["img"]["alpha"].max()) < 0.95 and float(orc["img"]["alpha"].min()) > 1.0 / 255.0 * min(n, 3)
    hip = run_hip(case, backward=True)
    compare_render_grads(hip["render_grads"], orc["grads"]["render_grads"])
    r = hip["call"].render_grads
    assert int((r[:, 3] != 0).sum()) == n                       # every Gaussian's row arrived (d/d opacity of a contributor)
    _pad_is_zero(hip["call"], 0)


# ---- the clean-workspace protocol over the whole pitch -----------------------------------------------------------------------------------

def _leaves(case):
    d = lambda t: t.to(DEV).clone().requires_grad_(True)
    return dict(means3D=d(case["means3D"]), shs=d(case["shs"]), opacities=d(case["opacities"]), scales=d(case["scales"]), rotations=d(case["rotations"]))


def _settings(case):
    cam = case["cam"]
    return GaussianRasterizationSettings(case["H"], case["W"], cam.tanfovx, cam.tanfovy, case["bg"].to(DEV), 1.0, cam.world_view_transform.to(DEV),
                                         cam.full_proj_transform.to(DEV), case["sh_degree"], cam.camera_center.to(DEV), False, True)


def _backward(case, loss, extras=None, **opts):
    """One forward + backward; loss(color, depth, alpha, extra images) -> scalar.  -> (input gradients, the call's record)"""
    t = _leaves(case)
    r = GaussianRasterizer(_settings(case), compute_normal=False, **opts)
    m2 = torch.zeros(case["N"], 3, device=DEV, requires_grad=True)
    color, depth, _normal, alpha, _radii, extra = r(means2D=m2, colors_precomp=None, cov3Ds_precomp=None, colors_extra=extras, **t)
    loss(color, depth, alpha, extra).backward()
    return {k: v.grad.detach().cpu().numpy() for k, v in t.items()}, r.last_call


@pytest.mark.parametrize("n_extra", [0, 2], ids=lambda v: f"extra{v}")
def test_clean_workspace_is_all_zero_afterwards_and_a_second_backward_reproduces_the_first(n_extra):
    case = make_case(n=600, H=64, W=96, seed=41)
    gen = torch.Generator().manual_seed(4)
    G = torch.randn(3, 64, 96, generator=gen).to(DEV)
    feats = [torch.rand(case["N"], 3, generator=gen).to(DEV) for _ in range(n_extra)]
    GX = [torch.randn(3, 64, 96, generator=gen).to(DEV) for _ in range(n_extra)]
    loss = lambda color, depth, alpha, extra: (color * G).sum() + sum((e * g).sum() for e, g in zip(extra or [], GX))
    rz._clean_ws.clear()
    runs = []
    for _ in range(2):
        grads, _call = _backward(case, loss, extras=feats or None)
        runs.append(grads)
        assert len(rz._clean_ws) == 1
        (key, ws), = rz._clean_ws.items()
        assert ws.numel() == case["N"] * L.bwd_stride(n_extra) and ws.data_ptr() % 64 == 0
        assert int(torch.count_nonzero(ws)) == 0, "the workspace (pad included) is not all zero after the backward"
    for k in runs[0]:
        assert np.abs(runs[0][k]).max() > 0, k
        # (the projection chain conic -> covariance -> mean / scale / rotation amplifies the atomic-order differences of the rows: its outputs
        #  take the end-to-end floor of tests/helpers.py, the others the strict bar)
        loose = k in ("means3D", "scales", "rotations")
        assert_grad_close(runs[1][k], runs[0][k], "second backward:" + k, atol_frac=END2END_ATOL_FRAC if loose else None,
                          rel_l2=END2END_REL_L2 if loose else None)


# ---- no depth / alpha-image gradient (null pointers) ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_extra", [0, 1], ids=lambda v: f"extra{v}")
@pytest.mark.parametrize("absgrad", [False, True], ids=["noabs", "absgrad"])
def test_null_depth_and_alpha_gradients_equal_explicit_zero_images(absgrad, n_extra):
    case = make_case(n=600, H=64, W=96, seed=43)
    gen = torch.Generator().manual_seed(6)
    G = torch.randn(3, 64, 96, generator=gen).to(DEV)
    feats = [torch.rand(case["N"], 3, generator=gen).to(DEV) for _ in range(n_extra)]
    GX = [torch.randn(3, 64, 96, generator=gen).to(DEV) for _ in range(n_extra)]
    base = lambda color, extra: (color * G).sum() + sum((e * g).sum() for e, g in zip(extra or [], GX))
    # neither gradient arrives (set_materialize_grads(False): null pointers) / both arrive as explicit zero images
    _, none = _backward(case, lambda c, d, a, x: base(c, x), extras=feats or None, keep_render_grads=True, absgrad=absgrad)
    _, zero = _backward(case, lambda c, d, a, x: base(c, x) + (d * 0.0).sum() + (a * 0.0).sum(), extras=feats or None, keep_render_grads=True,
                        absgrad=absgrad)
    got, ref = hip_render_grads(none, 96, 64), hip_render_grads(zero, 96, 64)
    names = ["mean2D", "conic", "opacity", "rgb"] + (["abs"] if absgrad else []) + [f"rgb_extra{k}" for k in range(n_extra)]
    for k in names:
        assert np.abs(ref[k]).max() > 0, k
        assert_grad_close(got[k], ref[k], "no-depth:" + k)
    assert int(torch.count_nonzero(none.render_grads[:, 2])) == 0          # float 2 (d/d depth) is never added
    _pad_is_zero(none, n_extra)
    _pad_is_zero(zero, n_extra)


def test_null_depth_and_alpha_gradients_against_the_oracle():
    """The same call against the CPU oracle with zero depth / alpha gradients (the oracle's depth row is then zero as well)."""
    case = make_case(n=600, H=64, W=96, seed=44)
    case["dL_ddepth"] = np.zeros_like(case["dL_ddepth"])
    case["dL_dalpha"] = np.zeros_like(case["dL_dalpha"])
    orc = run_oracle(case, backward=True)
    G = torch.from_numpy(case["dL_dcolor"]).to(DEV)
    _, call = _backward(dict(case, flags=case["flags"] & ~co.F_NORMAL), lambda c, d, a, x: (c * G).sum(), keep_render_grads=True)
    compare_render_grads(hip_render_grads(call, 96, 64), orc["grads"]["render_grads"])


# ---- the camera gradient reads the rows through the pitch ----------------------------------------------------------------------------------

def test_camera_gradient_on_kept_rows():
    """emd_raster_backward_camera on the kept rows of a finished call against tests/camera_grad_ref.py (the bar and the case of
    tests/test_camera_grad_gpu.py), and the rows are left as they were."""
    from tests import camera_grad_ref as R
    from tests import test_camera_grad_gpu as T
    rf, hip = T._reference("static-sh"), T._hip("static-sh")
    ref, N = rf["ref"], rf["case"]["N"]
    call = hip["call"]
    assert call.render_grads.shape == (N, L.bwd_stride(0))
    rows = ref.rows(hip["rows"])
    want, terms = ref.camera35_from_rows(rows), ref.terms(rows)
    outs = {}
    b = T._bwd_args(hip, rf["case"], rf["raw"], outs)
    b.flags = call.flags
    rows0 = call.render_grads.clone()
    ws_bytes = L.camera_grad_workspace_size(N)
    ws = torch.empty(ws_bytes // 4, device=DEV)
    out = torch.full((35,), float("nan"), device=DEV)
    L.check(L.load().emd_raster_backward_camera(C.byref(b), out.data_ptr(), ws.data_ptr(), ws_bytes, L.stream()), "camera")
    torch.cuda.synchronize()
    assert torch.equal(call.render_grads, rows0)
    assert T._ratio(out.cpu().numpy().astype(np.float64), want, R.bound35(want, terms), "kept rows at the 64-byte pitch") <= 1.0
