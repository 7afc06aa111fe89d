"""The dense dL/dshs of the one-call default backward is zeroed by the render backward's own workgroups (K7: a slice of the N x 12 float4 each,
csrc/common.h emd_fill_slice) and the projection backward (K8), behind it on the stream, stores the rows of the contributing Gaussians only
(PreBwdArgs.shs_prezeroed).  Every other form keeps the dense K8: the two-call backward, EMD_FLAG_DETERMINISTIC, the factored SH gradient, M != 16.

Every case applies three checks to a finished call (check_prefill):
  poison       every buffer the binding allocates for the call is filled with NaN first (torch.empty of emd_amd.rasterizer replaced for the length
               of the call): afterwards every gradient element is finite and inside the project's gradient bars against the CPU oracle
               (tests/helpers.compare_backward: 1e-4 |b| + 1e-6 max|b| element-wise, relative L2 <= 1e-5)
  exact zeros  a Gaussian with RasterCall.contributed == 0 has a dL/dshs row of 48 words 0x00000000, and +0 words in every other per-Gaussian gradient
  same set     the rows written non-zero belong to flagged Gaussians; the set itself obeys tests/test_contributing_set_gpu.check_invariant

The five small gradients (means3D, scales, rotations, opacities, means2D) are not part of the fill: they leave through K8's staging tile, zeros included.
Shapes: the smallest at which the fill or the predicate can go wrong (N <= 20 000, images <= 128 x 96)."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from emd_amd import rasterizer
from tests.helpers import (assert_grad_close, compare_backward, make_case, place_in_depth_band, raw_params_parity, run_hip, run_oracle,
                           run_oracle_extra_sets)
from tests.test_contributing_set_gpu import (_behind_the_camera, _grads, _leaves, _loss, _rasterizer, check_invariant, occluded_case,
                                             oracle_contributing)

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


class _PoisonedTorch:
    """`torch` as emd_amd.rasterizer sees it, with `empty` handing out NaN-filled floating-point tensors."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    def empty(self, *a, **kw):
        t = self._real.empty(*a, **kw)
        if t.is_floating_point() and t.is_cuda and t.numel():
            t.fill_(NAN)
        return t


@contextlib.contextmanager
def poisoned_buffers():
    real = rasterizer.torch
    rasterizer.torch = _PoisonedTorch(real)
    try:
        probe = rasterizer.torch.empty(3, device=DEV, dtype=torch.float32)
        assert bool(torch.isnan(probe).all())
        yield
    finally:
        rasterizer.torch = real


def per_gaussian(grads, N):
    """(name, [N, -] float32 array) of every per-Gaussian gradient of a call."""
    for k, v in grads.items():
        for j, x in enumerate(v if isinstance(v, list) else [v]):
            if x is None or k == "actor_pose":
                continue
            yield f"{k}[{j}]" if isinstance(v, list) else k, np.ascontiguousarray(np.asarray(x, np.float32)).reshape(N, -1)


def check_zero_rows(grads, c, N):
    """exact zeros + same set of the module docstring, on host arrays."""
    for k, x in per_gaussian(grads, N):
        assert np.isfinite(x).all(), f"grads[{k}]: a poisoned element was left unwritten"
        assert not x.view(np.uint32)[~c].any(), f"grads[{k}] of an unflagged Gaussian is not +0 bit for bit"
    if grads.get("shs") is not None:
        shs = np.asarray(grads["shs"]).reshape(N, -1)
        assert shs.shape[1] in (27, 48) and not (shs.any(1) & ~c).any()


def check_prefill(hip, orc, names=None):
    N = hip["call"].N
    compare_backward(hip, orc, names=names)
    c = check_invariant(hip, orc)
    check_zero_rows(hip["grads"], c, N)
    return c


def poisoned_run(case, **kw):
    with poisoned_buffers():
        return run_hip(case, backward=True, **kw)


def small_image_case(n, seed=0, **kw):
    """48 x 40: T = 9 tiles, so K7's grid is the padded minimum, most of its workgroups surplus ones that return before the walk."""
    return make_case(n=n, H=40, W=48, seed=seed, **kw)


@functools.lru_cache(maxsize=None)
def _three_class(motion):
    """3000 Gaussians at 64 x 96, the first 15 % behind the camera, an opaque near layer in front of the rest; with its oracle, built once, never modified."""
    case = occluded_case(n=3000, layer_div=30 if motion else 5, seed=21, motion=motion, residual=motion)
    _behind_the_camera(case, torch.arange(450))
    return case, run_oracle(case, backward=True)


def class_shares(orc):
    vis, oc = orc["pre"]["radii"] > 0, oracle_contributing(orc)
    n = float(len(vis))
    return (~vis).sum() / n, (vis & ~oc).sum() / n, (vis & oc).sum() / n


@pytest.mark.parametrize("motion", [False, True], ids=["static", "motion"])
def test_the_three_class_scenes_hold_a_tenth_of_each_class(motion):
    """The input condition of case 5, on the CPU oracle alone: culled, visible without a contribution, contributing -- at least 10 % of N each."""
    case, orc = _three_class(motion)
    shares = class_shares(orc)
    print(f"three classes ({'motion' if motion else 'static'}): culled {shares[0]:.3f}, visible without a contribution {shares[1]:.3f}, contributing {shares[2]:.3f}")
    assert min(shares) >= 0.10


# ---- 1: ragged slices ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1000, 5003, 20000])
def test_ragged_slices(n):
    case = small_image_case(n, seed=n % 97)
    orc = run_oracle(case, backward=True)
    c = check_prefill(poisoned_run(case), orc)
    assert 0 < c.sum() < n


# ---- 2: fewer than 64 float4 per workgroup -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [37, 1])
def test_few_rows_per_workgroup(n):
    """N = 37 at 128 x 96: 444 float4 over the grid's workgroups -- seven slices of 64 (the last ragged), every other one empty; and a single Gaussian."""
    case = make_case(n=n, H=96, W=128, seed=4)
    place_in_depth_band(case, torch.arange(0, n, 2), 2.0, 4.0, seed=4)          # every other one certainly visible
    orc = run_oracle(case, backward=True)
    assert oracle_contributing(orc).any()
    check_prefill(poisoned_run(case), orc)


# ---- 3: nothing visible --------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_nothing_visible():
    case = small_image_case(700, seed=3)
    _behind_the_camera(case, torch.arange(700))
    orc = run_oracle(case, backward=True)
    hip = poisoned_run(case)
    c = check_prefill(hip, orc)
    assert not (hip["radii"] > 0).any() and not c.any()
    assert not hip["grads"]["shs"].view(np.uint32).any()          # every row +0: the waves all left at wave_n == 0, after their slices


# ---- 4: an overflowed call -----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_overflowed_call():
    """capacity 16 against some thousand (tile, Gaussian) pairs, in no_sync mode (the forward does not retry): the overflow bit of the status is set, the
    ranges are empty, every K7 wave leaves at wave_n == 0 -- and every gradient is an exact zero, none left unwritten."""
    case = make_case(n=2000, H=40, W=56, seed=9)          # (an image size of its own: the binding's capacity cache is keyed by it)
    key = (torch.device(DEV).index or 0, case["H"], case["W"])
    rasterizer._capacity_hint.pop(key, None)
    try:
        with poisoned_buffers():
            t, r = _leaves(case), _rasterizer(case, keep_render_grads=True, no_sync=True, min_capacity=16, capacity_hint=16)
            out = r(**t)
            _loss(case, out).backward()
        call = r.last_call
        st = call.last_status()
        assert st["overflow"] & 1 and st["num_rendered"] > 16
        g = _grads(t)
        assert not call.contributed.cpu().numpy().any()
        for k, x in per_gaussian(g, case["N"]):
            assert not x.view(np.uint32).any(), f"grads[{k}] of an overflowed call is not all +0"
    finally:
        rasterizer._capacity_hint.pop(key, None)
        rasterizer._watch.pop(key, None)


# ---- 5: culled, visible without a contribution, contributing -- in one call ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("motion", [False, True], ids=["static", "motion"])
def test_three_classes_at_once(motion):
    case, orc = _three_class(motion)
    hip = poisoned_run(case)
    c = check_prefill(hip, orc)
    vis = hip["radii"] > 0
    got = ((~vis).mean(), (vis & ~c).mean(), c.mean())
    assert min(got) >= 0.10, got
    assert np.abs(hip["grads"]["shs"][c]).max() > 0
    if motion:
        assert np.abs(hip["grads"]["actor_pose"]).max() > 0


# ---- 6: instantiations ---------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_absgrad():
    case, orc = _three_class(False)
    hip = poisoned_run(case, absgrad=True)
    check_prefill(hip, orc)
    assert np.abs(hip["grads"]["means2D_abs"]).max() > 0


@gpu
@pytest.mark.parametrize("n_extra", [1, 2], ids=lambda v: f"extra{v}")
def test_extra_colour_sets(n_extra):
    case, _ = _three_class(False)
    g = torch.Generator().manual_seed(50 + n_extra)
    feats = [torch.rand(case["N"], 3, generator=g) for _ in range(n_extra)]
    dX = [torch.randn(3, case["H"], case["W"], generator=g).numpy() for _ in range(n_extra)]
    orc = run_oracle_extra_sets(case, feats, dX)
    hip = poisoned_run(case, colors_extra=feats, dL_dextra=dX)
    check_prefill(hip, orc, names=("means3D", "means2D", "shs", "opacities", "scales", "rotations"))
    for k, of in enumerate(orc["extra"]):
        assert_grad_close(hip["grads"]["colors_extra"][k], of["grads"]["colors"], f"colors_extra[{k}]")


@gpu
def test_normal_gradient():
    case = occluded_case(n=3000, seed=24, normal_loss=True)
    _behind_the_camera(case, torch.arange(450))
    assert case["dL_dnormal"] is not None
    check_prefill(poisoned_run(case), run_oracle(case, backward=True))


@gpu
def test_raw_parameters():
    case = occluded_case(seed=25)
    g = torch.Generator().manual_seed(7)
    log_s = torch.log(case["scales"])
    raw_q = case["rotations"] * (0.5 + torch.rand(case["N"], 1, generator=g))
    logit = torch.logit(case["opacities"].clamp(1e-4, 1 - 1e-4))
    with poisoned_buffers():
        res = raw_params_parity(case, log_s, raw_q, logit)          # (its own comparison against the oracle at the helpers' bars: a NaN fails it)
    assert res["V"] > 1000


@gpu
def test_nine_coefficients_keep_the_dense_path():
    """M != 16: K8 writes dL/dshs row by row itself, zero rows included; K7 must not have been told to fill (its slices are sized for 16 coefficients)."""
    case = occluded_case(n=3000, seed=26, sh_degree=2)
    case["shs"] = case["shs"][:, :9].contiguous()
    _behind_the_camera(case, torch.arange(450))
    hip = poisoned_run(case)
    assert hip["grads"]["shs"].shape == (3000, 9, 3)
    check_prefill(hip, run_oracle(case, backward=True))


@gpu
def test_factored_sh_gradient_has_no_dense_rows():
    case, orc = _three_class(False)
    hip = poisoned_run(case, factored_sh_grad=True)
    assert hip["grads"]["shs"] is None
    c = check_prefill(hip, orc)
    factor = hip["call"].sh_color_grad.cpu().numpy()
    assert np.isfinite(factor).all() and not factor.view(np.uint32)[~c].any()
    np.testing.assert_array_equal(factor, hip["call"].render_grads.cpu().numpy()[:, 7:10] * (orc["pre"]["clamped"] == 0))


@gpu
def test_deterministic_mode_keeps_the_dense_path():
    """EMD_FLAG_DETERMINISTIC: the deterministic K7 does not fill and K8 writes densely, by radii.  Two runs on poisoned buffers agree bit for bit and with
    the oracle.  (Bit-identity with the build before this change: checked once with both libraries side by side, profiles/backward_prefill_ab.txt.)"""
    case, orc = _three_class(True)
    a, b = poisoned_run(case, deterministic=True), poisoned_run(case, deterministic=True)
    compare_backward(a, orc)
    vis = a["radii"] > 0
    check_zero_rows(a["grads"], vis, case["N"])
    for k, v in a["grads"].items():
        if v is not None:
            np.testing.assert_array_equal(v.view(np.uint32), b["grads"][k].view(np.uint32), err_msg=k)


# ---- 7: the two-call form --------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_two_call_form_writes_densely():
    """Camera tensors that require grad make the binding issue EMD_FLAG_BWD_RENDER_ONLY, the camera gradient, EMD_FLAG_BWD_PROJECT_ONLY, with a dense
    dL_dshs: neither call runs both kernels, so K7 does not fill and K8 must write every row -- a wrongly set flag would leave the poison."""
    from tests.test_camera_grad_gpu import _run
    case, orc = _three_class(False)
    with poisoned_buffers():
        hip = _run(case)
    assert hip["call"].camera_grad is not None and bool(torch.isfinite(hip["call"].camera_grad).all())
    grads = {k: v.cpu().numpy() for k, v in hip["grads"].items()}
    c = hip["call"].contributed.cpu().numpy()
    assert c[oracle_contributing(orc)].all()
    check_zero_rows(grads, c, case["N"])
    assert_grad_close(grads["shs"], orc["grads"]["shs"], "shs")
    assert_grad_close(grads["means2D"], orc["grads"]["means2D"], "means2D")
    assert_grad_close(grads["opacities"], orc["grads"]["opacities"], "opacities")


# ---- 8: two backward passes on one forward -------------------------------------------------------------------------------------------------------------
@gpu
def test_two_backward_passes_on_one_forward():
    case, orc = _three_class(False)
    passes = []
    with poisoned_buffers():
        t, r = _leaves(case), _rasterizer(case, keep_render_grads=True)
        loss = _loss(case, r(**t))
        for rep in range(2):
            for v in t.values():
                v.grad = None
            loss.backward(retain_graph=(rep == 0))
            call = r.last_call
            passes.append((_grads(t), call.render_grads.cpu().numpy().copy(), call.contributed.cpu().numpy().copy()))
    (g0, rows0, c0), (g1, rows1, c1) = passes
    np.testing.assert_array_equal(c0, c1)
    assert c0[oracle_contributing(orc)].all()
    same_rows = np.array_equal(rows0.view(np.uint32), rows1.view(np.uint32))
    for g in (g0, g1):
        check_zero_rows(g, c0, case["N"])
        assert_grad_close(g["shs"], orc["grads"]["shs"], "shs")
    for k in g0:
        if same_rows:
            np.testing.assert_array_equal(g0[k].view(np.uint32), g1[k].view(np.uint32), err_msg=k)
        else:
            assert_grad_close(g1[k], g0[k], k, atol_frac=1e-4, rel_l2=1e-4)          # (the reorder level of K7's float atomics, as tests/test_contributing_set_gpu.py)


# ---- 9: inside a captured graph ----------------------------------------------------------------------------------------------------------------------------
@gpu
def test_replayed_from_a_captured_graph():
    """One forward + backward captured into a hipGraph (one stream: the fill adds no node, no fork) and replayed three times, every gradient buffer of
    the graph refilled with NaN between replays: each replay leaves the eager call's gradients, exact zero rows included."""
    case, orc = _three_class(False)
    eager = poisoned_run(case)
    c = check_prefill(eager, orc)
    D = eager["status"]["num_rendered"]
    t = _leaves(case)
    r = _rasterizer(case, no_sync=True, capacity_hint=int(1.3 * D) + 1024)

    G = [torch.from_numpy(case[k]).to(DEV) for k in ("dL_dcolor", "dL_ddepth", "dL_dalpha")]          # (no upload inside the capture)

    def body():
        for v in t.values():
            v.grad = None
        out = r(**t)
        ((out[0] * G[0]).sum() + (out[1] * G[1]).sum() + (out[3] * G[2]).sum()).backward()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        body()
    try:
        for rep in range(3):
            for v in t.values():
                v.grad.fill_(NAN)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            g = _grads(t)
            check_zero_rows(g, c, case["N"])
            for k in g:          # against the eager call: the reorder level of K7's float atomics, as tests/test_contributing_set_gpu.py
                assert_grad_close(g[k], eager["grads"][k], f"replay {rep}: {k}", atol_frac=1e-4, rel_l2=1e-4)
            for k in ("shs", "means2D", "opacities"):
                assert_grad_close(g[k], orc["grads"][k], f"replay {rep}: {k} against the oracle")
    finally:
        graph.reset()
