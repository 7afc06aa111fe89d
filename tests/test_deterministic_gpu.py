"""-m gpu: the deterministic backward (RasterOptions.deterministic, EMD_FLAG_DETERMINISTIC) through the product path.

  1. structure   the accumulator rows equal, BIT FOR BIT, the numpy restatement of the pinned association (tests/segsum_checks.py) applied to the
                 call's own contribution rows and sorted lists; keys non-decreasing, slots strictly ascending inside a run
  2. run to run  the same call on the default stream, on a side stream, and beside another rasterizer busy on a third stream: identical bits
  3. parity      against the CPU oracle at the bars of tests/helpers.py, unchanged; the forward equals the default call's bit for bit
  4. long runs   runs longer than EMD_SEG_CHUNK through the real path (frame-filling Gaussians; an actor with > 2 chunks of visible points)
  5. edges, 6. hipGraph replay, 7. refusals
No assertion is made about the default mode: that its gradients may differ from run to run is the premise, not a test."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from emd_amd import GaussianRasterizationSettings, GaussianRasterizer, rasterizer
from emd_amd import _lib as L
from oracle import cpu_oracle as co
from tests import segsum_checks as sg
from tests.helpers import (IMAGE_TOL, assert_grad_close, assert_pose_close, compare_backward, compare_forward, make_case, run_hip, run_oracle,
                           run_oracle_extra_sets)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH = L.SEG_CHUNK


def _det(case, **kw):
    return run_hip(case, backward=True, deterministic=True, **kw)


@contextlib.contextmanager
def _deterministic_by_default():
    """The process-wide default every GaussianRasterizer reads when it is built: for helpers that construct their own rasterizer."""
    old = rasterizer.RasterConfig.deterministic
    rasterizer.RasterConfig.deterministic = True
    try:
        yield
    finally:
        rasterizer.RasterConfig.deterministic = old


def _lists(call):
    """-> (keys, slots, contribution rows below the slots in use, counts) of a deterministic call, on the host."""
    st = call.det_state
    counts = st["counts"].cpu().numpy().view(np.uint32)
    used, kept = int(counts[0]), int(counts[1])
    assert kept <= used <= st["rows"].shape[0]
    keys = st["keys"][:kept].cpu().numpy().view(np.uint32)
    slots = st["slots"][:kept].cpu().numpy().view(np.uint32)
    return keys, slots, st["rows"][:max(used, 1)].cpu().numpy(), counts


def _check_structure(hip, width=12):
    """(1) of the module docstring on one call; -> (longest run, number of runs)."""
    call = hip["call"]
    keys, slots, rows, counts = _lists(call)
    assert counts[0] == 4 * hip["status"]["num_rendered"]
    if len(keys) == 0:
        assert not call.render_grads.cpu().numpy().any()
        return 0, 0
    assert (np.diff(keys.astype(np.int64)) >= 0).all(), "keys must be non-decreasing"
    same = keys[1:] == keys[:-1]
    assert (np.diff(slots.astype(np.int64))[same] > 0).all(), "slots must ascend strictly inside a run"
    assert slots.max() < counts[0] and keys.max() < call.N
    got = call.render_grads.cpu().numpy()
    want = np.zeros_like(got)                                    # rows without a run keep the zero fill
    sg.segsum_reference(keys, slots, rows, width, want)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg="accumulator rows vs the restatement on the call's own lists")
    start, length = sg.run_structure(keys)
    return int(length.max()), len(start)


def _same_bits(a, b, what):
    assert set(a["grads"]) == set(b["grads"])
    for k, v in a["grads"].items():
        w = b["grads"][k]
        if v is None:
            assert w is None, k
            continue
        for x, y in zip(v if isinstance(v, list) else [v], w if isinstance(w, list) else [w]):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"{what}: grads[{k}]")
    for k, v in a["render_grads"].items():
        np.testing.assert_array_equal(v.view(np.uint32), b["render_grads"][k].view(np.uint32), err_msg=f"{what}: render_grads[{k}]")
    for k in ("color", "depth", "alpha", "normal", "radii"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


# ---- 1. structure ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(n=3000, H=64, W=96, seed=0), dict(n=80000, H=96, W=128, seed=9, scale_mult=1.0)],
                         ids=["n3000", "deep-lists-n80000"])
def test_rows_are_the_pinned_sum_of_the_calls_own_lists(kw):
    hip = _det(make_case(**kw))
    longest, runs = _check_structure(hip)
    assert runs > 1000 and longest >= 4
    assert hip["call"].render_grads.abs().max() > 0


# ---- 2. run to run -----------------------------------------------------------------------------------------------------------------------------
def _busy(stream, rounds=6):
    """Another rasterizer's forward + backward passes enqueued on `stream` (never waited for here): work that shares the device meanwhile."""
    case = make_case(n=20000, H=128, W=192, seed=7, scale_mult=1.5)
    cam = case["cam"]
    with torch.cuda.stream(stream):
        rs = GaussianRasterizationSettings(case["H"], case["W"], cam.tanfovx, cam.tanfovy, case["bg"].to(DEV), 1.0, cam.world_view_transform.to(DEV),
                                           cam.full_proj_transform.to(DEV), 3, cam.camera_center.to(DEV), False, False)
        rast = GaussianRasterizer(rs, no_sync=True, capacity_hint=1 << 19)
        T = {k: case[k].to(DEV).requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        m2 = torch.zeros(case["N"], 3, device=DEV, requires_grad=True)
        g = torch.from_numpy(case["dL_dcolor"]).to(DEV)
        for _ in range(rounds):
            (rast(means2D=m2, **T)[0] * g).sum().backward()


@pytest.mark.parametrize("motion", [False, True], ids=["static", "motion-residual"])
def test_three_runs_give_identical_bits(motion):
    case = make_case(n=4000, H=64, W=96, seed=12, motion=motion, residual=motion)
    a = _det(case, absgrad=True)
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = _det(case, absgrad=True)
    torch.cuda.synchronize()
    _busy(other)
    c = _det(case, absgrad=True)
    torch.cuda.synchronize()
    assert np.abs(a["grads"]["means2D_abs"]).max() > 0 and np.abs(a["grads"]["means3D"]).max() > 0
    if motion:
        assert np.abs(a["grads"]["actor_pose"]).max() > 0
    _same_bits(a, b, "default stream vs side stream")
    _same_bits(a, c, "alone vs beside another rasterizer")
    _check_structure(a)


# ---- 3. parity with the oracle at today's bars -------------------------------------------------------------------------------------------------
def _forward_is_the_default_calls(case, hip, **kw):
    base = run_hip(case, backward=False, **kw)
    for k in ("color", "depth", "alpha", "normal", "radii", "keys", "ids", "ranges"):
        np.testing.assert_array_equal(hip[k], base[k], err_msg=f"forward output {k} with and without the flag")


@pytest.mark.parametrize("kw", [
    dict(n=3000, H=64, W=96, seed=0),                                   # static SH
    dict(n=4000, H=64, W=96, seed=12, motion=True, residual=True),      # motion + residual_dx + residual_dq, pose gradients
    dict(n=3000, H=64, W=96, seed=104, normal_loss=True),               # a loss on the normal image
    dict(n=3000, H=80, W=80, seed=5, colors_precomp=True, cov_precomp=True),
], ids=["static-sh", "motion-residual", "normal-loss", "colors-cov-precomp"])
def test_parity_with_the_oracle(kw):
    case = make_case(**kw)
    orc = run_oracle(case, backward=True)
    hip = _det(case)
    compare_forward(hip, orc, tol=IMAGE_TOL)
    checked = compare_backward(hip, orc)
    assert "means3D" in checked and "opacities" in checked
    if kw.get("motion"):
        assert {"actor_pose", "residual_dx", "residual_dq"} <= set(checked)
    if kw.get("colors_precomp"):
        assert {"colors", "cov3D"} <= set(checked)
    _forward_is_the_default_calls(case, hip)
    _check_structure(hip)


def test_parity_absgrad():
    case = make_case(n=3000, H=64, W=96, seed=21)
    orc = run_oracle(case, backward=True)
    hip = _det(case, absgrad=True)
    assert "means2D_abs" in compare_backward(hip, orc, names=("means2D", "means2D_abs"))
    assert np.abs(hip["grads"]["means2D_abs"]).max() > 0


@pytest.mark.parametrize("n_extra", [1, 2], ids=lambda v: f"extra{v}")
def test_parity_extra_colour_sets(n_extra):
    case = make_case(n=3000, H=64, W=96, seed=101 + n_extra)
    g = torch.Generator().manual_seed(7 + n_extra)
    feats = [torch.rand(case["N"], 3, generator=g) for _ in range(n_extra)]
    dX = [torch.randn(3, case["H"], case["W"], generator=g).numpy() for _ in range(n_extra)]
    orc = run_oracle_extra_sets(case, feats, dX)
    hip = _det(case, colors_extra=feats, dL_dextra=dX)
    compare_forward(hip, orc, tol=IMAGE_TOL)
    compare_backward(hip, orc, names=("means3D", "means2D", "shs", "opacities", "scales", "rotations"))
    for k, of in enumerate(orc["extra"]):
        np.testing.assert_array_equal(hip["extra"][k].view(np.uint32), of["img"]["color"].view(np.uint32))
        assert_grad_close(hip["render_grads"][f"rgb_extra{k}"], of["grads"]["render_grads"]["rgb"], f"render:rgb_extra{k}")
        assert_grad_close(hip["grads"]["colors_extra"][k], of["grads"]["colors"], f"colors_extra[{k}]")
    _check_structure(hip, width=12 + 4 * n_extra)


@pytest.mark.parametrize("motion", [False, True], ids=["static", "motion"])
def test_parity_raw_parameters(motion):
    from tests.helpers import raw_params_parity
    case = make_case(n=4000, H=64, W=96, seed=61, motion=motion)
    g = torch.Generator().manual_seed(5)
    log_s = torch.log(case["scales"])
    raw_q = case["rotations"] * (0.5 + torch.rand(case["N"], 1, generator=g))
    logit = torch.logit(case["opacities"].clamp(1e-4, 1 - 1e-4))
    with _deterministic_by_default():
        raw_params_parity(case, log_s, raw_q, logit)


# ---- 4. long runs through the real path ----------------------------------------------------------------------------------------------------------
def test_frame_filling_gaussians_make_runs_longer_than_a_chunk():
    """256 x 256 = 256 tiles = 1024 quadrants: a faint Gaussian that covers the frame owns one contribution row in most of them."""
    case = make_case(n=2003, H=256, W=256, seed=33, scale_mult=1.0)
    case["means3D"][-3:] = torch.tensor([[0.30, 0.0, 1.0], [0.32, 0.02, 1.01], [0.34, -0.02, 0.99]])      # in front of everything else
    case["scales"][-3:] = 0.5
    case["opacities"][-3:] = 0.03
    orc = run_oracle(case, backward=True)
    hip = _det(case)
    longest, _ = _check_structure(hip)
    assert longest > CH, f"the longest run has {longest} rows: the case does not reach a second chunk"
    compare_forward(hip, orc, tol=IMAGE_TOL)
    compare_backward(hip, orc)


def test_actor_with_more_than_two_chunks_of_visible_points():
    """actor 0: > 2 EMD_SEG_CHUNK visible points, actor 1: three points, actor 2: none visible (gradient exactly 0), actor 3: no point at all."""
    case = make_case(n=6000, H=64, W=96, seed=14, motion=True, residual=True, actors=4)
    ids = torch.full((case["N"],), -1, dtype=torch.int32)
    n_dyn = case["N"] // 2
    ids[:n_dyn] = 0
    ids[100:103] = 1
    ids[200:260] = 2
    case["actor_ids"] = ids
    pose = case["actor_pose"].clone()
    pose[:, 7] = 1.0
    pose[2, 4] = -40.0                              # actor 2 is behind the camera (the camera looks along +x)
    pose[0, 4:7] = torch.tensor([8.0, 0.0, 1.2])
    pose[1, 4:7] = torch.tensor([7.0, 0.5, 1.2])
    case["actor_pose"] = pose
    orc = run_oracle(case, backward=True)
    vis = orc["pre"]["radii"] > 0
    counts = [int((vis & (ids.numpy() == a)).sum()) for a in range(4)]
    assert counts[0] > 2 * CH and counts[1] == 3 and counts[2] == 0 and counts[3] == 0, counts
    hip = _det(case)
    st = hip["call"].det_state
    kept = int(st["counts"].cpu().numpy().view(np.uint32)[2])
    assert kept == counts[0] + counts[1]
    pk = st["pose_keys"][:kept].cpu().numpy()
    pp = st["pose_points"][:kept].cpu().numpy()
    assert (np.diff(pk) >= 0).all() and (np.diff(pp)[pk[1:] == pk[:-1]] > 0).all()
    want = np.zeros((4, 12), np.float32)
    sg.segsum_reference(pk, pp, st["pose_rows"].cpu().numpy(), 12, want)
    got = hip["grads"]["actor_pose"]
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg="actor_pose vs the restatement on the call's own pose rows")
    assert not got[2].any() and not got[3].any() and np.abs(got[0]).max() > 0 and np.abs(got[1]).max() > 0
    assert_pose_close(got, orc["grads"]["actor_pose"], orc["grads"], orc["scene"])
    compare_forward(hip, orc, tol=IMAGE_TOL)
    assert "actor_pose" in compare_backward(hip, orc)
    again = _det(case)
    _same_bits(hip, again, "second run")


# ---- 5. edges ----------------------------------------------------------------------------------------------------------------------------------
def test_nothing_visible_and_a_single_gaussian():
    case = make_case(n=500, H=48, W=64, seed=31)
    case["means3D"][:, 0] = -5.0
    hip = _det(case)
    assert np.all(hip["radii"] == 0) and _check_structure(hip) == (0, 0)
    for k, v in hip["grads"].items():
        if v is not None:
            assert np.all(v == 0), k
    one = make_case(n=1, H=48, W=64, seed=32)
    one["means3D"][:] = torch.tensor([3.0, 0.0, 1.0])
    one["scales"][:] = 0.3
    orc = run_oracle(one, backward=True)
    hip = _det(one)
    assert hip["radii"][0] > 0
    compare_forward(hip, orc)
    compare_backward(hip, orc)
    assert _check_structure(hip)[1] == 1


def test_gaussian_with_list_entries_but_no_survivor():
    """An opaque wall in front: the Gaussians behind it are in the tile lists, and in no quadrant's walked survivor list -- no run, zero rows."""
    case = make_case(n=3000, H=64, W=96, seed=35)
    case["means3D"][-3:] = torch.tensor([[0.50, 0.0, 1.0], [0.55, 0.0, 1.0], [0.60, 0.0, 1.0]])      # alpha is capped at 0.99: three walls saturate a pixel
    case["scales"][-3:] = 3.0
    case["opacities"][-3:] = 0.9999
    orc = run_oracle(case, backward=True)
    hip = _det(case)
    keys = _lists(hip["call"])[0]
    listed = np.unique(hip["ids"])
    hidden = np.setdiff1d(listed, np.unique(keys))
    assert len(hidden) > 0, "every listed Gaussian has a contribution: the case shows nothing"
    assert not hip["call"].render_grads.cpu().numpy()[hidden].any()
    _check_structure(hip)
    compare_forward(hip, orc, tol=IMAGE_TOL)
    compare_backward(hip, orc)


def test_no_sync_overflow_retry_and_factored_sh():
    case = make_case(n=6000, H=96, W=128, seed=41)
    ref = _det(case)
    _same_bits(ref, _det(case, no_sync=True, capacity_hint=1 << 18), "no_sync")
    # a capacity overflow healed by the retry: the backward's workspace is sized by the capacity the retry ended with
    rasterizer._capacity_hint.clear()
    old = rasterizer.RasterConfig.min_capacity
    rasterizer.RasterConfig.min_capacity = 16
    try:
        rasterizer._capacity_hint[(0, 96, 128)] = 16
        healed = _det(case)
    finally:
        rasterizer.RasterConfig.min_capacity = old
    assert healed["call"].capacity == int(healed["status"]["num_rendered"] * 1.25) + 1024 != ref["call"].capacity      # (the regrown capacity)
    _same_bits(ref, healed, "after an overflow retry")
    _check_structure(healed)
    fac = _det(case, factored_sh_grad=True)
    assert fac["grads"]["shs"] is None
    f1 = fac["call"].sh_color_grad.cpu().numpy()
    f2 = _det(case, factored_sh_grad=True)["call"].sh_color_grad.cpu().numpy()
    np.testing.assert_array_equal(f1.view(np.uint32), f2.view(np.uint32))
    np.testing.assert_array_equal(fac["grads"]["means3D"].view(np.uint32), ref["grads"]["means3D"].view(np.uint32))
    assert np.abs(f1).max() > 0


def test_camera_tensor_that_requires_grad():
    """The two-call form (render half -> camera kernel -> projection half) with the workspace on both halves: viewmatrix.grad inside the bound of
    tests/test_camera_grad_gpu.py, and identical across two runs -- as is everything else the call returns."""
    from tests import test_camera_grad_gpu as tc
    rf = tc._reference("motion-residual")
    with _deterministic_by_default():
        a = tc._run(rf["case"], rf["raw"])
        b = tc._run(rf["case"], rf["raw"])
    assert a["call"].det_state is not None
    assert tc._ratio(a["cam35"], rf["e2e"], tc.R.bound35(rf["e2e"], rf["e2e_terms"]), "deterministic, end to end") <= 1.0
    np.testing.assert_array_equal(a["cam35"], b["cam35"])
    assert torch.equal(a["call"].render_grads, b["call"].render_grads)
    assert set(a["grads"]) == set(b["grads"]) and "actor_pose" in a["grads"]
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


# ---- 6. hipGraph -------------------------------------------------------------------------------------------------------------------------------
def test_captured_step_replays_to_the_eager_bits():
    case = make_case(n=4000, H=64, W=96, seed=12, motion=True, residual=True)
    cam = case["cam"]
    d = lambda t: t.to(DEV).clone().requires_grad_(t.is_floating_point())
    rs = GaussianRasterizationSettings(case["H"], case["W"], cam.tanfovx, cam.tanfovy, case["bg"].to(DEV), 1.0, cam.world_view_transform.to(DEV),
                                       cam.full_proj_transform.to(DEV), 3, cam.camera_center.to(DEV), False, False)
    names = ("means3D", "shs", "opacities", "scales", "rotations", "actor_pose", "residual_dx", "residual_dq")
    T = {k: d(case[k]) for k in names}
    ids = case["actor_ids"].to(DEV)
    m2 = torch.zeros(case["N"], 3, device=DEV, requires_grad=True)
    gC, gD = torch.from_numpy(case["dL_dcolor"]).to(DEV), torch.from_numpy(case["dL_ddepth"]).to(DEV)
    rast = GaussianRasterizer(rs, no_sync=True, capacity_hint=1 << 17, deterministic=True, aux_stream=False, absgrad=True)

    def step():
        color, depth = rast(means2D=m2, actor_ids=ids, **T)[:2]
        grads = torch.autograd.grad((color * gC).sum() + (depth * gD).sum(), [T[k] for k in names])
        return list(grads) + [rast.last_call.absgrad]
    eager = [g.clone() for g in step()]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            captured = step()
    torch.cuda.current_stream().wait_stream(s)
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append([g.clone() for g in captured])
    assert all(g.abs().max() > 0 for g in eager)
    for k, e, r0, r1 in zip(names + ("absgrad",), eager, *replays):
        assert torch.equal(r0, r1), f"two replays differ in {k}"
        assert torch.equal(r0, e), f"replay differs from the eager deterministic step in {k}"


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_flag_without_workspace_and_with_pair_stats():
    from tests import test_camera_grad_gpu as tc
    case = make_case(**tc.R.N_CASE, seed=0)
    hip = tc._run(case, camera=False)
    outs = {}
    b = tc._bwd_args(hip, case, None, outs)
    lib = L.load()
    b.flags = hip["call"].flags | L.FLAG_DETERMINISTIC
    assert lib.emd_raster_backward(C.byref(b), L.stream()) == L.EMD_ERR_WORKSPACE
    assert b"det_ws" in lib.emd_last_error() and b"emd_raster_det_workspace_size" in lib.emd_last_error()
    need = L.det_workspace_size(case["N"], hip["call"].capacity, 0)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    b.det_ws, b.det_bytes = ws.data_ptr(), need - 1
    assert lib.emd_raster_backward(C.byref(b), L.stream()) == L.EMD_ERR_WORKSPACE
    stats = torch.zeros(4, device=DEV, dtype=torch.int64)
    b.det_bytes, b.pair_stats = need, stats.data_ptr()
    assert lib.emd_raster_backward(C.byref(b), L.stream()) == L.EMD_ERR_INVALID
    assert b"pair_stats" in lib.emd_last_error()
    torch.cuda.synchronize()
    assert not stats.any()
    # ... and with the workspace the same arguments go through
    b.pair_stats = None
    color = hip["outs"][0]
    gC = torch.from_numpy(case["dL_dcolor"]).to(DEV)
    b.dL_dcolor = gC.data_ptr()
    assert lib.emd_raster_backward(C.byref(b), L.stream()) == 0, lib.emd_last_error()
    torch.cuda.synchronize()
    assert outs["means3D"].abs().max() > 0 and color.abs().max() > 0
