"""-m gpu: the deterministic stand-alone motion backward (transform_gaussians(..., deterministic=True), emd_motion_backward_det; DESIGN.md section
8.10).  dL/dactor_pose is the pinned sum (tests/segsum_checks.py) of the call's own [n, 12] rows in ascending point index, bit for bit; the
per-point outputs are the default entry's; all gradients have identical bits from run to run, on another stream and in a hipGraph replay; and the
values stay inside the existing bars of tests/test_motion_sh_gpu.py, tests/test_nodes_gpu.py and tests/helpers.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from emd_amd import _lib as L
from emd_amd import motion
from oracle import torch_ref as tr
from tests import det_list_checks as dl
from tests import test_motion_sh_gpu as base
from tests import test_nodes_gpu as nodes_base
from tests.helpers import GRAD_RTOL, POSE_TERM_RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _refuse(name):
    def f(*a, **k):
        raise AssertionError(f"{name} must not be called here")
    return f


@functools.lru_cache(maxsize=None)
def _case(n, sizes, seed=0):
    """n points of which sizes[a] are bound to actor a, interleaved with the static ones (actor_id -1) by a random permutation; residuals on.
    -> dict of float32 / int32 numpy arrays, never modified."""
    rng = np.random.default_rng(seed)
    A = len(sizes)
    ids = np.full(n, -1, np.int32)
    ids[:sum(sizes)] = np.repeat(np.arange(A, dtype=np.int32), sizes)
    ids = ids[rng.permutation(n)]
    pose = rng.standard_normal((A, 12)).astype(np.float32)
    pose[:, 0:4] /= np.linalg.norm(pose[:, 0:4], axis=1, keepdims=True)
    pose[:, 8:12] /= np.linalg.norm(pose[:, 8:12], axis=1, keepdims=True)
    pose[:, 7] = 1.0
    if A > 2:
        pose[2, 7] = 0.0                                         # an actor that is not visible in this frame
    f = lambda *shape, s=1.0: (s * rng.standard_normal(shape)).astype(np.float32)
    return dict(n=n, A=A, ids=ids, pose=pose, means=f(n, 3), quats=f(n, 4), opac=rng.random(n).astype(np.float32), rdx=f(n, 3, s=0.05),
                rdq=f(n, 4, s=0.05), g_wm=f(n, 3), g_wq=f(n, 4), g_wo=f(n))


def _call(case, det, want_pose=True):
    """emd_motion_backward_det (det) or emd_motion_backward through ctypes with the test's own workspace -> dict of numpy outputs, ws, lay."""
    lib = L.load()
    n, A = case["n"], case["A"]
    t = {k: torch.from_numpy(v).to(DEV) for k, v in case.items() if isinstance(v, np.ndarray)}
    m = L.EmdMotion(t["ids"].data_ptr(), t["pose"].data_ptr(), A, t["rdx"].data_ptr(), t["rdq"].data_ptr())
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    out = dict(d_means=nan(n, 3), d_quats=nan(n, 4), d_opac=nan(n), d_pose=nan(A, 12) if want_pose else None, d_rdx=nan(n, 3), d_rdq=nan(n, 4))
    args = [n, t["means"].data_ptr(), t["quats"].data_ptr(), t["opac"].data_ptr(), C.byref(m), t["g_wm"].data_ptr(), t["g_wq"].data_ptr(),
            t["g_wo"].data_ptr(), out["d_means"].data_ptr(), out["d_quats"].data_ptr(), out["d_opac"].data_ptr(), L.ptr(out["d_pose"]),
            out["d_rdx"].data_ptr(), out["d_rdq"].data_ptr()]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = lay = None
    if det:
        if want_pose:
            ws = torch.empty(L.motion_det_workspace_size(n), dtype=torch.uint8, device=DEV)
            ws.fill_(0xA5)                                       # never cleared by the call, and need not be
        lay = L.motion_det_layout(n, A)
        L.check(lib.emd_motion_backward_det(*args, L.ptr(ws), 0 if ws is None else ws.numel(), st), "emd_motion_backward_det")
    else:
        L.check(lib.emd_motion_backward(*args, st), "emd_motion_backward")
    torch.cuda.synchronize()
    res = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    res.update(ws=ws, lay=lay)
    return res


def _check_call(case):
    got, default = _call(case, det=True), _call(case, det=False)
    n, A = case["n"], case["A"]
    lengths, raw, keys, slots = dl.check_lists(got["ws"], got["lay"], n, L.ACTOR_STRIDE, L.ACTOR_STRIDE, got["d_pose"], A)
    assert np.array_equal(raw.view(np.int32), np.where(case["ids"] >= 0, case["ids"], -1))          # the destination of row i is the actor of point i
    assert np.array_equal(np.bincount(keys, minlength=A), np.bincount(case["ids"][case["ids"] >= 0], minlength=A))
    for q in ("d_means", "d_quats", "d_opac", "d_rdx", "d_rdq"):                                    # per point: the default entry's bits
        assert np.array_equal(got[q].view(np.uint32), default[q].view(np.uint32)), q
    # the default entry adds the same rows with float atomics: the condition-aware pose bar of tests/helpers.py, the terms being the rows themselves
    rows = dl.read_workspace(got["ws"], got["lay"], n, L.ACTOR_STRIDE)[0]
    terms = np.zeros((A, 12))
    bound = case["ids"] >= 0
    np.add.at(terms, case["ids"][bound], np.abs(rows[bound].astype(np.float64)))
    limit = GRAD_RTOL * np.abs(got["d_pose"]) + POSE_TERM_RTOL * terms + 1e-12
    assert (np.abs(default["d_pose"].astype(np.float64) - got["d_pose"]) <= limit).all()
    return got


def test_pose_gradient_is_the_pinned_sum_of_the_calls_own_rows():
    """4000 points, actors of 1500 (three chunks), 700 (two), 300 (one), 1 and 0 points, the rest static, all interleaved."""
    case = _case(4000, (1500, 700, 300, 1, 0))
    got = _check_call(case)
    assert (got["d_pose"][4].view(np.uint32) == 0).all()         # the empty actor: +0.0
    assert (np.abs(got["d_pose"][:4]).max(axis=1) > 0).all()
    ids = case["ids"]
    assert (ids < 0).sum() == 4000 - 2501 and all((np.diff(np.flatnonzero(ids == a)) > 1).any() for a in range(3))      # interleaved, not blocked by actor


def _reference(case):
    """oracle/torch_ref.motion_transform in float64 with autograd.  The pose table enters once per POINT (row i: the pose of point i's actor), so that
    its gradient is the per-point terms whose sum over an actor is that actor's pose gradient -> dict of float64 gradients, terms [A, 12]."""
    n, A = case["n"], case["A"]
    t = lambda k: torch.from_numpy(case[k]).double().requires_grad_(True)
    means, quats, opac, rdx, rdq = t("means"), t("quats"), t("opac"), t("rdx"), t("rdq")
    ids = torch.from_numpy(case["ids"]).long()
    per_point = torch.from_numpy(case["pose"]).double()[ids.clamp_min(0)].clone().requires_grad_(True)
    own = torch.where(ids >= 0, torch.arange(n), torch.full((n,), -1))
    wm, wq, wo = tr.motion_transform(means, quats, opac, own, per_point, rdx, rdq)
    g = lambda k: torch.from_numpy(case[k]).double()
    ((wm * g("g_wm")).sum() + (wq * g("g_wq")).sum() + (wo.reshape(-1) * g("g_wo")).sum()).backward()
    rows = per_point.grad.numpy() * (case["ids"] >= 0)[:, None]
    pose, terms = np.zeros((A, 12)), np.zeros((A, 12))
    bound = case["ids"] >= 0
    np.add.at(pose, case["ids"][bound], rows[bound])
    np.add.at(terms, case["ids"][bound], np.abs(rows[bound]))
    return dict(means=means.grad.numpy(), quats=quats.grad.numpy(), opac=opac.grad.numpy(), rdx=rdx.grad.numpy(), rdq=rdq.grad.numpy(), pose=pose), terms


def _through_python(case, deterministic=True):
    t = lambda k: torch.from_numpy(case[k]).to(DEV).requires_grad_(True)
    leaves = dict(means=t("means"), quats=t("quats"), opac=t("opac"), pose=t("pose"), rdx=t("rdx"), rdq=t("rdq"))
    ids = torch.from_numpy(case["ids"]).to(DEV)
    wm, wq, wo = motion.transform_gaussians(leaves["means"], leaves["quats"], leaves["opac"], ids, leaves["pose"], leaves["rdx"], leaves["rdq"],
                                            deterministic=deterministic)
    g = lambda k: torch.from_numpy(case[k]).to(DEV)
    ((wm * g("g_wm")).sum() + (wq * g("g_wq")).sum() + (wo * g("g_wo")).sum()).backward()
    return {k: v.grad for k, v in leaves.items()}, (wm, wq, wo)


def test_parity_mixed_static_and_residual(monkeypatch):
    """The inputs of test_hip_motion_mixed_static_and_residual_matches_oracle (5000 points, 7 actors, residuals on) through
    transform_gaussians(deterministic=True): the forward is that test's, bit for bit; the per-point gradients within the bar of
    test_hip_motion_backward_matches_reference against the float64 reference; the pose gradient within GRAD_RTOL |ref| + POSE_TERM_RTOL sum|terms|."""
    monkeypatch.setattr(L.load(), "emd_motion_backward", _refuse("emd_motion_backward"))
    from oracle import cpu_oracle as co
    rng = np.random.default_rng(0)
    n, A = 5000, 7
    f32 = lambda a: a.astype(np.float32)
    means, quats, opac = f32(rng.standard_normal((n, 3))), f32(rng.standard_normal((n, 4))), f32(rng.random(n))
    ids = rng.integers(-1, A, n).astype(np.int32)
    pose = f32(rng.standard_normal((A, 12)))
    pose[:, 0:4] /= np.linalg.norm(pose[:, 0:4], axis=1, keepdims=True)
    pose[:, 8:12] /= np.linalg.norm(pose[:, 8:12], axis=1, keepdims=True)
    pose[:, 7] = (rng.random(A) > 0.3)
    case = dict(n=n, A=A, ids=ids, pose=pose, means=means, quats=quats, opac=opac, rdx=f32(0.05 * rng.standard_normal((n, 3))),
                rdq=f32(0.05 * rng.standard_normal((n, 4))), g_wm=f32(rng.standard_normal((n, 3))), g_wq=f32(rng.standard_normal((n, 4))),
                g_wo=f32(rng.standard_normal(n)))
    got, (hm, hq, ho) = _through_python(case)
    wm, wq, wo = co.motion_forward(means, quats, opac, ids, pose, case["rdx"], case["rdq"])
    for h, w in ((hm, wm), (hq, wq), (ho, wo)):
        np.testing.assert_array_equal(h.detach().cpu().numpy().view(np.uint32), w.view(np.uint32))
    ref, terms = _reference(case)
    for k in ("means", "quats", "opac", "rdx", "rdq"):
        r = ref[k]
        assert np.abs(got[k].cpu().numpy() - r).max() <= 5e-5 * max(1.0, np.abs(r).max()), k
    limit = GRAD_RTOL * np.abs(ref["pose"]) + POSE_TERM_RTOL * terms + 1e-12
    worst = float((np.abs(got["pose"].cpu().numpy() - ref["pose"]) / limit).max())
    print(f"pose gradient: worst |got - ref| / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("tag", ["train", "train5"])
def test_parity_with_the_reference_golden(tag, monkeypatch):
    """test_hip_motion_backward_matches_reference as it stands (RigidNodes golden vectors, its bars), with the switch on."""
    monkeypatch.setattr(L.load(), "emd_motion_backward", _refuse("emd_motion_backward"))
    monkeypatch.setattr(motion, "transform_gaussians", functools.partial(motion.transform_gaussians, deterministic=True))
    base.test_hip_motion_backward_matches_reference(tag)


def test_identical_bits_across_runs_streams_and_graph_replay(monkeypatch):
    monkeypatch.setattr(L.load(), "emd_motion_backward", _refuse("emd_motion_backward"))
    case = _case(4000, (1500, 700, 300, 1, 0))
    t = lambda k, grad=True: torch.from_numpy(case[k]).to(DEV).requires_grad_(grad)
    leaves = [t("means"), t("quats"), t("opac"), t("pose"), t("rdx"), t("rdq")]
    ids, g_wm, g_wq, g_wo = t("ids", False), t("g_wm", False), t("g_wq", False), t("g_wo", False)

    def step():
        wm, wq, wo = motion.transform_gaussians(leaves[0], leaves[1], leaves[2], ids, leaves[3], leaves[4], leaves[5], deterministic=True)
        return torch.autograd.grad((wm * g_wm).sum() + (wq * g_wq).sum() + (wo * g_wo).sum(), leaves)
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    first = [g.clone() for g in step()]
    assert float(first[3].abs().max()) > 0
    assert same(first, step())
    busy = torch.randn(2048, 2048, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(8):
        busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        on_side = [g.clone() for g in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert same(first, on_side)
    with torch.cuda.stream(side):
        step()                                                   # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same(first, captured)


@pytest.mark.parametrize("n,sizes", [(1, (1,)), (1, (0,)), (255, (100, 60)), (513, (513,)), (513, (0, 0, 0)), (257, (60, 57, 55))])
def test_edges_of_the_chunk_and_the_block(n, sizes):
    """One point (bound / static), a ragged block, one run of a chunk and one element, every point static, and one workgroup and one lane with three
    actors and a third of the points static.  (_check_call: the per-point outputs are the default entry's, bit for bit -- both kernels include one
    text.  The last case is appended, so the earlier cases keep their ids.)"""
    got = _check_call(_case(n, sizes, seed=n))
    if sum(sizes) == 0:
        assert (got["d_pose"].view(np.uint32) == 0).all()


def test_without_a_pose_gradient_no_workspace_is_needed():
    case = _case(513, (300, 100), seed=5)
    got, default = _call(case, det=True, want_pose=False), _call(case, det=False, want_pose=False)
    assert got["ws"] is None
    for q in ("d_means", "d_quats", "d_opac", "d_rdx", "d_rdq"):
        assert np.isfinite(got[q]).all() and np.array_equal(got[q].view(np.uint32), default[q].view(np.uint32)), q


def test_through_rigid_gaussians(monkeypatch):
    """The inputs of tests/test_nodes_gpu.py through rigid_gaussians(deterministic=True): two runs give bit-identical gradients on every input, and the
    values stay inside that file's bars against the reference."""
    from emd_amd.motion import actor_pose_table
    from emd_amd.nodes import rigid_gaussians
    monkeypatch.setattr(L.load(), "emd_motion_backward", _refuse("emd_motion_backward"))
    dev = torch.device("cuda", 0)
    g = np.load(os.path.join(nodes_base.G, "or_nodes.npz"))
    runs = []
    for _ in range(2):
        d = nodes_base._inputs(g, "rigid_", dev)
        pose = actor_pose_table(d["instances_quats"], d["instances_trans"], d["instances_fv"], int(g["rigid_frame"]))
        gs = rigid_gaussians(d["means"], d["quats"], d["opacity_logits"], d["log_scales"], d["features_dc"], d["features_rest"], d["point_ids"][:, None],
                             pose, torch.from_numpy(g["camera_center"]).to(dev), sh_degree=3, step=int(g["rigid_step"]), deterministic=True)
        nodes_base._check(g, "rigid_", gs, d)
        runs.append({k: v.grad.clone() for k, v in d.items() if v.requires_grad and v.grad is not None})
    assert set(runs[0]) == set(runs[1]) and {"means", "quats", "instances_quats", "instances_trans"} <= set(runs[0])
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
