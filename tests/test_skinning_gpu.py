"""-m gpu: linear-blend skinning of SMPL pedestrian nodes (emd_amd.smpl / nodes.smpl_gaussians, csrc/skinning.hip) against the fp64 restatement
of the contract (tests/skinning_ref.py) under the criterion of DESIGN.md section 5 -- element-wise 1e-4 |ref| + 1e-6 max |ref|, relative L2 1e-5.

Shapes: 5 instances of 1, 70, 300, 0 and 129 points (less than a wave, more than a wave, more than one chunk, empty, one past a wave
multiple), once sorted and once shuffled with 17 unbound rows interleaved; three parent tables (SMPL, a path of depth 23, a star); with and
without canon_inv; one invalid instance.  Points within 1e-3 of a branch boundary of matrix_to_quaternion (at most 1 %, asserted) are left out
of the quaternion comparisons and get no upstream quaternion gradient."""
import functools

import pytest
import torch

from tests import skinning_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TABLES = {"smpl": R.SMPL_PARENTS, "path": R.PATH_PARENTS, "star": R.STAR_PARENTS}
GRADS = ("d_theta", "d_weights", "d_means", "d_quats", "d_opacities", "d_trans")


@functools.lru_cache(maxsize=None)
def _case(table, canon, shuffled):
    """The case and its fp64 reference, computed once and shared (nothing below writes into them)."""
    c = R.make_case(TABLES[table], canon=canon, shuffled=shuffled)
    ref = R.reference(c)
    assert int(ref["tie"].sum()) <= 0.01 * sum(R.COUNTS)
    assert int(ref["branch_counts"].min()) > 0
    return c, ref


def _run(c, g_wq, fused=False, layout=None):
    """Forward + backward on the device -> dict of outputs and gradients (device tensors)."""
    from emd_amd import smpl
    d = lambda k: c[k].to(DEV).clone().requires_grad_(True)
    theta, means, quats, opac, weights, trans = d("theta"), d("means"), d("quats"), d("opacities"), d("weights"), d("trans")
    ids, joints, valid = c["ids"].to(DEV), c["joints"].to(DEV), c["valid"].to(DEV)
    canon = None if c["canon_inv"] is None else c["canon_inv"].to(DEV)
    out = {}
    if fused:
        wm, wq, wo = smpl.posed_skin_gaussians(means, quats, opac, ids, weights, theta, joints, trans, valid, c["parents"], canon, layout=layout)
    else:
        A = smpl.joint_transforms(theta, joints, c["parents"], canon)
        A.retain_grad()
        wm, wq, wo = smpl.skin_gaussians(means, quats, opac, ids, weights, A, trans, valid, layout=layout)
        out["A"] = A
    ((wm * c["g_wm"].to(DEV)).sum() + (wq * g_wq.float().to(DEV)).sum() + (wo * c["g_wo"].to(DEV)).sum()).backward()
    out.update(wm=wm, wq=wq, wo=wo, d_theta=theta.grad, d_weights=weights.grad, d_means=means.grad, d_quats=quats.grad, d_opacities=opac.grad,
               d_trans=trans.grad)
    if not fused:
        out["d_A"] = A.grad
    return {k: v.detach() for k, v in out.items()}


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("canon", [False, True], ids=["plain", "canon"])
@pytest.mark.parametrize("table", list(TABLES))
def test_values_and_gradients_match_the_fp64_contract(table, canon, shuffled):
    c, ref = _case(table, canon, shuffled)
    got = _run(c, ref["g_wq"])
    keep = ~ref["tie"]
    R.criterion(got["A"], ref["A"], "A")
    R.criterion(got["wm"], ref["wm"], "world_means")
    R.criterion(got["wo"], ref["wo"], "opacities")
    R.criterion(got["wq"], ref["wq"], "world_quats", rows=keep)
    R.criterion(got["d_A"], ref["d_A"], "d_A")
    for k in GRADS:
        R.criterion(got[k], ref[k], k, rows=keep if k == "d_quats" else None)
    inv = c["ids"] == R.INVALID
    assert float(got["wo"].cpu()[inv].abs().max()) == 0.0 and float(got["wo"].cpu()[~inv].abs().min()) > 0.0
    # the one-node form: the same kernels in the same order, so the same bits
    fused = _run(c, ref["g_wq"], fused=True)
    for k in ("wm", "wq", "wo") + GRADS:
        assert torch.equal(fused[k], got[k]), k


def test_unbound_rows_pass_through_as_transform_gaussians_does():
    from emd_amd.motion import transform_gaussians
    c, ref = _case("smpl", True, True)
    got = _run(c, c["g_wq"])
    u = (c["ids"] < 0).to(DEV)
    assert int(u.sum()) == 17
    pose = torch.randn(c["P"], 12, device=DEV)
    wm, wq, wo = transform_gaussians(c["means"].to(DEV), c["quats"].to(DEV), c["opacities"].to(DEV), c["ids"].to(DEV), pose)
    assert torch.equal(got["wm"][u], wm[u]) and torch.equal(got["wq"][u], wq[u]) and torch.equal(got["wo"][u], wo[u])
    assert torch.equal(got["d_means"][u], c["g_wm"].to(DEV)[u]) and torch.equal(got["d_quats"][u], c["g_wq"].to(DEV)[u])
    assert torch.equal(got["d_opacities"][u], c["g_wo"].to(DEV)[u]) and float(got["d_weights"][u].abs().max()) == 0.0


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_bit_reproducible_across_runs_and_streams(shuffled):
    c, ref = _case("smpl", True, shuffled)
    first = _run(c, ref["g_wq"])
    second = _run(c, ref["g_wq"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _run(c, ref["g_wq"])
    side.synchronize()
    for k, v in first.items():
        assert torch.equal(v, second[k]) and torch.equal(v, third[k]), k


def test_layout_independence_of_the_per_instance_sums():
    """The shuffled layout holds the same bound points in other chunks: d_theta / d_trans agree within the criterion (not bit for bit: chunk
    membership differs), and the per-point gradients of a point are the same bits wherever it sits."""
    cs, rs = _case("smpl", True, False)
    cu, ru = _case("smpl", True, True)
    a, b = _run(cs, rs["g_wq"]), _run(cu, ru["g_wq"])
    for k in ("d_theta", "d_trans"):
        R.criterion(b[k], a[k], k + " shuffled vs sorted")
        R.criterion(b[k], rs[k], k + " shuffled vs reference")
    rows = cu["perm"] >= 0
    for k in ("wm", "wq", "wo", "d_means", "d_quats", "d_opacities", "d_weights"):
        assert torch.equal(b[k].cpu()[rows], a[k].cpu()[cu["perm"][rows]]), k


def _step_inputs(c):
    g = torch.Generator().manual_seed(5)
    N = c["ids"].numel()
    leaf = lambda t: t.to(DEV).clone().requires_grad_(True)
    return dict(means=leaf(c["means"]), quats=leaf(c["quats"]), opacity_logits=leaf(torch.randn(N, generator=g) + 2.0),
                log_scales=leaf(torch.randn(N, 3, generator=g) * 0.3 - 2.5), features_dc=leaf(torch.rand(N, 3, generator=g)),
                features_rest=leaf(torch.randn(N, 15, 3, generator=g) * 0.1), point_ids=c["ids"].to(DEV), weights=leaf(c["weights"]),
                theta=leaf(c["theta"]), joints=c["joints"].to(DEV), trans=leaf(c["trans"]), valid=c["valid"].to(DEV),
                camera_center=torch.tensor([0.0, 0.0, -20.0], device=DEV), canon_inv=c["canon_inv"].to(DEV))


LEAVES = ("means", "quats", "opacity_logits", "weights", "theta", "trans", "features_dc", "features_rest", "log_scales")


def _step(inp, layout, gout):
    from emd_amd.nodes import smpl_gaussians
    gs = smpl_gaussians(**inp, sh_degree=3, step=3000, check_finite=False, layout=layout)
    loss = sum((gs[k] * gout[k]).sum() for k in gs)
    grads = torch.autograd.grad(loss, [inp[k] for k in LEAVES])
    return [gs[k] for k in sorted(gs)] + list(grads)


def test_step_replays_from_a_captured_graph_bit_for_bit():
    from emd_amd import smpl
    c, _ = _case("smpl", True, True)
    inp = _step_inputs(c)
    lay = smpl.SkinLayout(c["P"])
    g = torch.Generator().manual_seed(6)
    N = c["ids"].numel()
    gout = {k: torch.randn(*s, generator=g).to(DEV) for k, s in dict(_means=(N, 3), _opacities=(N, 1), _rgbs=(N, 3), _scales=(N, 3), _quats=(N, 4)).items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                            # warm-up: builds the layout (its one host read) and the parent table
        _step(inp, lay, gout)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _step(inp, lay, gout)
    # another pose, written in place into the captured input
    other = R.make_case(R.SMPL_PARENTS, canon=True, shuffled=True, seed=12)["theta"].to(DEV)
    assert not torch.equal(other, inp["theta"])
    with torch.no_grad():
        inp["theta"].copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    eager = _step(inp, lay, gout)
    assert len(eager) == len(captured) == 5 + len(LEAVES)
    for i, (a, b) in enumerate(zip(captured, eager)):
        assert torch.isfinite(b).all() and torch.equal(a, b), i
    assert float(eager[5 + LEAVES.index("theta")].abs().max()) > 0


def test_end_to_end_through_rasterization():
    from emd_amd import gsplat_api, smpl
    from emd_amd.nodes import smpl_gaussians
    c, _ = _case("smpl", True, False)
    inp = _step_inputs(c)
    with torch.no_grad():                                                    # the people stand in front of a camera at the origin looking down +z
        inp["trans"].copy_(torch.tensor([[-1.0, 0.0, 6.0], [0.5, 0.3, 7.0], [0.0, -0.2, 5.0], [1.0, 1.0, 8.0], [1.0, 0.2, 6.5]], device=DEV))
    inp["camera_center"] = torch.zeros(3, device=DEV)
    gs = smpl_gaussians(**inp, sh_degree=3, step=3000, layout=smpl.SkinLayout(c["P"]))
    H, W = 64, 96
    K = torch.tensor([[80.0, 0.0, W / 2], [0.0, 80.0, H / 2], [0.0, 0.0, 1.0]], device=DEV)
    renders, alphas, info = gsplat_api.rasterization(means=gs["_means"], quats=gs["_quats"], scales=gs["_scales"], opacities=gs["_opacities"].squeeze(-1),
                                                     colors=gs["_rgbs"], viewmats=torch.eye(4, device=DEV)[None], Ks=K[None], width=W, height=H,
                                                     near_plane=0.1, render_mode="RGB")
    assert float(alphas.detach().max()) > 0.1
    renders.sum().backward()
    gt = inp["theta"].grad
    assert torch.isfinite(gt).all()
    for p, n in enumerate(R.COUNTS):
        if p == R.INVALID or n == 0:
            assert float(gt[p].abs().max()) == 0.0, p                       # an invalid instance is transparent: exactly no gradient
        else:
            assert float(gt[p].abs().max()) > 0.0, p
    assert float(inp["trans"].grad[R.INVALID].abs().max()) == 0.0
