"""-m gpu: the neighbour-std regulariser (knn.neighbour_std on emd_neighbour_std_forward / _backward, csrc/neighbour_reg.hip) and the SMPLNodes
store on an MI355X, against the fp64 restatement of tests/neighbour_std_ref.py (pinned by tests/test_neighbour_std_cpu.py, which also asserts the
input conditions of every case below).  Terms: relative, at four times the rounding count derived in neighbour_std_ref.py (DESIGN.md section
8.19).  Gradients: the project's rule, element-wise 1e-4 |ref| + 1e-6 max|ref| and relative L2 <= 1e-5, per block."""
import ctypes as C
import functools
import types

import pytest
import torch

from tests import neighbour_std_cases as cases
from tests import neighbour_std_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _table(K):
    """The device table of a case: built by the code under test and required to BE the contract's table, on which the conditions were asserted."""
    from emd_amd.knn import KnnTable
    pts, seg = cases.cloud()
    t = KnnTable(pts.to(DEV), k=K - 1, segment_start=seg.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(t.idx.cpu().long(), cases.table(K)), "the device table differs from the fp64 table of the case"
    return t


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = cases.build(name)
    return R.reference(c["blocks"], c["idx"], c["weights"], c["acts"], c["g_terms"])


def _run(c, table):
    from emd_amd.knn import neighbour_std
    xs = [b.to(DEV).clone().requires_grad_(True) for b in c["blocks"]]
    terms = neighbour_std(xs, table, c["weights"], c["acts"])
    (terms * c["g_terms"].to(DEV)).sum().backward()
    return terms.detach(), [x.grad for x in xs]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_terms_and_gradients_match_the_fp64_restatement(name):
    c = cases.build(name)
    table = _table(c["K"])
    terms, grads = _run(c, table)
    ref_terms, ref_grads = _reference(name)
    assert terms.shape == (len(c["blocks"]),) and terms.dtype == torch.float32
    R.terms_close(terms, ref_terms, c["acts"], c["weights"], name, rtol=R.TIGHT_RTOL if c["tight"] else None)
    for b, (got, ref) in enumerate(zip(grads, ref_grads)):
        assert (got is None) == (ref is None) == (c["weights"][b] == 0), b
        if ref is not None:
            assert got.shape == c["blocks"][b].shape
            R.grad_close(got, ref, f"{name} block {b}")
    # groups with -1 slots and groups of one are part of every case
    assert int((table.idx == -1).sum()) > 0 and int(((table.idx >= 0).sum(dim=1) == 0).sum()) > 0


def test_identical_members_give_exactly_zero():
    c = cases.build("K3-identical")
    terms, grads = _run(c, _table(3))
    for b in (0, 2):                                                     # quaternions and opacities: every group bit-identical
        assert float(terms[b]) == 0.0 and torch.count_nonzero(grads[b]) == 0 and torch.isfinite(grads[b]).all()
    for b in (1, 3, 4):
        assert float(terms[b]) > 0.0 and torch.count_nonzero(grads[b]) > 0


def _direct(c, table, fill=float("nan")):
    """The C entry points on buffers of the test's own: every gradient buffer pre-filled with NaN -> (terms, [dx])."""
    from emd_amd import _lib as L
    lib = L.load()
    n = cases.N
    xs = [b.to(DEV).reshape(n, -1).contiguous() for b in c["blocks"]]
    a = L.EmdNeighbourStdArgs()
    a.num_points, a.k, a.num_blocks = n, table.k, len(xs)
    a.idx, a.rev_start, a.rev_slot = table.idx.data_ptr(), table.rev_start.data_ptr(), table.rev_slot.data_ptr()
    dxs = [torch.full_like(x, fill) for x in xs]
    for b, (x, act, w) in enumerate(zip(xs, c["acts"], c["weights"])):
        a.x[b], a.dx[b], a.cols[b], a.act[b], a.weight[b] = x.data_ptr(), dxs[b].data_ptr(), x.shape[1], L.NSTD_ACT[act], w
    cols = sum(x.shape[1] for x, w in zip(xs, c["weights"]) if w != 0)
    stash = torch.full((n * cols * 2,), fill, device=DEV)
    terms = torch.full((len(xs),), fill, device=DEV)
    ws = torch.zeros(lib.emd_neighbour_std_workspace_size(), dtype=torch.uint8, device=DEV)
    g = c["g_terms"].to(DEV).float().contiguous()
    a.stash, a.terms, a.g_terms = stash.data_ptr(), terms.data_ptr(), g.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.emd_neighbour_std_forward(C.byref(a), ws.data_ptr(), ws.numel(), st), "emd_neighbour_std_forward")
    L.check(lib.emd_neighbour_std_backward(C.byref(a), st), "emd_neighbour_std_backward")
    torch.cuda.synchronize()
    assert int(ws[:16].count_nonzero()) == 0, "the ticket must be zero again after the call"
    return terms, dxs


def test_zero_weight_blocks_are_skipped_and_every_other_element_is_written():
    c = cases.build("K3-zero-weights")
    table = _table(3)
    terms, dxs = _direct(c, table)
    auto_terms, auto_grads = _run(c, table)
    assert torch.equal(terms, auto_terms) and torch.isfinite(terms).all()
    for b, w in enumerate(c["weights"]):
        if w == 0:
            assert float(terms[b]) == 0.0 and torch.isnan(dxs[b]).all() and auto_grads[b] is None        # untouched: no gradient at all
        else:
            assert torch.isfinite(dxs[b]).all(), f"block {b}: an element of the gradient was not written"
            assert torch.equal(dxs[b].reshape(auto_grads[b].shape), auto_grads[b])
    # the full set as well: no NaN survives in any block
    full = cases.build("K9-deg3")
    _, dxs = _direct(full, _table(9))
    assert all(torch.isfinite(d).all() for d in dxs)


def test_bit_identical_across_runs_streams_and_graph_replay():
    from emd_amd.knn import neighbour_std
    c = cases.build("K3-deg1")
    table = _table(3)
    first = _run(c, table)
    second = _run(c, table)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _run(c, table)
    side.synchronize()
    for other in (second, third):
        assert torch.equal(first[0], other[0])
        for a, b in zip(first[1], other[1]):
            assert torch.equal(a, b)
    # captured once on a single stream, replayed twice with other values in place
    statics = [b.to(DEV).clone().requires_grad_(True) for b in c["blocks"]]
    gt = c["g_terms"].to(DEV)
    with torch.cuda.stream(side):                                        # warm-up on the capture stream (allocator, autograd)
        (neighbour_std(statics, table, c["weights"], c["acts"]) * gt).sum().backward()
        for s in statics:
            s.grad = None
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static_terms = neighbour_std(statics, table, c["weights"], c["acts"])
        (static_terms * gt).sum().backward()
    other = cases.build("K3-zero-weights")                               # the same shapes, other values
    for src, ref in ((other, _run(dict(other, weights=c["weights"]), table)), (c, first)):
        with torch.no_grad():
            for s, v in zip(statics, src["blocks"]):
                s.copy_(v.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_terms.detach(), ref[0])
        for s, r in zip(statics, ref[1]):
            assert torch.equal(s.grad, r)


# ---- SMPLNodes --------------------------------------------------------------------------------------------------------------------------------
CTRL = dict(sh_degree=1, check_finite=False, knn_neighbors=3, knn_update_interval=100)
REG = dict(knn_reg=dict(lambda_std_q=0.002, lambda_std_s=0.002, lambda_std_o=0.0005, lambda_std_shs_dc=0.001, lambda_std_shs_rest=0.001))


def _smpl_node():
    from emd_amd.nodes import SMPLNodes
    g = torch.Generator().manual_seed(51)
    P, n, F = 3, 200, 4
    N = P * n
    ids = torch.arange(P).repeat_interleave(n)[torch.randperm(N, generator=g)]          # unsorted: creation groups them
    node = SMPLNodes("SMPLNodes", CTRL, reg=REG, device=DEV)
    w = torch.rand(N, 24, generator=g) ** 4
    quats = torch.randn(N, 4, generator=g)
    node.create_from_tensors(torch.randn(N, 3, generator=g) * 0.4, torch.rand(N, 3, generator=g), torch.randn(N, 3, generator=g) * 0.3 - 3.0, ids,
                             torch.randn(F, P, 4, generator=g), torch.randn(F, P, 23, 4, generator=g), torch.randn(F, P, 3, generator=g) * 3,
                             torch.ones(P, 3), torch.rand(F, P, generator=g) > 0.1, torch.randn(P, 24, 3, generator=g) * 0.3, w / w.sum(dim=1, keepdim=True),
                             quats=quats)
    with torch.no_grad():                                                # values a trained model would have: no block is constant
        node._opacities.add_(torch.randn(N, 1, generator=g).to(DEV))
        node._features_rest.add_(torch.randn(N, 3, 3, generator=g).to(DEV) * 0.1)
    return node, ids, N, P


def test_smpl_nodes_step_end_to_end():
    node, ids, N, P = _smpl_node()
    assert node.num_points == N and torch.equal(node.ids32.cpu().long(), ids.sort().values)
    assert node.segment_start.cpu().tolist() == [0, 200, 400, 600] and node.segment_start.dtype == torch.int32
    groups = node.get_param_groups()
    for short, attr in (("ins_rotation", "instances_quats"), ("smpl_rotation", "smpl_quats"), ("ins_translation", "instances_trans"), ("xyz", "_means")):
        assert groups["SMPLNodes#" + short][0] is getattr(node, attr)
    assert node.smpl_quats.shape == (4, P, 23, 4) and "SMPLNodes#embedding" not in groups
    opt = torch.optim.Adam([dict(params=p, name=k, lr=1e-3) for k, p in groups.items()])
    cam = types.SimpleNamespace(camtoworlds=torch.eye(4, device=DEV) + torch.tensor([[0, 0, 0, 0.3], [0, 0, 0, -2.0], [0, 0, 0, 9.0], [0, 0, 0, 0]], device=DEV))
    node.preprocess_per_train_step(100)
    node.set_cur_frame(2)
    gs = node.get_gaussians(cam)
    assert {k: tuple(v.shape) for k, v in gs.items()} == dict(_means=(N, 3), _opacities=(N, 1), _rgbs=(N, 3), _scales=(N, 3), _quats=(N, 4))
    reg = node.compute_reg_loss()
    assert list(reg) == ["knn_reg"] and node.knn_table is not None and node.knn_table.k == 2
    (sum((v * v).sum() for v in gs.values()) * 1e-3 + reg["knn_reg"]).backward()
    assert all(torch.isfinite(p.grad).all() for p in (node.smpl_quats, node.instances_quats, node.instances_trans, node._means))
    assert float(node.smpl_quats.grad[2].abs().max()) > 0 and float(node.smpl_quats.grad[0].abs().max()) == 0          # only the current frame is posed
    # the table keeps to the instances, and knn_reg with its parameter gradients is the restatement on the class's own table
    t = node.knn_table
    assert (t.idx.cpu().long() // 200 == torch.arange(N)[:, None] // 200).all()
    R.check_segments(node._means.detach().cpu(), node.segment_start.cpu(), t.idx.cpu(), t.d2.cpu(), 2)
    attrs = [a for a, _ in node.KNN_REG_BLOCKS.values()]
    acts = [a for _, a in node.KNN_REG_BLOCKS.values()]
    weights = [REG["knn_reg"][k] for k in node.KNN_REG_BLOCKS]
    blocks = [getattr(node, a).detach().cpu() for a in attrs]
    R.assert_conditions(blocks, t.idx.cpu(), acts)
    only = {a: torch.autograd.grad(node.compute_reg_loss()["knn_reg"], getattr(node, a))[0] for a in attrs}
    ref_terms, ref_grads = R.reference(blocks, t.idx.cpu(), weights, acts)
    value = float(reg["knn_reg"].detach())
    rel = abs(value - float(ref_terms.sum())) / float(ref_terms.sum())
    print(f"SMPLNodes knn_reg {value:.9e} ref {float(ref_terms.sum()):.9e} rel {rel:.3e}")
    assert rel <= max(R.term_rtol(a) for a in acts)
    for a, ref in zip(attrs, ref_grads):
        R.grad_close(only[a], ref, "SMPLNodes " + a)
    # the refinement hook: a refresh at the interval and nothing else
    opt.step()
    before = dict(n=node.num_points, ids=node.point_ids.clone(), state={k: {s: v.clone() for s, v in opt.state[p[0]].items()} for k, p in groups.items()},
                  params={k: p[0] for k, p in groups.items()})
    with torch.no_grad():
        node._means.add_(torch.randn(N, 3, generator=torch.Generator().manual_seed(52)).to(DEV) * 0.2)
    old = t.idx.clone()
    node.preprocess_per_train_step(150)
    assert node.refinement_after(150, opt) is None and node.knn_table is t and torch.equal(t.idx, old)                 # not at the interval
    node.preprocess_per_train_step(200)
    assert node.refinement_after(200, opt) is None and node.knn_table is t and not torch.equal(t.idx, old)             # refreshed in place
    R.check_segments(node._means.detach().cpu(), node.segment_start.cpu(), t.idx.cpu(), t.d2.cpu(), 2)
    assert node.num_points == before["n"] and torch.equal(node.point_ids, before["ids"])
    for k, p in node.get_param_groups().items():
        assert p[0] is before["params"][k]
        for s, v in opt.state[p[0]].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(before["state"][k][s])), (k, s)


def test_smpl_nodes_without_the_key_or_with_sh_degree_0():
    from emd_amd.nodes import SMPLNodes
    node, _, N, _ = _smpl_node()
    node.reg_cfg = None
    assert node.compute_reg_loss() == {}
    g = torch.Generator().manual_seed(53)
    flat = SMPLNodes("SMPLNodes", dict(CTRL, sh_degree=0, knn_neighbors=4), reg=REG, device=DEV)
    flat.create_from_tensors(torch.randn(90, 3, generator=g), torch.rand(90, 3, generator=g), torch.randn(90, 3, generator=g) * 0.3 - 3.0,
                             torch.arange(90) % 2, torch.randn(1, 2, 4, generator=g), torch.randn(1, 2, 23, 4, generator=g), torch.zeros(1, 2, 3),
                             torch.ones(2, 3), torch.ones(1, 2, dtype=torch.bool), torch.zeros(2, 24, 3), torch.full((90, 24), 1 / 24),
                             quats=torch.randn(90, 4, generator=g))
    assert flat._features_rest.shape == (90, 0, 3)
    reg = flat.compute_reg_loss()["knn_reg"]                             # four blocks: the rest block has no rows
    reg.backward()
    assert flat.knn_table.k == 3 and float(reg) > 0 and flat._features_rest.grad is None and float(flat._quats.grad.abs().max()) > 0
