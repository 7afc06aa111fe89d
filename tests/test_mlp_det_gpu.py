"""-m gpu: the deterministic forms of the MLP kernels (csrc/mlp_det.hip) and of the temporal table's backward (csrc/embed_det.hip), DESIGN.md section
8.14: level_mlp(..., deterministic=True) against the float64 network of tests/test_mlp_gpu.py at that file's bars and against the default mode; the
reduction as a contract (a call's slabs read back and added again in numpy: ascending workgroup, float64 from 0.0, one rounding -- the same bits);
slabs and gradient buffers that start as NaN; the same bits from run to run, on a side stream beside a long copy and in hipGraph replays; the temporal
table's gather form against the oracle, the default kernel and a numpy restatement of its enumeration.  Nothing here asserts that the DEFAULT mode
differs between runs."""
import functools

import numpy as np
import pytest
import torch

from oracle import deform_oracle as do
from tests.test_deform_gpu import test_temporal_embed_vs_oracle as _te_parent
from tests.test_mlp_gpu import _case, _leaves, _net, _reference
from tests.test_mlp_gpu import test_level_mlp_matches_float64 as _mlp_parent

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _param_table(fn):
    mark = next(m for m in fn.pytestmark if m.name == "parametrize")
    return mark.args[1], mark.kwargs.get("ids")


_MLP_CASES = dict(zip(_param_table(_mlp_parent)[1], _param_table(_mlp_parent)[0]))
# one row: a single ragged tile in one workgroup (the seed is chosen on the float64 reference alone: no ReLU of the row within 1e-5 of its kink)
_MLP_CASES["n1"] = _case(1, 128, 4, [(True, 1, 3), (True, 1, 48), (False, 2, 3)], (0, 1), seed=1)
IDS = ["coarse", "fine-recomputed", "ragged", "deep-l1", "first3-l1", "first8-recomputed-l1", "first64", "70k", "n1"]


@functools.lru_cache(maxsize=None)
def _ref(case_id):
    """The float64 reference of a case, computed once (the set-up of test_level_mlp_matches_float64, draw for draw)."""
    N, ka, kb, heads, l1_heads, seed = _MLP_CASES[case_id]
    g = torch.Generator().manual_seed(seed)
    net = _net(g, ka, kb, heads)
    xa = torch.randn(N, ka, generator=g, dtype=torch.float64).requires_grad_(True) if ka else None
    xb = torch.randn(N, kb, generator=g, dtype=torch.float64).requires_grad_(True)
    gouts = [torch.randn(N, o, generator=g, dtype=torch.float64) for _, _, o in heads]
    lam = [0.5 + 0.25 * j for j in range(len(l1_heads))]
    kink = []
    ref = _reference(net, xa, xb, kink, l1_heads)
    ref, ref_l1 = ref[:len(heads)], ref[len(heads):]
    near = torch.stack(kink).min(dim=0).values < 1e-5
    assert int(near.sum()) <= max(8, N // 20)
    assert not l1_heads or int(near.sum()) == 0
    for go in gouts:
        go[near] = 0.0
    (sum((r * go).sum() for r, go in zip(ref, gouts)) + sum(w * r for w, r in zip(lam, ref_l1))).backward()
    return dict(net=net, xa=xa, xb=xb, gouts=gouts, lam=lam, outs=[r.detach() for r in ref + ref_l1], ka=ka, heads=heads, l1_heads=l1_heads)


@functools.lru_cache(maxsize=None)
def _hip(case_id, deterministic):
    """One forward + backward of the case on the device: outputs, dL/dxa, dL/dxb, parameter gradients (in _leaves' order), on the CPU."""
    from emd_amd.mlp import level_mlp
    r = _ref(case_id)
    net = r["net"]
    c = lambda t: None if t is None else t.detach().to(DEV, torch.float32).requires_grad_(True)
    hx, hb = c(r["xa"]), c(r["xb"])
    hnet = dict(w0=c(net["w0"]), b=c(net["b"]),
                branches=[(ri, [(c(w), c(b)) for w, b in hid], (c(wo), c(bo))) for ri, hid, (wo, bo) in net["branches"]])
    outs = level_mlp(hx, hb, hnet["w0"], hnet["b"], net["col_a"], net["col_b"], hnet["branches"], l1_heads=r["l1_heads"], deterministic=deterministic)
    nh = len(r["heads"])
    assert len(outs) == nh + len(r["l1_heads"])
    (sum((o * go.to(DEV, torch.float32)).sum() for o, go in zip(outs[:nh], r["gouts"])) + sum(w * o for w, o in zip(r["lam"], outs[nh:]))).backward()
    cpu = lambda t: None if t is None else t.detach().cpu()
    return dict(outs=[cpu(o) for o in outs], d_xa=cpu(hx.grad) if hx is not None else None, d_xb=cpu(hb.grad), grads=[cpu(t.grad) for t in _leaves(hnet)])


@pytest.mark.parametrize("case_id", IDS)
def test_deterministic_level_matches_float64_at_the_bars_of_the_default_mode(case_id):
    r, h = _ref(case_id), _hip(case_id, True)
    ka = r["ka"]
    for k, (o, want) in enumerate(zip(h["outs"], r["outs"])):
        err = float((o.double() - want).abs().max())
        assert err <= 2e-5 * max(1.0, float(want.abs().max())), ("output", k, err)

    def check(name, got, want):
        scale = max(float(want.abs().max()), 1e-12)
        err = float((got.double() - want).abs().max())
        assert err <= 1e-4 * scale, (name, err, scale)
    if r["xa"] is not None:
        check("d_xa", h["d_xa"], r["xa"].grad)
    check("d_xb", h["d_xb"], r["xb"].grad)
    dw0, rw0 = h["grads"][0], r["net"]["w0"].grad
    if ka:
        check("d_w0[a]", dw0[:, :ka], rw0[:, :ka])
    check("d_w0[b]", dw0[:, ka + 32:], rw0[:, ka + 32:])
    assert float(dw0[:, ka:ka + 32].abs().max()) == 0.0          # the temporal columns are not the kernels' business: the caller's zeros stay
    for k, (a, b) in enumerate(zip(h["grads"][1:], _leaves(r["net"])[1:])):
        check(f"param {k}", a, b.grad)


@pytest.mark.parametrize("case_id", IDS)
def test_deterministic_level_against_the_default_mode(case_id):
    """The mode does not touch the head outputs, dL/dxa and dL/dxb: the same bits.  Weight and bias gradients and the regularisers are the same sums in
    another order: the bar tests/test_mlp_gpu.py uses for float atomics against rounding."""
    r, d, a = _ref(case_id), _hip(case_id, True), _hip(case_id, False)
    nh = len(r["heads"])
    for k in range(nh):
        assert torch.equal(d["outs"][k], a["outs"][k]), ("output", k)
    assert (d["d_xa"] is None) == (a["d_xa"] is None) and (d["d_xa"] is None or torch.equal(d["d_xa"], a["d_xa"]))
    assert torch.equal(d["d_xb"], a["d_xb"])
    for k, (x, y) in enumerate(zip(d["grads"] + d["outs"][nh:], a["grads"] + a["outs"][nh:])):
        assert float((x - y).abs().max()) <= 2e-5 * max(float(y.abs().max()), 1e-20), (k, float((x - y).abs().max()), float(y.abs().max()))


def _device_level(N, ka, kb, heads, l1_heads, seed):
    """A level on the device with fixed inputs; step() runs forward + backward and returns (outputs, gradients of xa, xb and every parameter)."""
    from emd_amd import mlp
    g = torch.Generator().manual_seed(seed)
    net = _net(g, ka, kb, heads)
    c = lambda t: t.detach().to(DEV, torch.float32).requires_grad_(True)
    xa = torch.randn(N, ka, generator=g).to(DEV).requires_grad_(True) if ka else None
    xb = torch.randn(N, kb, generator=g).to(DEV).requires_grad_(True)
    gouts = [torch.randn(N, o, generator=g).to(DEV) for _, _, o in heads]
    hnet = dict(w0=c(net["w0"]), b=c(net["b"]), branches=[(ri, [(c(w), c(b)) for w, b in hid], (c(wo), c(bo))) for ri, hid, (wo, bo) in net["branches"]])
    leaves = ([xa] if ka else []) + [xb] + _leaves(hnet)

    def step(deterministic=True):
        outs = mlp.level_mlp(xa, xb, hnet["w0"], hnet["b"], net["col_a"], net["col_b"], hnet["branches"], l1_heads=l1_heads, deterministic=deterministic)
        loss = sum((o * go).sum() for o, go in zip(outs, gouts)) + sum((0.5 + 0.25 * j) * o for j, o in enumerate(outs[len(heads):]))
        return [o.detach() for o in outs], list(torch.autograd.grad(loss, leaves))
    return step, hnet, ka


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.mark.parametrize("N,ka,groups", [(1000, 128, 8), (1000, 0, 8), (70001, 128, 256)], ids=["8-workgroups", "8-workgroups-recomputed", "capped-grid"])
def test_the_reduction_is_the_contract(N, ka, groups, monkeypatch):
    """Every weight and bias gradient and every L1 mean of a call equals, bit for bit, its slab (read back through the offsets emd_mlp_det_slab_bytes
    reports) added again in numpy: ascending workgroup, float64 from 0.0, times the scale in float64, one rounding to float32."""
    from emd_amd import mlp
    heads = [(True, 1, 3), (True, 1, 1), (True, 1, 48)] + ([(False, 2, 3)] if ka else [])
    l1_heads = (0, 2)
    step, hnet, _ = _device_level(N, ka, 4, heads, l1_heads, seed=N + ka)
    trace = []
    monkeypatch.setattr(mlp, "DET_TRACE", trace)
    outs, grads = step()
    torch.cuda.synchronize()
    assert [t["direction"] for t in trace] == ["forward", "backward"]
    fwd, bwd = trace
    assert len(fwd["jobs"]) == len(l1_heads) and len(bwd["jobs"]) == sum(2 * d + 2 for _, d, _ in heads) + (3 if ka else 2)

    def restate(t, j):
        assert j["offset"] % 256 == 0 and j["pitch"] >= j["rows"] * j["cols"]
        slab = t["slab"][j["offset"]:j["offset"] + 4 * j["groups"] * j["pitch"]].view(torch.float32).view(j["groups"], j["pitch"]).cpu().numpy()
        acc = np.zeros(j["rows"] * j["cols"], dtype=np.float64)
        for s in range(j["groups"]):                                  # ascending workgroup index, one add each
            acc = acc + slab[s, :j["rows"] * j["cols"]].astype(np.float64)
        return (acc * np.float64(j["scale"])).astype(np.float32).reshape(j["rows"], j["cols"])

    def written(j):
        dst = j["dst"].detach()
        return (dst[:, j["col0"]:j["col0"] + j["cols"]] if j["rows"] > 1 else dst.reshape(1, -1)[:, j["col0"]:j["col0"] + j["cols"]]).cpu().numpy()
    # the regularisers: the forward's jobs, in the order of l1_heads; two workgroups per CU for the one-tile heads, one for the 48-wide head
    for j, k, o in zip(fwd["jobs"], l1_heads, outs[len(heads):]):
        assert j["groups"] == (groups if heads[k][2] > 32 else min(2 * groups, -(-(-(-N // 32)) // 4)))
        assert j["scale"] == 1.0 / (float(N) * float(heads[k][2]))
        want = restate(fwd, j)
        assert np.array_equal(want.view(np.uint32).ravel(), _bits(o).ravel()), ("l1", k)
    # the gradients: per head (w_h, b_h) x depth, w_out, b_out, then the trunk's blocks of d_w0 and d_b -- against what autograd handed out
    leaves = _leaves(hnet)
    params, w0_grad, b_grad = grads[-(len(leaves) - 2):], grads[-len(leaves)], grads[-len(leaves) + 1]
    jobs = list(bwd["jobs"])
    for k, got in enumerate(params):
        j = jobs.pop(0)
        assert j["groups"] == groups and j["col0"] == 0
        assert np.array_equal(restate(bwd, j).view(np.uint32).ravel(), _bits(got).ravel()), ("param", k)
    col = 0
    for j in jobs[:-1]:                                               # the xa block (with HexPlane features) and the embedding block of d_w0
        assert j["groups"] == groups
        assert np.array_equal(restate(bwd, j).view(np.uint32), _bits(w0_grad[:, j["col0"]:j["col0"] + j["cols"]])), ("d_w0", j["col0"])
        col += j["cols"]
    assert col == ka + 4 and float(w0_grad[:, ka:ka + 32].abs().max()) == 0.0
    assert np.array_equal(restate(bwd, jobs[-1]).view(np.uint32).ravel(), _bits(b_grad).ravel())
    for t in trace:                                                   # and the reduction wrote what it computed where the job says
        for j in t["jobs"]:
            assert np.array_equal(restate(t, j).view(np.uint32), written(j).view(np.uint32))


@pytest.mark.parametrize("ka", [128, 0], ids=["coarse", "fine-recomputed"])
def test_nan_filled_slabs_and_gradient_buffers(ka, monkeypatch):
    """The slab is never read before it is written and the reduction writes, it does not add: with a slab and gradient buffers that start as NaN
    (all but the temporal columns of d_w0, which nobody writes: the caller's zeros) no NaN comes out, the guard bands around the slab keep every byte,
    and the temporal columns stay exactly 0."""
    from emd_amd import mlp
    N, GUARD = 1000, 4096
    heads = [(True, 1, 3), (True, 1, 1), (True, 1, 48)] + ([(False, 2, 3)] if ka else [])
    step, hnet, _ = _device_level(N, ka, 4, heads, (0, 2), seed=11 + ka)
    ld = ka + 32 + 4
    made = []

    def slab(nbytes, dev):
        buf = torch.full((nbytes + 2 * GUARD,), 0xFF, device=dev, dtype=torch.uint8)          # 0xFFFFFFFF: a NaN in every float
        made.append((buf, nbytes))
        return buf[GUARD:GUARD + nbytes]

    def grads(numel, dev):
        flat = torch.full((numel,), float("nan"), device=dev, dtype=torch.float32)
        flat[:64 * ld].view(64, ld)[:, ka:ka + 32] = 0.0
        return flat
    monkeypatch.setattr(mlp, "_alloc_slab", slab)
    monkeypatch.setattr(mlp, "_alloc_grads", grads)
    outs, got = step()
    torch.cuda.synchronize()
    assert len(made) == 2
    for buf, nbytes in made:
        assert bool((buf[:GUARD] == 0xFF).all()) and bool((buf[GUARD + nbytes:] == 0xFF).all())
    for k, t in enumerate(outs + got):
        assert bool(torch.isfinite(t).all()), k
    w0_grad = got[-len(_leaves(hnet))]
    assert float(w0_grad[:, ka:ka + 32].abs().max()) == 0.0 and float(w0_grad.abs().max()) > 0.0
    # and the values are those of a run with the usual allocations
    monkeypatch.undo()
    outs2, got2 = step()
    for a, b in zip(outs + got, outs2 + got2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("ka", [128, 0], ids=["coarse", "fine-recomputed"])
def test_same_bits_in_every_setting(ka):
    """Two eager runs, a run on a side stream while a long copy occupies the default stream, and two replays of a captured forward + backward."""
    heads = [(True, 1, 3), (True, 1, 1), (True, 1, 48)] + ([(False, 2, 3)] if ka else [])
    step, _, _ = _device_level(5003, ka, 4, heads, (0, 2), seed=41 + ka)
    flat = lambda r: [t.clone() for t in r[0] + r[1]]
    runs = [flat(step()), flat(step())]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    src = torch.empty(1 << 26, device=DEV)
    dst = torch.empty_like(src)
    for _ in range(4):
        dst.copy_(src)                                               # 256 MB each way, on the default stream
    with torch.cuda.stream(side):
        runs.append(flat(step()))
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                       # (warm-up on the capture stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = step()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        runs.append(flat(captured))
    names = ["eager 2", "side stream", "replay 1", "replay 2"]
    for name, run in zip(names, runs[1:]):
        for k, (a, b) in enumerate(zip(runs[0], run)):
            assert torch.equal(a, b), f"{name} differs from the first eager run in tensor {k}"
    for k, t in enumerate(runs[0]):
        assert bool(torch.isfinite(t).all()) and float(t.abs().sum()) > 0, k


# ---- the temporal table ----------------------------------------------------------------------------------------------------------------------------
_TE_CASES = list(_param_table(_te_parent)[0]) + [(20, 8, 5, 0.5), (150, 32, 30, 14.0 / 29.0), (12, 6, 12, 1.0)]          # ... and t on a row boundary, t = 1 at k = rows


def _f(x):
    return np.float32(x)


def _reflect(c, size):
    """reflect_coord of csrc/temporal_sample.h in float32, operation for operation (no contraction there)."""
    v = ((_f(c) + _f(1)) * _f(0.5)) * _f(size - 1)
    if size <= 1:
        return _f(0)
    span = _f(size - 1)
    if v < 0:
        v = -v
    extra = np.fmod(v, span)
    flips = int(np.floor(v / span))
    v = span - extra if flips & 1 else extra
    if not v > 0:
        v = _f(0)
    elif not v < span:
        v = span
    return _f(v)


def _resized_row(r, k, rows):
    scale = _f(rows - 1) / _f(k - 1) if k > 1 else _f(0)
    src = scale * _f(r)
    h0 = int(src)
    h1 = h0 + (1 if h0 < rows - 1 else 0)
    l1 = src - _f(h0)
    return h0, h1, _f(1) - l1, l1


def _te_restated(rows, dim, k, t, g):
    """dL/dtable of one table: the default kernel's adds in its issue order -- j ascending, r = 0, 1, then (ha, x0), (hb, x0), (ha, x1), (hb, x1) --,
    each product formed left to right in float32, added in float64 from 0.0, rounded once."""
    iy = _reflect((_f(t) - _f(0.5)) * _f(2), k)
    y0f = np.floor(iy)
    y0 = int(y0f)
    wy1 = iy - y0f
    wy = (_f(1) - wy1, wy1)
    row = [_resized_row(min(y0, k - 1), k, rows), _resized_row(min(y0 + 1, k - 1), k, rows)]
    in1 = y0 + 1 <= k - 1
    G = np.zeros((rows, dim), dtype=np.float64)
    for j in range(dim):
        gx = (_f(j) / _f(dim - 1) - _f(0.5)) * _f(2) if dim > 1 else _f(-1)
        ix = _reflect(gx, dim)
        x0f = np.floor(ix)
        x0 = int(x0f)
        wx1 = ix - x0f
        wx0 = _f(1) - wx1
        for r in range(2):
            if r == 1 and not in1:
                continue
            ha, hb, la, lb = row[r]
            G[ha, x0] += np.float64(_f(g[j]) * wx0 * wy[r] * la)
            G[hb, x0] += np.float64(_f(g[j]) * wx0 * wy[r] * lb)
            if x0 + 1 <= dim - 1:
                G[ha, x0 + 1] += np.float64(_f(g[j]) * wx1 * wy[r] * la)
                G[hb, x0 + 1] += np.float64(_f(g[j]) * wx1 * wy[r] * lb)
    return G.astype(np.float32)


def _te_run(w, t, k, gout, deterministic):
    from emd_amd.deformation import temporal_embed
    w1, t1 = w.to(DEV).requires_grad_(True), torch.tensor([t], device=DEV, requires_grad=True)
    e1 = temporal_embed(w1, t1, k, deterministic=deterministic)
    (e1 * gout.to(DEV)).sum().backward()
    return e1.detach().cpu(), w1.grad.cpu(), t1.grad.cpu().reshape(())


@pytest.mark.parametrize("rows,dim,k,t", _TE_CASES)
def test_temporal_table_gather_form(rows, dim, k, t):
    g = torch.Generator().manual_seed(rows * 1000 + k)
    w = torch.randn(rows, dim, generator=g)
    gout = torch.randn(dim, generator=g)
    w0, t0 = w.clone().requires_grad_(True), torch.tensor(t, requires_grad=True)
    (do.temporal_embed(w0, k, t0) * gout).sum().backward()
    e_d, gw_d, gt_d = _te_run(w, t, k, gout, True)
    e_a, gw_a, gt_a = _te_run(w, t, k, gout, False)
    # against the oracle: the bars of test_temporal_embed_vs_oracle
    np.testing.assert_allclose(gw_d.numpy(), w0.grad.numpy(), rtol=1e-5, atol=5e-6)
    np.testing.assert_allclose(gt_d.numpy(), t0.grad.numpy(), rtol=1e-4, atol=1e-4)
    # against the default kernel: the forward is the same launch; the table gradient is the same products added in another order and precision
    assert torch.equal(e_d, e_a)
    assert float((gw_d - gw_a).abs().max()) <= 1e-6 * max(float(gw_a.abs().max()), 1e-20)
    # dL/dt: the same `dim` terms, each at most 2 max|g| max|w| wx, with contraction off here and left to the compiler there: a few float32 roundings
    # per term, times d iy / d t = k - 1
    assert abs(float(gt_d - gt_a)) <= 1e-6 * dim * float(gout.abs().max()) * float(w.abs().max()) * max(k - 1, 1)
    # against the enumeration restated in numpy: bit for bit; rows no sample touches keep the caller's zeros
    want = _te_restated(rows, dim, k, t, gout.numpy())
    assert np.array_equal(want.view(np.uint32), gw_d.numpy().view(np.uint32))
    assert int((np.abs(want).sum(axis=1) > 0).sum()) <= 4


def test_temporal_table_gather_form_batched():
    """Three tables: each table's gradient as its own single-table call gives it, bit for bit; dL/dt is the tables' values added in ascending order."""
    g = torch.Generator().manual_seed(5)
    rows, dim, k, t = 150, 32, 44, 0.61
    w = torch.randn(3, rows, dim, generator=g)
    gout = torch.randn(3, dim, generator=g)
    _, gw, gt = _te_run(w, t, k, gout, True)
    _, gw_a, gt_a = _te_run(w, t, k, gout, False)
    _, gw2, gt2 = _te_run(w, t, k, gout, True)
    assert torch.equal(gw, gw2) and torch.equal(gt, gt2)
    total = np.float32(0)
    for a in range(3):
        _, gw1, gt1 = _te_run(w[a], t, k, gout[a], True)
        assert torch.equal(gw[a], gw1), a
        assert np.array_equal(_te_restated(rows, dim, k, t, gout[a].numpy()).view(np.uint32), gw[a].numpy().view(np.uint32)), a
        total = np.float32(total + np.float32(gt1.numpy()))
    assert np.float32(gt.numpy()) == total
    assert float((gw - gw_a).abs().max()) <= 1e-6 * float(gw_a.abs().max())
    assert abs(float(gt - gt_a)) <= 1e-6 * 3 * dim * float(gout.abs().max()) * float(w.abs().max()) * (k - 1)
