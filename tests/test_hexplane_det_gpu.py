"""-m gpu: the deterministic HexPlane backward (HexPlaneField.deterministic / DeterministicSum, EMD_HEX_FLAG_DETERMINISTIC).
Every plane gradient is the pinned sum (tests/segsum_checks.py) of the call's own contribution lists, bit for bit; all outputs have identical bits
from run to run, under other work on the device, for every visiting order and in a hipGraph replay; and the values stay inside the bound of
tests/test_hexplane_gpu.py against the CPU oracle.  The oracle's results are computed once per case and shared."""
import functools

import numpy as np
import pytest
import torch

from oracle import hexplane_oracle as ho
from tests import segsum_checks as sg
from tests.test_hexplane_gpu import _close

pytestmark = pytest.mark.gpu
RES, MULTIRES, BOUNDS = [16, 12, 10, 6], [1, 2, 4], 1.6
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
LAYOUTS = ("uniform", "clustered", "same_time", "per_point_times")


def _scale_res(s):
    return [r * MULTIRES[s] for r in RES[:3]] + RES[3:]


@functools.lru_cache(maxsize=None)
def _case(C, layout, N):
    """Inputs on the CPU and the oracle's features and gradients for them (numpy), computed once."""
    g = torch.Generator().manual_seed(1000 * C + 7 * N + len(layout))
    planes = [[torch.rand([1, C, _scale_res(s)[b], _scale_res(s)[a]], generator=g) + 0.3 for a, b in PAIRS] for s in range(len(MULTIRES))]
    pts = torch.rand(N, 3, generator=g) * 3.6 - 1.8                      # bounds 1.6: border clamps occur
    t = torch.rand(N, 1, generator=g) * 2.2 - 1.1
    if layout == "clustered":
        pts = torch.randn(N, 3, generator=g) * 0.02 + torch.tensor([0.3, -0.7, 1.1])
    elif layout == "same_time":
        t = torch.full((N, 1), 0.21)
    elif layout == "per_point_times":                                    # every point inside the box, times beyond the time axis at both ends
        pts = torch.rand(N, 3, generator=g) * 3.0 - 1.5
        t = torch.rand(N, 1, generator=g) * 2.6 - 1.3
    elif layout == "outside":
        # 1100 points beyond the corner the LAST texel of every spatial plane sits at (normalised coordinate > 1 on every axis: x1 == x0, y1 == y0,
        # all four taps on that one texel) + 2000 ordinary ones
        assert N == 3100
        pts[:1100] = -1.65 - 0.15 * torch.rand(1100, 3, generator=g)
    else:
        assert layout == "uniform"
    gout = torch.randn(N, C * len(MULTIRES), generator=g)
    aabb = torch.tensor([[BOUNDS] * 3, [-BOUNDS] * 3])
    ref = None
    if N > 0:
        p0, t0 = pts.clone().requires_grad_(True), t.clone().requires_grad_(True)
        pl0 = [[p.clone().requires_grad_(True) for p in sc] for sc in planes]
        f0 = ho.hexplane_features(p0, t0, aabb, pl0)
        (f0 * gout).sum().backward()
        ref = dict(feat=f0.detach().numpy(), pts=p0.grad.numpy(), times=t0.grad.numpy(), planes=[[p.grad.numpy() for p in sc] for sc in pl0])
    return dict(C=C, N=N, pts=pts, t=t, gout=gout, planes=planes, ref=ref)


def _field(case, dev, deterministic=True, planes_grad=True):
    from emd_amd.hexplane import HexPlaneField
    cfg = {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": case["C"], "resolution": RES}
    field = HexPlaneField(BOUNDS, cfg, MULTIRES).to(dev)
    field.deterministic = deterministic
    for gp, vals in zip(field.grids, case["planes"]):
        for prm, v in zip(gp, vals):
            prm.data = v.to(dev).contiguous(memory_format=torch.channels_last)
            prm.requires_grad_(planes_grad)
    return field


def _run(case, field, order=None, keep=None, times=None):
    """One forward + backward through _HexLookup with a DeterministicSum record -> (features, dL/dpts, dL/dtimes, [plane gradients], det_state)."""
    from emd_amd.hexplane import DeterministicSum, _HexLookup
    dev = field.aabb.device
    p1 = case["pts"].to(dev).requires_grad_(True)
    t1 = (case["t"] if times is None else times).to(dev).requires_grad_(True)
    planes = [p for gp in field.grids for p in gp]
    for p in planes:
        p.grad = None
    rec = DeterministicSum(keep_plane=keep, order=order)
    f1 = _HexLookup.apply(p1, t1, field._aabb_host(), field._res, rec, *planes)
    (f1 * case["gout"].to(dev)).sum().backward()
    return f1.detach(), p1.grad, t1.grad, [None if p.grad is None else p.grad.clone() for p in planes], rec.det_state


def _same_bits(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3]))


def _parity(case, got):
    ref = case["ref"]
    np.testing.assert_allclose(got[0].cpu().numpy(), ref["feat"], rtol=2e-6, atol=1e-7)
    _close(got[1], ref["pts"], "pts")
    _close(got[2], ref["times"], "times")
    for s in range(len(MULTIRES)):
        for p in range(6):
            _close(got[3][6 * s + p], ref["planes"][s][p], f"plane {s} {p}")


def _texels(case, s, p):
    """The texel of every slot e = k N + n of plane (s, p), in numpy from the points: k_hexplane_bwd's arithmetic in fp32.  The box normalisation
    (p - lo) * scale - 1 may or may not be contracted into one fma by the compiler: both roundings are returned (they differ for a point whose
    coordinate sits on a cell boundary to the last bit)."""
    f32 = np.float32
    pts, t, res = case["pts"].numpy(), case["t"].numpy().reshape(-1), _scale_res(s)
    lo, hi = f32(BOUNDS), f32(-BOUNDS)                                    # aabb[0], aabb[1] of HexPlaneField
    scale = f32(2.0) / f32(hi - lo)
    d = (pts - lo).astype(f32)
    q_plain = (d * scale).astype(f32) - f32(1.0)
    q_fma = (d.astype(np.float64) * np.float64(scale) - 1.0).astype(f32)  # (the fp64 product of two fp32 numbers is exact)
    out = []
    for q3 in (q_plain, q_fma):
        q = np.concatenate((q3, t.reshape(-1, 1).astype(f32)), axis=1)

        def axis(k):
            size = res[k]
            v = ((q[:, k] + f32(1.0)).astype(f32) * f32(0.5 * (size - 1))).astype(f32)
            v = np.where(~(v > 0), f32(0.0), np.where(~(v < size - 1), f32(size - 1), v))
            i0 = np.floor(v).astype(np.int64)
            return i0, np.minimum(i0 + 1, size - 1)
        (x0, x1), (y0, y1), W = axis(PAIRS[p][0]), axis(PAIRS[p][1]), res[PAIRS[p][0]]
        out.append(np.concatenate((y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1)))       # taps (x0,y0), (x1,y0), (x0,y1), (x1,y1)
    return out


def _check_lists(case, s, p, state, plane_grad):
    """det_state of kept plane (s, p): the structure of the lists, and plane_grad == the pinned sum of them, bit for bit.  -> run lengths"""
    N, C = case["N"], case["C"]
    rows, keys, slots = state["rows"].cpu().numpy(), state["keys"].cpu().numpy().astype(np.int64), state["slots"].cpu().numpy().astype(np.int64)
    assert int(state["counts"][0]) == 4 * N and rows.shape == (4 * N, C) and len(keys) == len(slots) == 4 * N
    assert (np.diff(keys) >= 0).all()                                      # keys non-decreasing
    assert (np.diff(slots)[np.diff(keys) == 0] > 0).all()                  # slots ascending within a run: ascending (tap, point)
    assert np.array_equal(np.sort(slots), np.arange(4 * N))                # a permutation of the slots
    plain, fma = _texels(case, s, p)
    assert ((keys == plain[slots]) | (keys == fma[slots])).all()           # key[e] = texel of tap e // N of point e % N
    assert np.array_equal(state["raw_keys"].cpu().numpy().astype(np.int64)[slots], keys)
    res = _scale_res(s)
    W, H = res[PAIRS[p][0]], res[PAIRS[p][1]]
    want = np.zeros((W * H, C), np.float32)                                # texels without a contribution keep the caller's zeros
    sg.segsum_reference(keys, slots, rows, C, want)
    got = plane_grad[0].permute(1, 2, 0).reshape(H * W, C).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return sg.run_structure(keys)[1]


KEPT = ((0, 0), (2, 0), (1, 2))          # a coarse spatial plane, the finest spatial one, a time plane


@pytest.mark.parametrize("C", [32, 16])
def test_plane_gradients_are_the_pinned_sums_of_the_calls_own_lists(C):
    dev = torch.device("cuda", 0)
    case = _case(C, "uniform", 30011)
    field = _field(case, dev)
    runs = [_run(case, field, keep=k) for k in KEPT]
    for (s, p), r in zip(KEPT, runs):
        assert r[4] is not None and r[4]["passes"] == (1 if (s, p) != (2, 0) else 2)      # 64 x 48 texels: 12 key bits, two passes
        _check_lists(case, s, p, r[4], r[3][6 * s + p])
    _same_bits(runs[0], runs[1])                                           # which plane is kept (= processed last) changes no bit
    _same_bits(runs[0], runs[2])
    assert _run(case, field)[4] is None                                    # nothing kept: no views


def test_runs_longer_than_two_chunks_occur_same_time():
    """One shared time: on plane (x, t) of scale 0 the 30011 tap-(x0,y0) elements fall on at most 16 texels, so some run is >= 1876 > 2 x 512."""
    dev = torch.device("cuda", 0)
    case = _case(32, "same_time", 30011)
    field = _field(case, dev)
    r = _run(case, field, keep=(0, 2))
    lengths = _check_lists(case, 0, 2, r[4], r[3][2])
    assert lengths.max() > 2 * sg.SEG_CHUNK
    _parity(case, r)


def test_runs_longer_than_two_chunks_occur_outside_points():
    """1100 points beyond the box on every axis: all four taps of each clamp to ONE texel of every spatial plane, a run of >= 4400 over all four taps."""
    dev = torch.device("cuda", 0)
    case = _case(32, "outside", 3100)
    field = _field(case, dev)
    r = _run(case, field, keep=(1, 0))
    lengths = _check_lists(case, 1, 0, r[4], r[3][6])
    keys, slots = r[4]["keys"].cpu().numpy(), r[4]["slots"].cpu().numpy()
    res = _scale_res(1)
    last = res[0] * res[1] - 1
    assert lengths.max() >= 4400 and (keys == last).sum() >= 4400
    assert sorted(set((slots[keys == last] // 3100).tolist())) == [0, 1, 2, 3]          # every tap takes part in that run
    _parity(case, r)


def test_identical_bits_across_runs_streams_and_orders():
    from emd_amd.hexplane import VisitingOrders, morton_order
    dev = torch.device("cuda", 0)
    case = _case(32, "uniform", 30011)
    field = _field(case, dev)
    first = _run(case, field)
    # other work on the device: another field's lookups on a second stream, never waited for until the end
    other_case = _case(16, "clustered", 30011)
    other = _field(other_case, dev, deterministic=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    po, to, go = other_case["pts"].to(dev), other_case["t"].to(dev), other_case["gout"].to(dev)
    for _ in range(3):
        with torch.cuda.stream(side):
            for _ in range(4):
                (other(po, to) * go).sum().backward()
        _same_bits(first, _run(case, field))
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(3)
    p_dev = case["pts"].to(dev)
    orders = [morton_order(p_dev, field.aabb), torch.randperm(case["N"], generator=g).to(torch.int32).to(dev),
              VisitingOrders.build(p_dev, field.aabb, field._res, window=0)]
    assert orders[2].defer_mask == 0b111
    for o in orders:
        _same_bits(first, _run(case, field, order=o))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C", [32, 16, 4])
def test_parity_with_the_oracle(C, layout):
    dev = torch.device("cuda", 0)
    case = _case(C, layout, 30011)
    _parity(case, _run(case, _field(case, dev)))


def test_broadcast_timestamp():
    """A [1, 1] time tensor, as HexPlaneField.get_density passes the base of a broadcast: its gradient is the pinned sum of the per-point column."""
    dev = torch.device("cuda", 0)
    case = _case(32, "same_time", 30011)
    field = _field(case, dev)
    t11 = torch.tensor([[0.21]])
    a, b = _run(case, field, times=t11, keep=(0, 0)), _run(case, field, times=t11, keep=(0, 0))
    assert a[2].shape == (1, 1) and torch.equal(a[2], b[2])
    _same_bits(a, b)
    want = np.asarray([[case["ref"]["times"].astype(np.float64).sum()]])
    _close(a[2], want, "time sum")
    col = a[4]["time_column"].cpu().numpy().reshape(-1, 1)
    pinned = sg.segsum_reference(np.zeros(len(col), np.uint32), np.arange(len(col)), col, 1, np.zeros((1, 1), np.float32))
    assert np.array_equal(a[2].cpu().numpy().view(np.uint32), pinned.view(np.uint32))
    _close(a[1], case["ref"]["pts"], "pts")
    for s in range(len(MULTIRES)):
        for p in range(6):
            _close(a[3][6 * s + p], case["ref"]["planes"][s][p], f"plane {s} {p}")


@pytest.mark.parametrize("N", [1, 255, 512, 513])
def test_edges_of_the_chunk_and_the_block(N):
    dev = torch.device("cuda", 0)
    case = _case(32, "uniform", N)
    field = _field(case, dev)
    a, b = _run(case, field), _run(case, field)
    _parity(case, a)
    _same_bits(a, b)


def test_no_points_no_launch():
    """N = 0 returns before anything is launched or checked for the mode: the pointers below are never dereferenced."""
    import ctypes as C
    from emd_amd import _lib as L
    fake = 1 << 20
    a, g = L.EmdHexArgs(), L.EmdHexGrads()
    a.num_points, a.channels, a.num_scales = 0, 32, 1
    for k in range(4):
        a.res[0][k] = RES[k]
    for p in range(6):
        a.planes[0][p] = g.dL_dplanes[0][p] = fake
    g.dL_dout, g.dL_dpts, g.flags, g.det_keep_plane = fake, fake, L.HEX_FLAG_DETERMINISTIC, 1
    assert L.load().emd_hexplane_backward(C.byref(a), C.byref(g), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()


def test_only_point_gradients_need_no_workspace():
    dev = torch.device("cuda", 0)
    case = _case(32, "uniform", 30011)
    field = _field(case, dev, planes_grad=False)
    p1 = case["pts"].to(dev).requires_grad_(True)
    out = field(p1, case["t"].to(dev))
    (out * case["gout"].to(dev)).sum().backward()
    assert field.det_state is None and all(p.grad is None for p in field.parameters())
    _close(p1.grad, case["ref"]["pts"], "pts")
    full = _run(case, _field(case, dev))
    assert torch.equal(p1.grad, full[1])


def test_captured_step_replays_the_eager_bits():
    from emd_amd.hexplane import DeterministicSum, _HexLookup
    dev = torch.device("cuda", 0)
    case = _case(32, "uniform", 30011)
    field = _field(case, dev)
    eager = _run(case, field)
    pts, t, gout = case["pts"].to(dev).requires_grad_(True), case["t"].to(dev).requires_grad_(True), case["gout"].to(dev)      # static inputs
    planes = [p for gp in field.grids for p in gp]

    def step():
        out = _HexLookup.apply(pts, t, field._aabb_host(), field._res, DeterministicSum(), *planes)
        return (out, *torch.autograd.grad((out * gout).sum(), [pts, t, *planes]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        _same_bits(eager, (res[0], res[1], res[2], list(res[3:])))


def test_default_mode_is_untouched_in_behaviour():
    dev = torch.device("cuda", 0)
    case = _case(32, "uniform", 30011)
    field = _field(case, dev, deterministic=False)
    p1, t1 = case["pts"].to(dev).requires_grad_(True), case["t"].to(dev).requires_grad_(True)
    out = field(p1, t1)
    (out * case["gout"].to(dev)).sum().backward()
    assert field.det_state is None and field._det_record is None           # no record, no workspace
    _parity(case, (out.detach(), p1.grad, t1.grad, [p.grad for gp in field.grids for p in gp]))


def test_through_the_deformation_network():
    """DeformOptions.deterministic reaches the field: the HexPlane parameters' gradients have identical bits across two backward passes.  (Not asserted
    for the other parameters: their kernels keep their atomics)"""
    from emd_amd.deformation import DeformOptions, deform_network
    dev = torch.device("cuda", 0)
    torch.manual_seed(11)
    opt = DeformOptions(deterministic=True, multires=[1, 2, 4],
                        kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32, "resolution": [32, 32, 32, 25]})
    net = deform_network(opt)
    net.deformation_net.set_aabb([40.0, 15.0, 8.0], [-5.0, -15.0, -3.0])
    for n, prm in net.named_parameters():
        if "grid" in n and "aabb" not in n:
            prm.data = torch.rand_like(prm) + 0.3
        elif prm.dim() > 1 and "grid" not in n and "time_offset" not in n:
            prm.data = torch.randn_like(prm) * 0.2
    net = net.to(dev)
    assert net.deformation_net.grid.deterministic is True
    N = 20000
    pt = (torch.rand(N, 3) * torch.tensor([50.0, 34.0, 13.0]) + torch.tensor([-7.0, -17.0, -4.0])).to(dev)
    sc, ro, op, sh, em = (x.to(dev) for x in (torch.randn(N, 3), torch.randn(N, 4), torch.randn(N, 1), torch.randn(N, 16, 3), torch.randn(N, 4) * 0.3))
    times = torch.full((N, 1), 0.42, device=dev)
    weights = [torch.randn_like(x) for x in (pt, sc, ro, op, sh)]
    grids = [prm for n, prm in net.named_parameters() if "grid" in n and "aabb" not in n]
    assert len(grids) == 18
    grads = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        got = net(pt, sc, ro, op, sh, times, em, 12000, 1, 0.1, True)
        sum((o * w).sum() for o, w in zip(got[:5], weights) if o.requires_grad).backward()
        grads.append([prm.grad.clone() for prm in grids])
    assert all(float(g.abs().max()) > 0.0 for g in grads[0])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
