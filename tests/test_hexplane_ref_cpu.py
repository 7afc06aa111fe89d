"""CPU: the float64 HexPlane reference (tests/hexplane_ref.py) and its bounds, proved before any GPU run: against the grid_sample oracle run in float64
(continuous inputs and every lattice case of tests/test_hexplane_edges_gpu.py: same node, face and clip conventions), against the golden vectors of
the reference's own HexPlaneField, with the float32 oracle as an independent fp32 implementation under the same bounds, the exactness of the lattice,
and the sharpness of the plane bound (a lost tap would show)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import hexplane_oracle as ho
from tests import hexplane_ref as R
from tests.test_hexplane_edges_gpu import CASE_KEYS

G = os.path.join(os.path.dirname(__file__), "golden")


def _oracle(pts, times, lo, hi, planes, gout, dtype):
    """oracle/hexplane_oracle.py (grid_sample, autograd) in `dtype` on the float32 inputs: numpy feat, dpts, dtimes [N], plane gradients (flat list)."""
    N = pts.shape[0]
    p = torch.from_numpy(np.asarray(pts, np.float32)).to(dtype).requires_grad_(True)
    t = torch.from_numpy(np.asarray(times, np.float32).reshape(-1, 1)).to(dtype).requires_grad_(True)
    aabb = torch.tensor([list(lo), list(hi)], dtype=torch.float32).to(dtype)
    pl = [[torch.from_numpy(x).to(dtype).requires_grad_(True) for x in row] for row in planes]
    f = ho.hexplane_features(p, t.expand(N, 1) if t.shape[0] == 1 else t, aabb, pl)
    (f * torch.from_numpy(np.asarray(gout, np.float32)).to(dtype)).sum().backward()
    return f.detach().numpy(), p.grad.numpy(), t.grad.numpy().reshape(-1), [x.grad.numpy() for row in pl for x in row]


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max()) / max(float(np.abs(b).max()), 1e-300)


def _equals_oracle64(lo, hi, res, pts, times, planes, gout, tol=1e-12):
    ref = R.hexplane_ref(pts, times, lo, hi, res, planes, gout)
    f, dp, dt, gp = _oracle(pts, times, lo, hi, planes, gout, torch.float64)
    assert _rel(f, ref.feat) <= tol and _rel(dp, ref.dpts) <= tol
    assert _rel(dt, ref.dtimes if dt.size == ref.N else np.array([ref.dtime_sum])) <= tol          # (one timestamp: the oracle returns the sum)
    for s in range(ref.S):
        for p in range(6):
            assert _rel(gp[s * 6 + p], ref.planes[s][p].g) <= tol, (s, p)
    # the magnitudes dominate the values, and equal them where nothing is signed
    assert (ref.feat_mag >= np.abs(ref.feat)).all() and (ref.dpts_mag >= np.abs(ref.dpts) * (1 - 1e-12)).all()
    return ref


@pytest.mark.parametrize("N,C,res,multires", [(20000, 32, [16, 16, 16, 8], [1, 2, 4]), (5000, 16, [9, 7, 5, 3], [1, 2]), (3000, 4, [4, 4, 4, 2], [1])])
def test_reference_equals_the_float64_oracle_on_continuous_inputs(N, C, res, multires):
    """the shapes of test_hexplane_vs_oracle, points outside the box and times beyond +-1"""
    g = torch.Generator().manual_seed(N)
    scales = [[r * m for r in res[:3]] + res[3:] for m in multires]
    planes = [[(torch.rand(1, C, r[b], r[a], generator=g) + 0.3).numpy() for a, b in R.PAIRS] for r in scales]
    pts = (torch.rand(N, 3, generator=g) * 3.6 - 1.8).numpy()
    t = (torch.rand(N, 1, generator=g) * 2.2 - 1.1).numpy()
    gout = torch.randn(N, C * len(multires), generator=g).numpy()
    _equals_oracle64((1.6, 1.6, 1.6), (-1.6, -1.6, -1.6), scales, pts, t, planes, gout)


def test_reference_within_the_golden_tolerance():
    g = np.load(os.path.join(G, "s3g_hexplane.npz"))
    S = len(g["multires"])
    planes = [[g[f"plane_{s}_{p}"] for p in range(6)] for s in range(S)]
    res = [[planes[s][0].shape[3], planes[s][0].shape[2], planes[s][1].shape[2], planes[s][2].shape[2]] for s in range(S)]
    ref = R.hexplane_ref(g["pts"], g["times"], g["aabb"][0], g["aabb"][1], res, planes, g["gout"])
    # the tolerances test_hexplane_matches_reference_golden holds the kernels to (the golden vectors are fp32 results themselves: the float64 values
    # differ from them by their own rounding, which in dL/dpts, a sum of differences, exceeds what two fp32 runs of the same arithmetic differ by)
    def close(a, b, what, rel=1e-4):
        assert np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-30), (what, np.abs(a - b).max(), np.abs(b).max())
    np.testing.assert_allclose(ref.feat, g["feat"], rtol=2e-6, atol=1e-7)
    close(ref.dpts, g["g_pts"], "pts")
    for s in range(S):
        for p in range(6):
            close(ref.planes[s][p].g, g[f"g_plane_{s}_{p}"], f"plane {s} {p}")
    # (continuous coordinates: their own rounding in q moves a weight by more than the counted bounds allow, which is why those are for lattice inputs)


@functools.lru_cache(maxsize=None)
def _case_and_ref(layout, C, signed, bcast):
    case = R.make_case(layout, C, signed)
    times = case.times[:1] if bcast else case.times
    return case, times, R.hexplane_ref(case.pts, times, case.lo, case.hi, case.res, case.planes, case.gout, terms=True)


@pytest.mark.parametrize("key", CASE_KEYS, ids=lambda k: "-".join(str(x) for x in k))
def test_lattice_case(key):
    """Every (layout, channels, signed planes, broadcast timestamp) the GPU file runs: the lattice is exact; the reference equals the float64 oracle; the
    float32 oracle stays inside the bounds and meets the exact-zero conditions; the plane bound would show a lost tap."""
    layout, C, signed, bcast = key
    case, times, ref = _case_and_ref(*key)
    assert R.lattice_is_exact(case)
    if case.N == 0:
        return
    _equals_oracle64(case.lo, case.hi, case.res, case.pts, times, case.planes, case.gout)
    f, dp, dt, gp = _oracle(case.pts, times, case.lo, case.hi, case.planes, case.gout, torch.float32)
    R.check_against(ref, f, dp, dt, [x for x in gp], what=key)
    # sharpness: in every touched entry the largest |term| exceeds twice the entry's bound, and in 90 % of them the median |term| does
    touched = med_ok = 0
    for s in range(ref.S):
        for p in range(6):
            r = ref.planes[s][p]
            idx, val = r.terms
            o = np.lexsort((val, idx))
            idx, val = idx[o], val[o]
            start = np.flatnonzero(np.r_[True, idx[1:] != idx[:-1]])
            cnt = np.diff(np.r_[start, idx.size])
            entry = idx[start]
            assert np.array_equal(cnt, r.m.reshape(-1)[entry]) and entry.size == int((r.m > 0).sum())
            bound = R.bound_plane(r.mag, r.m).reshape(-1)[entry]
            assert (val[start + cnt - 1] > 2 * bound).all(), (key, s, p)
            touched += entry.size
            med_ok += int((val[start + (cnt - 1) // 2] > 2 * bound).sum())           # (the lower median: no laxer than the median)
    assert med_ok >= 0.9 * touched, (key, med_ok, touched)


def test_signed_zero_time_is_the_same_case_to_the_reference():
    a, b = R.make_case("zero_uniform", 16), R.make_case("zero_signed", 16)
    assert np.array_equal(a.pts, b.pts) and np.signbit(b.times).sum() == 1 and not np.signbit(a.times).any() and np.array_equal(a.times, b.times)


def test_layouts_place_what_they_name():
    """The seams the layouts are for, recomputed from their taps: nodes, faces and a resolution of one; runs longer than the windows they cross."""
    c = R.make_case("nodes_inverted", 4)
    q = R.normalise(c.pts, c.times, c.lo, c.hi)
    for a in range(4):
        assert {-1.0, 1.0} <= set(q[:, a]) and (np.abs(q[:, a]) > 1).any() and (q[:, a] == 1 - 1 / 1024).any() and (q[:, a] == -1 - 1 / 1024).any()
    i0, i1, f, ds = R.axis_taps(q[:, 0], 17)
    assert ((f == 0) & (ds > 0)).sum() >= 15 and ((i1 == i0) & (ds == 0)).any()                  # interior nodes; the collapsed footprint at the face
    assert any(r[3] == 1 for r in c.res) and any(6 in [x - 1 for x in r] for r in c.res)
    assert tuple(c.lo) > tuple(c.hi) and R.make_case("nodes_forward", 4).lo < R.make_case("nodes_forward", 4).hi

    def cells(layout, axis, size, block=slice(0, 256)):
        cc = R.make_case(layout, 16)
        return R.axis_taps(R.normalise(cc.pts, cc.times, cc.lo, cc.hi)[block, axis], size)[0]
    for a, name in enumerate(("window_x", "window_y", "window_z")):
        x0 = cells(name, a, 17)
        assert x0.max() - x0.min() + 1 == 10 and (x0 == x0.min() + 6).any() and (x0 > x0.min() + 6).any()     # inside, astride (x0 the last column), outside
        assert all(np.ptp(cells(name, b, 17)) <= 1 for b in range(3) if b != a)
    assert all(np.ptp(cells("time_uniform", a, 33)) + 1 > 19 for a in range(3))
    assert np.unique(cells("time_mixed", 3, 5)).size >= 3 and np.ptp(cells("time_mixed", 0, 33)) + 1 > 9
    assert all(np.ptp(cells("deferred_time", a, 129)) + 1 > 68 for a in range(3))
    assert all(np.ptp(cells("plane_window", a, 33)) + 1 >= 20 for a in range(3))
    x0 = cells("plane_window", 0, 33)
    assert (x0 == x0.min() + 11).any()
    assert all(np.ptp(cells("piled", a, 17)) == 0 for a in range(4) if a < 3) and np.unique(R.make_case("piled", 16).times).size == 1
