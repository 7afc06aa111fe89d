"""-m gpu: every HexPlane kernel against the float64 reference (tests/hexplane_ref.py) on exact-lattice inputs placed on the seams of the kernels --
grid nodes, the faces of the box and beyond, times on nodes and at +-1, a resolution of one, the edges of the aggregating kernel's 7 x 7 spatial and 19-cell
/ 9 x 2 / 68-cell time windows, of the per-plane pass's 12 x 12 window, piled points, the tiles of the forward and backward kernels, an empty input --
through `_HexLookup.apply`, entry by entry under the counted bounds of the reference (no entry left out), with the two exact-zero conditions, and the
forward bit-identical across visiting orders.  Each test prints its worst error / bound per quantity (DESIGN.md section 8.17 has the table)."""
import functools

import numpy as np
import pytest
import torch

from tests import hexplane_ref as R

pytestmark = pytest.mark.gpu


def _arms():
    """(layout, channels, signed planes, arm, time gradient, null outputs).  arm: direct (no order: k_hexplane_fwd2 / fwd4 + k_hexplane_bwd), perm (direct with a
    permutation), agg (an int32 order: k_hexplane_bwd_agg), defer_all / defer_some (VisitingOrders with a defer_mask: + k_hexplane_bwd_plane), det
    (DeterministicSum).  Time gradient: 0 not requested, 1 per point, 2 one broadcast timestamp [1, 1] (time_tables in the forward at 16 / 32 channels).
    null: "" | "planes" (no plane requires a gradient) | "pts" (the points do not)."""
    A = []
    nodes = "nodes_inverted"
    A += [(nodes, C, False, "direct", 1, "") for C in (1, 2, 4, 8, 16, 32, 64)]
    A += [(nodes, 8, False, "perm", 1, ""), (nodes, 8, False, "direct", 2, ""), (nodes, 64, False, "direct", 2, ""), (nodes, 1, False, "direct", 0, "")]
    A += [(nodes, 8, True, "direct", 1, ""), (nodes, 32, True, "agg", 1, ""), (nodes, 16, True, "det", 1, ""), (nodes, 16, True, "defer_all", 2, "")]
    for null in ("planes", "pts"):
        A += [(nodes, 8, False, "direct", 1, null), (nodes, 32, False, "agg", 1, null), (nodes, 16, False, "det", 1, null), (nodes, 16, False, "agg", 2, null)]
    for layout in R.LAYOUTS:
        A += [(layout, C, False, "agg", dt, "") for C in (16, 32) for dt in (0, 1, 2)]
        A += [(layout, C, False, "det", 1, "") for C in (4, 16, 32)]
    A += [(nodes, 16, False, "det", 2, ""), (nodes, 4, False, "det", 0, ""), ("nodes_forward", 8, False, "direct", 1, ""), ("nodes_forward", 64, False, "direct", 1, "")]
    for layout in (nodes, "nodes_forward", "window_x", "time_mixed", "piled"):
        A += [(layout, C, False, arm, 1, "") for C in (16, 32) for arm in ("defer_all", "defer_some")]
    A += [("deferred_time", 16, False, "defer_all", dt, "") for dt in (0, 1, 2)] + [("deferred_time", 32, False, "defer_all", 1, "")]
    A += [("plane_window", C, False, arm, dt, "") for C in (16, 32) for arm, dt in (("defer_all", 1), ("defer_some", 1), ("defer_some", 2))]
    # tile seams: fwd4's 128-point chunks and its chunk -> XCD remap (1025: nine chunks on a grid of sixteen), fwd2's 64-point tiles, the direct backward's
    # EMD_BLOCK / C points per block, the aggregating backward's 256-point blocks, and the empty input
    A += [(f"tile_{n}", 32, False, "direct", 1, "") for n in (1, 127, 128, 129, 1025)] + [(f"tile_{n}", 16, False, "direct", 2, "") for n in (129, 1025)]
    A += [(f"tile_{n}", C, False, "direct", 1, "") for n in (63, 64, 65) for C in (8, 64)]
    A += [("tile_5", 64, False, "direct", 1, "")] + [(f"tile_{n}", 1, False, "direct", dt, "") for n in (255, 256, 257) for dt in (1, 2)]
    A += [(f"tile_{n}", C, False, "agg", dt, "") for n in (255, 256, 257) for C, dt in ((32, 1), (16, 2), (32, 0))]
    A += [(f"tile_{n}", 32, False, "defer_all", 1, "") for n in (255, 257)] + [(f"tile_{n}", 16, False, "det", 2, "") for n in (255, 257)]
    A += [("tile_0", C, False, arm, dt, "") for C, arm, dt in ((8, "direct", 1), (32, "direct", 1), (32, "agg", 1), (16, "agg", 2), (32, "defer_all", 1), (16, "det", 1))]
    assert len(set(A)) == len(A)
    return A


ARMS = _arms()
# what the reference is computed for, once each: (layout, channels, signed, one broadcast timestamp); tests/test_hexplane_ref_cpu.py proves every one
CASE_KEYS = sorted({(a[0], a[1], a[2], a[4] == 2 and a[0] not in ("tile_0", "tile_1")) for a in ARMS})


@functools.lru_cache(maxsize=None)
def _case_and_ref(layout, C, signed, bcast):
    case = R.make_case(layout, C, signed)
    return case, R.hexplane_ref(case.pts, case.times[:1] if bcast else case.times, case.lo, case.hi, case.res, case.planes, case.gout)


def _inverse(o):
    return torch.empty_like(o).scatter_(0, o.long(), torch.arange(o.numel(), dtype=torch.int32, device=o.device))


def _order(case, arm, dev):
    """What travels in `_HexLookup.apply`'s order position.  Layouts whose seam is a BLOCK of points as laid out are visited in identity order, in 3-D and in
    the planes; the others along the Morton curve, with arbitrary permutations as plane orders (built by hand, as `plane_pass_random_orders` does)."""
    from emd_amd.hexplane import DeterministicSum, VisitingOrders, morton_order
    N, C = case.N, case.C
    g = torch.Generator().manual_seed(N + C)
    if arm == "direct":
        return None
    if arm == "perm" or (arm == "det" and C not in (16, 32)):
        return torch.randperm(N, generator=g).to(torch.int32).to(dev)
    if case.identity:
        order = torch.arange(N, dtype=torch.int32, device=dev)
    else:
        order = morton_order(torch.from_numpy(case.pts), torch.tensor([list(case.lo), list(case.hi)])).to(dev)
    assert sorted(order.cpu().tolist()) == list(range(N))
    if arm == "agg":
        return order
    if arm == "det":
        return DeterministicSum(order=order)
    o2 = [order.clone() if case.identity else torch.randperm(N, generator=g).to(torch.int32).to(dev) for _ in range(3)]
    mask = (1 << case.S) - 1
    if arm == "defer_some":
        mask = 0b101 & mask if case.S == 3 else 0b01
    return VisitingOrders(order, o2, [_inverse(o) for o in o2], mask)


@pytest.mark.parametrize("arm", ARMS, ids=lambda a: "-".join(str(x) for x in a if x != ""))
def test_hexplane_edges(arm):
    from emd_amd.hexplane import DeterministicSum, _HexLookup
    layout, C, signed, kind, dt, null = arm
    dev = torch.device("cuda", 0)
    case, ref = _case_and_ref(layout, C, signed, dt == 2 and layout not in ("tile_0", "tile_1"))
    N, S = case.N, case.S
    pts = torch.from_numpy(case.pts).to(dev).requires_grad_(null != "pts")
    times = torch.from_numpy(case.times[:1] if (dt == 2 and N > 1) else case.times).to(dev).requires_grad_(dt != 0)
    planes = [torch.from_numpy(p).to(dev).requires_grad_(null != "planes") for row in case.planes for p in row]
    gout = torch.from_numpy(case.gout).to(dev)
    aabb6, order = [*case.lo, *case.hi], _order(case, kind, dev)
    if kind == "det":
        order = order if isinstance(order, DeterministicSum) else DeterministicSum(order=order)
    feat = _HexLookup.apply(pts, times, aabb6, case.res, order, *planes)
    assert feat.shape == (N, S * C) and feat.dtype == torch.float32
    (feat * gout).sum().backward()
    torch.cuda.synchronize()
    if kind != "direct":
        # the forward's arithmetic per point does not depend on the order it visits the points in
        with torch.no_grad():
            plain = _HexLookup.apply(pts.detach(), times.detach(), aabb6, case.res, None, *[p.detach() for p in planes])
        assert torch.equal(plain, feat.detach())
    assert (pts.grad is None) == (null == "pts") and (times.grad is None) == (dt == 0) and all((p.grad is None) == (null == "planes") for p in planes)
    assert pts.grad is None or pts.grad.shape == (N, 3)
    assert times.grad is None or times.grad.shape == times.shape
    assert all(p.grad is None or p.grad.shape == p.shape for p in planes)
    if N == 0:
        assert all(p.grad is None or not p.grad.any() for p in planes)
    worst = R.check_against(ref, feat.detach().cpu().numpy(), None if pts.grad is None else pts.grad.cpu().numpy(),
                            None if times.grad is None else times.grad.cpu().numpy(),
                            None if null == "planes" else [p.grad.cpu().numpy() for p in planes], what=arm)
    print("hexplane-edges", "-".join(str(x) for x in arm if x != ""), " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))


def test_refused_configurations_say_why():
    """What `check_hex` and the backward refuse, with their messages: channel counts that are no power of two or above 64, a resolution below one, the
    deterministic mode above 32 channels."""
    from emd_amd import _lib as L
    from emd_amd.hexplane import DeterministicSum, _HexLookup
    dev = torch.device("cuda", 0)

    def lookup(C, res, order=None):
        pts = torch.zeros(4, 3, device=dev, requires_grad=True)
        planes = [torch.ones(1, C, max(res[b], 1), max(res[a], 1), device=dev, requires_grad=True) for a, b in R.PAIRS]
        out = _HexLookup.apply(pts, torch.zeros(4, 1, device=dev), [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], [res], order, *planes)
        out.sum().backward()
    for C in (3, 128):
        with pytest.raises(L.EmdError, match="channels must be a power of two <= 64"):
            lookup(C, [3, 3, 3, 2])
    with pytest.raises(L.EmdError, match="bad resolution"):
        lookup(8, [3, 0, 3, 2])
    with pytest.raises(L.EmdError, match="hexplane_det_workspace_size: bad argument .need num_points >= 0 and 1 <= channels <= 32"):
        lookup(64, [3, 3, 3, 2], DeterministicSum())
