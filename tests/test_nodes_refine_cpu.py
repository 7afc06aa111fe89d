"""No GPU: the torch restatement of the actor classes' refinement event (tests/nodes_refine_ref.py) against typed-out cases; its float32 and float64
decisions agree on every input the GPU tests use, with the margins that make the GPU comparison exact asserted row by row; and the argument checks
of emd_refine_nodes_decide / emd_refine_nodes_index, which refuse a bad call before anything is launched (so they run without a device)."""
import ctypes as C
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nodes_refine_ref as R  # noqa: E402


def _typed(means, normals, half=(1.0, 1.0, 1.0), log_scale=None, opacity=4.0, **cfg):
    """n rows of ONE actor with identity rotations, std 0.5 on every axis (well above the split size), hot gradients"""
    n = len(means)
    case = types.SimpleNamespace(num_samples=len(normals), num_actors=1, cfg=R.default_cfg(**cfg))
    case.ids = torch.zeros(n, dtype=torch.long)
    case.instances_size = torch.tensor([half]) * 2
    case.means = torch.tensor(means, dtype=torch.float32)
    case.log_scales = torch.log(torch.full((n, 3), 0.5)) if log_scale is None else torch.tensor(log_scale, dtype=torch.float32)
    case.quats = torch.tensor([[2.0, 0.0, 0.0, 0.0]] * n)                          # not normalised: the reference normalises
    case.opacity = torch.full((n,), float(opacity))
    case.grad_norm, case.vis_counts, case.max_2Dsize = torch.full((n,), 1e-2), torch.ones(n), torch.zeros(n)
    case.normals = torch.tensor(normals, dtype=torch.float32).reshape(len(normals), n, 3)
    case.moment = torch.arange(3.0 * n).reshape(n, 3) + 1
    return case


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_original_is_culled_but_its_sample_survives(dtype):
    # mean x = 1.2 outside the half extent 1; replica 0 is drawn back to 1.2 - 0.5 = 0.7, replica 1 pushed out to 1.7
    out = R.refine(_typed([[1.2, 0.0, 0.0]], [[[-1.0, 0.0, 0.0]], [[1.0, 0.0, 0.0]]]), dtype)
    assert out.counts == (0, 0, 1, [1, 0])
    assert out.src.tolist() == [0] and out.kind.tolist() == [2] and out.ids.tolist() == [0]
    torch.testing.assert_close(out.means.float(), torch.tensor([[0.7, 0.0, 0.0]]), rtol=0, atol=1e-6)
    torch.testing.assert_close(out.log_scales.float(), torch.log(torch.full((1, 3), 0.5 / 1.6)), rtol=0, atol=1e-6)
    assert out.moment.abs().max() == 0                                               # a new row starts without moments


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_only_replica_one_survives(dtype):
    # two rows inside at y = 0.9 / -0.9 (half extent 1): replica 0 leaves through the near face, replica 1 lands at 0.4 / -0.4
    case = _typed([[0.0, 0.9, 0.0], [0.0, -0.9, 0.0]], [[[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]], [[0.0, -1.0, 0.0], [0.0, 1.0, 0.0]]])
    out = R.refine(case, dtype)
    assert out.counts == (2, 0, 2, [0, 2])
    assert out.src.tolist() == [0, 1, 0, 1] and out.kind.tolist() == [0, 0, 3, 3]
    torch.testing.assert_close(out.means.float(), torch.tensor([[0.0, 0.9, 0.0], [0.0, -0.9, 0.0], [0.0, 0.4, 0.0], [0.0, -0.4, 0.0]]), rtol=0, atol=1e-6)
    assert torch.equal(out.moment[:2], case.moment) and out.moment[2:].abs().max() == 0
    # without the box test both replicas stay, replica-major
    out = R.refine(_typed([[0.0, 0.9, 0.0], [0.0, -0.9, 0.0]], case.normals.tolist(), cull_out_of_bound=False), dtype)
    assert out.kind.tolist() == [0, 0, 2, 2, 3, 3] and out.counts == (2, 0, 2, [2, 2])


def test_duplicate_after_the_reduction_order_and_grouping():
    """Row 0 (actor 1): scale 0.06, just above the split size 0.05: split AND duplicated (0.06 / 1.6 is below).  Row 1 (actor 0): scale 0.01, duplicated.
    Row 2 (actor 1): cold, stays.  Row 3 (actor 0): transparent, culled with everything it would have produced."""
    ls = torch.log(torch.tensor([[0.06] * 3, [0.01] * 3, [0.06] * 3, [0.06] * 3])).tolist()
    case = _typed([[0.1, 0.0, 0.0]] * 4, [[[0.5, 0.0, 0.0]] * 4], log_scale=ls)
    case.ids = torch.tensor([1, 0, 1, 0])
    case.num_actors, case.instances_size = 2, torch.ones(2, 3) * 2
    case.grad_norm[2] = 1e-6
    case.opacity[3] = -12.0
    out = R.refine(case)
    assert out.src.tolist() == [0, 1, 2, 0, 0, 1] and out.kind.tolist() == [0, 0, 0, 2, 1, 1] and out.counts == (3, 2, 2, [1])
    torch.testing.assert_close(out.log_scales[4], torch.log(torch.tensor([0.06 / 1.6] * 3)))       # the duplicate of a split row is reduced too
    out = R.refine(case, group=True)
    assert out.ids.tolist() == [0, 0, 1, 1, 1, 1] and out.src.tolist() == [1, 1, 0, 2, 0, 0] and out.kind.tolist() == [0, 1, 0, 0, 2, 1]


def test_float32_and_float64_decisions_agree_on_every_gpu_input_with_margins():
    rows = 0
    for name, case in R.gpu_cases():
        a, b = R.refine(case, torch.float32), R.refine(case, torch.float64)
        assert a.counts == b.counts and torch.equal(a.src, b.src) and torch.equal(a.kind, b.kind) and torch.equal(a.ids, b.ids), name
        # no row excluded: every row of the grown arrays keeps 16 rounding bounds from its box face, every threshold quantity its relative margin
        assert bool((b.box_distance >= R.BOX_FACTOR * b.box_bound).all()), name
        for what, v in b.margins.items():
            assert bool((v >= R.REL_MARGIN).all()), (name, what)
        assert not bool(R.hanging_rows(b).any()), name
        rows += b.grown_src.numel()
        if name == "box":                                        # the case is not vacuous: the box test decides, replica by replica
            no_box = R.refine(types.SimpleNamespace(**{**vars(case), "cfg": {**case.cfg, "cull_out_of_bound": False}}))
            assert all(x < y for x, y in zip(a.counts[3], no_box.counts[3])) and a.counts[0] < no_box.counts[0] and len(set(a.counts[3])) > 1
            assert a.counts[2] > 500 and a.counts[1] > 20
    assert rows > 30000


# ---- the C entry points refuse a bad call before any launch ----------------------------------------------------------------------------------------
def _lib():
    from emd_amd import _lib as L
    return L, L.load()


def test_new_symbols_are_present_and_the_abi_number_stays():
    L, lib = _lib()
    for name in ("emd_refine_nodes_decide", "emd_refine_nodes_index", "emd_refine_nodes_index_workspace"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.emd_abi_version() == 31 and L.ABI_VERSION == 31
    assert C.sizeof(L.EmdRefineNodesArgs) == C.sizeof(L.EmdRefineArgs) + 64
    for k, (name, _) in enumerate(L.EmdRefineArgs._fields_):                           # the shared fields sit where EmdRefineArgs has them
        assert L.EmdRefineNodesArgs._fields_[k][0] == name and getattr(L.EmdRefineNodesArgs, name).offset == getattr(L.EmdRefineArgs, name).offset
    assert lib.emd_refine_nodes_index_workspace(0) == 0 and lib.emd_refine_nodes_index_workspace(-3) == 0
    assert lib.emd_refine_nodes_index_workspace(5000) >= 4 * (6 * 5000 + 512 * 3)


_BUF = []


def _pointer():
    """Every call below is refused before a launch, so the address is never used.  Where a device is present it is still a real 256 KiB device
    buffer, larger than any array of these 300-point calls: a check that let a call through would fail this test, not fault the device."""
    if not torch.cuda.is_available():
        return 0x1000
    if not _BUF:
        _BUF.append(torch.zeros(1 << 16, dtype=torch.int32, device="cuda"))
    return _BUF[0].data_ptr()


def _args(L, **over):
    a = L.EmdRefineNodesArgs()
    a.num_points, a.num_actors, a.num_samples, a.do_densify, a.do_cull, a.cull_out_of_bound, a.group_by_actor = 300, 4, 2, 1, 1, 1, 1
    fake = _pointer()
    for f in ("scaling", "opacity", "grad_norm", "vis_counts", "max_2Dsize", "means", "rotation", "ids", "instances_size"):
        setattr(a, f, fake)
    for k, v in over.items():
        setattr(a, k, v)
    return a, fake


BAD_FIELDS = [dict(num_actors=0), dict(num_actors=-1), dict(num_actors=65537), dict(num_samples=0), dict(num_samples=14), dict(num_samples=-2),
              dict(num_points=-1), dict(cull_out_of_bound=2), dict(group_by_actor=-1)]


@pytest.mark.parametrize("bad", BAD_FIELDS, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_out_of_range_fields_are_refused(bad):
    L, lib = _lib()
    a, p = _args(L, **bad)
    assert lib.emd_refine_nodes_decide(C.byref(a), p, p, None) == L.EMD_ERR_INVALID
    assert lib.emd_refine_nodes_index(C.byref(a), 10, p, p, p, p, p, p, p, p, p, 1 << 18, None) == L.EMD_ERR_INVALID
    assert lib.emd_last_error()


def test_null_pointers_and_negative_sizes_are_refused():
    L, lib = _lib()
    a, p = _args(L)
    assert lib.emd_refine_nodes_decide(None, p, p, None) == L.EMD_ERR_INVALID
    assert lib.emd_refine_nodes_decide(C.byref(a), None, p, None) == L.EMD_ERR_INVALID
    assert lib.emd_refine_nodes_decide(C.byref(a), p, None, None) == L.EMD_ERR_INVALID
    for field in ("scaling", "ids", "opacity", "grad_norm", "vis_counts", "max_2Dsize", "means", "rotation", "instances_size"):
        b, _ = _args(L, use_split_screen=1, **{field: None})
        assert lib.emd_refine_nodes_decide(C.byref(b), p, p, None) == L.EMD_ERR_INVALID, field
    index = lambda a_, num_out, *ptrs, ws=p, nbytes=1 << 18: lib.emd_refine_nodes_index(a_, num_out, *ptrs, ws, nbytes, None)
    ok = [p] * 8                                                 # code, offsets, totals, src, kind, ids_out, segment_start, split_rank
    assert index(None, 10, *ok) == L.EMD_ERR_INVALID
    assert index(C.byref(a), -1, *ok) == L.EMD_ERR_INVALID
    for k in range(7):                                           # split_rank alone may be NULL
        ptrs = list(ok)
        ptrs[k] = None
        assert index(C.byref(a), 10, *ptrs) == L.EMD_ERR_INVALID, k
    b, _ = _args(L, ids=None)
    assert index(C.byref(b), 10, *ok) == L.EMD_ERR_INVALID
    assert index(C.byref(a), 10, *ok, ws=None) == L.EMD_ERR_INVALID                      # a grouped index needs its scratch ...
    assert index(C.byref(a), 10, *ok, nbytes=int(lib.emd_refine_nodes_index_workspace(10)) - 1) == L.EMD_ERR_INVALID          # ... all of it
