"""-m "not gpu": the deterministic forms of the MLP kernels and of the temporal table's backward as far as they go without a
device -- the symbols, the host-only slab layout against the header's formula, the refusals (all decided before anything is launched), and the
`deterministic` switch from DeformOptions down to mlp.level_mlp and temporal_embed."""
import ctypes as C
import inspect
import os
import types

import pytest
import torch

from emd_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("emd_mlp_det_slab_bytes", "emd_mlp_branch_forward_det", "emd_mlp_branch_backward_det", "emd_mlp_trunk_backward_det", "emd_mlp_det_reduce",
       "emd_temporal_embed_backward_det")
SIZES = (0, 1, 32, 129, 70_001, 2_000_000)
P = 0x7f0000001000          # a stand-in device address (256-byte aligned): the calls below are all refused before anything is launched


def _grid(n, per_cu):
    """mlp_grid of csrc/mlp_kernels.h, restated: ceil(ceil(N / 32) / 4) workgroups, at most 256 per_cu (and one for an empty launch)."""
    wgs = -(-(-(-n // 32)) // 4)
    return min(max(wgs, 1), 256 * per_cu)


def _round256(b):
    return (b + 255) // 256 * 256


def _branch(n=1000, depth=1, out_dim=3):
    b = L.EmdMlpBranch()
    b.num_points, b.depth, b.relu_input, b.out_dim, b.h = n, depth, 1, out_dim, P
    for d in range(depth):
        b.w_hidden[d], b.b_hidden[d] = P, P
    b.w_out, b.b_out, b.out, b.l1_sum = P, P, P, P
    return b


def _branch_grads():
    g = L.EmdMlpBranchGrads()
    g.g_out, g.g_h, g.d_w_out, g.d_b_out = P, P, P, P
    g.d_w_hidden[0], g.d_b_hidden[0] = P, P
    return g


def _trunk(n=1000, ka=128, kb=4):
    t = L.EmdMlpTrunk()
    t.num_points, t.ka, t.kb, t.ld_w, t.col_a, t.col_b = n, ka, kb, ka + 32 + kb, 0, ka + 32
    t.xa, t.xb, t.w, t.b = (P if ka else None), (P if kb else None), P, P
    return t


def _trunk_grads(d_xb=P):
    g = L.EmdMlpTrunkGrads()
    g.num_gh, g.g_h[0], g.d_xa, g.d_xb, g.d_w, g.d_b = 1, P, P, d_xb, P, P
    return g


def test_new_symbols_are_declared_listed_and_exported_and_the_abi_is_31():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "emd_raster.h")).read()
    for name in NEW:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name) and f" {name}(" in header, name
    assert lib.emd_abi_version() == 31 == L.ABI_VERSION
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert f"`{name}`" in integration, name


@pytest.mark.parametrize("n", SIZES)
def test_slab_layout_is_host_only_and_equals_the_header_formula(n):
    def expect(groups, pitches):
        offs, off = [], 0
        for p in pitches:
            offs.append(off)
            off += _round256(4 * groups * p)
        return dict(groups=groups, pitch=list(pitches), offset=offs, bytes=off)
    empty = lambda k: dict(groups=0, pitch=None, offset=[0] * k, bytes=0)

    def same(got, want):
        if n == 0:          # nothing is launched: no slots, no bytes
            assert got["groups"] == 0 and got["bytes"] == 0 and got["offset"] == want["offset"]
        else:
            assert got == want
    # a head's backward (one workgroup per CU), one and two hidden layers, a narrow and a two-tile output
    for depth, out_dim in ((1, 3), (1, 48), (2, 3), (2, 64), (1, 1)):
        hid2 = (4096, 64) if depth == 2 else (0, 0)
        want = expect(_grid(n, 1), (4096, 64) + hid2 + (64 * out_dim, out_dim)) if n else empty(6)
        same(L.mlp_det_layout(L.MLP_DET_BRANCH_BWD, _branch(n, depth, out_dim), _branch_grads()), want)
        # the L1 forward: two workgroups per CU for a one-hidden-layer head of one output tile, else one
        per_cu = 2 if depth == 1 and out_dim <= 32 else 1
        same(L.mlp_det_layout(L.MLP_DET_BRANCH_FWD, _branch(n, depth, out_dim)), expect(_grid(n, per_cu), (1,)) if n else empty(1))
    # the trunk: with HexPlane features one workgroup per CU; the embedding alone: its own kernel (one) when xb / d_xb are whole 16-byte rows, else the
    # MFMA form with no xa tile (two)
    same(L.mlp_det_layout(L.MLP_DET_TRUNK_BWD, _trunk(n, 128, 4), _trunk_grads()), expect(_grid(n, 1), (64 * 128, 64 * 4, 64)) if n else empty(3))
    same(L.mlp_det_layout(L.MLP_DET_TRUNK_BWD, _trunk(n, 72, 5), _trunk_grads()), expect(_grid(n, 1), (64 * 72, 64 * 5, 64)) if n else empty(3))
    same(L.mlp_det_layout(L.MLP_DET_TRUNK_BWD, _trunk(n, 0, 4), _trunk_grads()), expect(_grid(n, 1), (0, 256, 64)) if n else empty(3))
    same(L.mlp_det_layout(L.MLP_DET_TRUNK_BWD, _trunk(n, 0, 4), _trunk_grads(d_xb=P + 4)), expect(_grid(n, 2), (0, 256, 64)) if n else empty(3))
    same(L.mlp_det_layout(L.MLP_DET_TRUNK_BWD, _trunk(n, 0, 5), _trunk_grads()), expect(_grid(n, 2), (0, 320, 64)) if n else empty(3))


def test_the_grid_restatement_at_the_sizes_of_the_issue():
    assert [_grid(n, 1) for n in SIZES] == [1, 1, 1, 2, 256, 256]
    assert [_grid(n, 2) for n in SIZES] == [1, 1, 1, 2, 512, 512]
    assert _grid(70_001, 1) < -(-(-(-70_001 // 32)) // 4)          # 547 workgroups' worth of tiles on 256: the persistent stride is in play


def test_bad_kinds_and_shapes_have_no_layout():
    lib = L.load()
    b = _branch()
    assert lib.emd_mlp_det_slab_bytes(7, C.byref(b), None, None) == 0
    b.depth = 3
    assert lib.emd_mlp_det_slab_bytes(L.MLP_DET_BRANCH_BWD, C.byref(b), None, None) == 0
    assert lib.emd_mlp_det_slab_bytes(L.MLP_DET_TRUNK_BWD, None, None, None) == 0


def test_slab_refusals_come_before_any_launch():
    lib = L.load()
    b, g, t, tg = _branch(), _branch_grads(), _trunk(), _trunk_grads()
    need = L.mlp_det_layout(L.MLP_DET_BRANCH_BWD, b, g)["bytes"]
    assert need > 0
    for slab, nbytes in ((None, need), (P, need - 1), (P + 16, need), (P + 128, need)):           # missing, short, misaligned (256 B)
        assert lib.emd_mlp_branch_backward_det(C.byref(b), C.byref(g), slab, nbytes, None) == L.EMD_ERR_WORKSPACE, (slab, nbytes)
        assert b"slab" in lib.emd_last_error()
    need = L.mlp_det_layout(L.MLP_DET_TRUNK_BWD, t, tg)["bytes"]
    for slab, nbytes in ((None, need), (P, need - 1), (P + 64, need)):
        assert lib.emd_mlp_trunk_backward_det(C.byref(t), C.byref(tg), slab, nbytes, None) == L.EMD_ERR_WORKSPACE
    need = L.mlp_det_layout(L.MLP_DET_BRANCH_FWD, b)["bytes"]
    for slab, nbytes in ((None, need), (P, need - 1), (P + 4, need)):
        assert lib.emd_mlp_branch_forward_det(C.byref(b), slab, nbytes, None) == L.EMD_ERR_WORKSPACE
    # nothing to do: no slab needed, nothing launched
    b0, t0 = _branch(0), _trunk(0)
    assert lib.emd_mlp_branch_backward_det(C.byref(b0), C.byref(g), None, 0, None) == L.EMD_OK
    assert lib.emd_mlp_trunk_backward_det(C.byref(t0), C.byref(tg), None, 0, None) == L.EMD_OK
    assert lib.emd_mlp_branch_forward_det(C.byref(b0), None, 0, None) == L.EMD_OK


def test_every_refusal_of_the_default_entries_applies():
    lib = L.load()
    big = 1 << 30

    def both(name, *structs):
        """the default entry and its deterministic form (given a slab that would do) refuse the same call"""
        args = [C.byref(s) for s in structs]
        assert getattr(lib, name)(*args, None) == L.EMD_ERR_INVALID, name
        assert getattr(lib, name + "_det")(*args, P, big, None) == L.EMD_ERR_INVALID, name + "_det"
    b = _branch(); b.depth = 3
    both("emd_mlp_branch_backward", b, _branch_grads())
    both("emd_mlp_branch_forward", b)
    b = _branch(); b.w_out = None
    both("emd_mlp_branch_backward", b, _branch_grads())
    b = _branch(); b.out = None
    both("emd_mlp_branch_forward", b)
    g = _branch_grads(); g.g_h = None
    both("emd_mlp_branch_backward", _branch(), g)
    g = _branch_grads(); g.g_h = P + 4                                   # 16-byte alignment of dL/dh
    both("emd_mlp_branch_backward", _branch(), g)
    g = _branch_grads(); g.g_h_in = P                                    # the chained dL/dh: one hidden layer only
    b2 = _branch(depth=2)
    both("emd_mlp_branch_backward", b2, g)
    g = _branch_grads(); g.l1_grad = P                                   # ... needs the forward's outputs
    both("emd_mlp_branch_backward", _branch(), g)
    b = _branch(depth=2); b.xb, b.w_in, b.b_in, b.kb_in, b.ld_w_in = P, P, P, 4, 64          # recomputed h: one hidden layer only
    both("emd_mlp_branch_backward", b, _branch_grads())
    t = _trunk(); t.ka = 130
    both("emd_mlp_trunk_backward", t, _trunk_grads())
    tg = _trunk_grads(); tg.num_gh = 0
    both("emd_mlp_trunk_backward", _trunk(), tg)
    tg = _trunk_grads(); tg.num_gh = 7
    both("emd_mlp_trunk_backward", _trunk(), tg)
    tg = _trunk_grads(); tg.d_xa = P + 8
    both("emd_mlp_trunk_backward", _trunk(), tg)
    # the forward form is for the regulariser: without l1_sum it is refused
    b = _branch(); b.l1_sum = None
    assert lib.emd_mlp_branch_forward_det(C.byref(b), P, big, None) == L.EMD_ERR_INVALID
    assert lib.emd_mlp_branch_backward_det(None, None, P, big, None) == L.EMD_ERR_INVALID


def test_reduce_and_temporal_refusals():
    lib = L.load()
    jobs = (L.EmdMlpDetJob * 2)()
    for j in jobs:
        j.slab, j.dst, j.groups, j.pitch, j.rows, j.cols, j.ld, j.col0, j.scale = P, P, 8, 4096, 64, 64, 64, 0, 1.0
    assert lib.emd_mlp_det_reduce(None, 1, None) == L.EMD_ERR_INVALID
    assert lib.emd_mlp_det_reduce(jobs, 0, None) == L.EMD_ERR_INVALID
    assert lib.emd_mlp_det_reduce(jobs, L.MLP_DET_MAX_JOBS + 1, None) == L.EMD_ERR_INVALID
    for field, bad in (("slab", None), ("dst", None), ("groups", 0), ("pitch", 4095), ("rows", 0), ("ld", 63), ("col0", -1)):
        keep = getattr(jobs[1], field)
        setattr(jobs[1], field, bad)
        assert lib.emd_mlp_det_reduce(jobs, 2, None) == L.EMD_ERR_INVALID, field
        setattr(jobs[1], field, keep)
    te = lib.emd_temporal_embed_backward_det
    assert te(None, 1, 150, 32, 30, P, P, P, P, None, None) == L.EMD_ERR_INVALID
    assert te(P, 1, 150, 32, 0, P, P, P, P, None, None) == L.EMD_ERR_INVALID
    assert te(P, 1, 150, 32, 30, P, None, P, P, None, None) == L.EMD_ERR_INVALID
    assert te(P, 3, 150, 32, 30, P, P, P, P, None, None) == L.EMD_ERR_WORKSPACE          # dL/dt of several tables needs one partial per table


def test_the_switch_is_an_argument_and_defaults_to_off():
    from emd_amd import deformation, mlp
    assert inspect.signature(mlp.level_mlp).parameters["deterministic"].default is False
    assert inspect.signature(deformation.temporal_embed).parameters["deterministic"].default is False
    assert deformation.DeformOptions().deterministic is False
    assert mlp.DET_TRACE is None


def _record(monkeypatch):
    """level_mlp and temporal_embed replaced by recorders that return tensors of the right shapes (nothing runs on a device)."""
    from emd_amd import deformation, mlp
    seen = dict(mlp=[], te=[])

    def fake_level(xa, xb, w0, b_eff, col_a, col_b, branches, l1_heads=(), deterministic=False):
        seen["mlp"].append(deterministic)
        n = xb.shape[0]
        return [torch.zeros(n, wo.shape[0]) for _, _, (wo, _) in branches] + [torch.zeros(()) for _ in l1_heads]

    def fake_te(weight, t, k, deterministic=False):
        seen["te"].append(deterministic)
        return torch.zeros(weight.shape[-1])
    monkeypatch.setattr(mlp, "level_mlp", fake_level)
    monkeypatch.setattr(deformation, "temporal_embed", fake_te)
    return seen


@pytest.mark.parametrize("flag", [False, True])
def test_deform_options_deterministic_reaches_the_mlp_and_the_temporal_table(flag, monkeypatch):
    from emd_amd.deformation import DeformOptions, deform_network
    seen = _record(monkeypatch)
    kw = dict(deterministic=True) if flag else {}
    net = deform_network(DeformOptions(multires=[1, 2], no_coarse_hexplane_features=True,
                                       kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 16, "resolution": [16, 16, 16, 8]}, **kw))
    n = 40
    pts = types.SimpleNamespace(device=types.SimpleNamespace(type="cuda"), shape=(n, 3))          # (only its device is asked: neither level looks a point up)
    time, emb = torch.full((n, 1), 0.3), torch.zeros(n, 4)
    for coarse in (True, False):
        out = net.deformation_net._level_fused(pts, time, emb, coarse, None, 30, l1_keys=("dx",))
        assert out is not None and out["dx"].shape == (n, 3) and "dx_abs_mean" in out
    assert seen["mlp"] == [flag, flag] and seen["te"] == [flag, flag]


def test_a_level_outside_the_fused_kernels_raises_under_the_flag(monkeypatch):
    from emd_amd.deformation import DeformOptions, deform_network
    _record(monkeypatch)
    small = {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 16, "resolution": [16, 16, 16, 8]}
    n = 8
    pts, time, emb = torch.zeros(n, 3), torch.full((n, 1), 0.3), torch.zeros(n, 4)
    for kw in (dict(fused_mlp=False), dict(net_width=128), dict(defor_depth=2)):
        net = deform_network(DeformOptions(deterministic=True, multires=[1, 2], kplanes_config=small, **kw))
        with pytest.raises(NotImplementedError, match="deterministic"):
            net.deformation_net(pts, time, emb, is_coarse=False)
        # without the flag the same configuration is simply not the fused kernels' business
        net.args.deterministic = False
        assert net.deformation_net._level_fused(pts, time, emb, False, None, 30) is None
