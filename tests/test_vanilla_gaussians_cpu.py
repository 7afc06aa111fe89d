"""-m "not gpu": the contracts of csrc/vanilla.hip (tests/vanilla_ref.py) in fp32 torch on the CPU against their fp64 form under the criteria the
GPU tests use -- the bar comes from the formula and the number format, not from a kernel --, the conditions the seeded cases promise, and what
of the five entry points runs without a device: argument validation, the exported symbols (the struct sizes: tests/test_abi.py).

For orientation (not asserted): fp32 torch on the CPU at N = 3000 gave 1.2e-7 on the terms, 0.002 of the element bound on dL/dlog_scales and 0.38
on dL/dopacity_logits (the printed lines show the figures of each case)."""
import ctypes as C

import pytest
import torch

from emd_amd import _lib as L
from tests import vanilla_ref as R
from tests.sh_ref import CLAMP_MARGIN

F32 = torch.float32


# ---- the formulas at the kernels' precision ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DICT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_dictionary_fp32_formulation_meets_the_criterion(case):
    c, ref, got = R.dict_case(*case), R.dict_reference(*case), R.dictionary(R.dict_case(*case), F32)
    for k in R.OUTPUTS + R.GRADS:
        R.compare(got[k], ref[k], f"{case} {k}")
    K = c["K"]
    assert float(ref["d_features_rest"][:, K - 1:].abs().sum()) == 0.0                     # the rows the degree does not use


@pytest.mark.parametrize("case", R.DICT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_dictionary_cases_keep_clear_of_the_clamp_edges_and_fill_every_region(case):
    c, ref = R.dict_case(*case), R.dict_reference(*case)
    assert c["K"] <= c["M"] and c["features_rest"].shape == (c["N"], c["M"] - 1, 3)
    if not c["sh_mode"]:
        assert ref["pre"] is None
        return
    v = ref["pre"] + 0.5
    assert float(v.abs().min()) >= CLAMP_MARGIN and float((v - 1).abs().min()) >= CLAMP_MARGIN
    assert c["nudged"] <= max(1, c["N"] // 100)                                            # the nudge moves a handful of entries, not the case
    if c["N"] >= 255 and c["n"] >= 1:
        for name, region in (("below 0", v < 0), ("inside", (v > 0) & (v < 1)), ("above 1", v > 1)):
            share = float(region.double().mean())
            print(f"{case} {name}: {100 * share:.1f} %")
            assert share >= 0.02, (case, name, share)


@pytest.mark.parametrize("wname", list(R.WEIGHT_SETS))
@pytest.mark.parametrize("name", R.REG_CASES)
def test_regulation_fp32_formulation_meets_the_criteria(name, wname):
    ref, got = R.reg_reference(name, wname), R.regulation(R.reg_case(name), R.weights(wname), F32)
    R.scalar_criterion(got["terms"], ref["terms"], f"{name} {wname}")
    R.compare(got["d_log_scales"], ref["d_log_scales"], f"{name} {wname} d_log_scales")
    # the closed form the contract states for dL/dopacity_logits, in fp32, against autograd in fp64: on every case.  Autograd in fp32 as well where
    # no logit sits next to the clip (torch's sigmoid backward forms o * (1 - o) from a rounded o: 3 % off at |a| = 13.7, the edges cases)
    c, w = R.reg_case(name), R.weights(wname)
    R.compare(R.sparse_gradient(c, w, F32), ref["d_opacity_logits"], f"{name} {wname} d_opacity_logits (closed form)")
    R.compare(R.sparse_gradient(c, w), ref["d_opacity_logits"], f"{name} {wname} d_opacity_logits (closed form, fp64)")
    if not name.startswith("edges"):
        R.compare(got["d_opacity_logits"], ref["d_opacity_logits"], f"{name} {wname} d_opacity_logits")


@pytest.mark.parametrize("name", R.REG_CASES)
def test_regulation_cases_keep_clear_of_the_kinks(name):
    c = R.reg_case(name)
    s = torch.exp(c["log_scales"].double())
    ratio = s.amax(-1) / s.amin(-1)
    assert float((ratio - R.RATIO).abs().min()) >= R.GAP
    assert float((s.amin(-1) - 30.0).abs().min()) >= R.GAP
    above = float((ratio > R.RATIO).double().mean())
    print(f"{name}: {100 * above:.1f} % of the ratios above {R.RATIO}")
    if name.startswith("n"):
        assert 0.08 <= above <= 0.3
        assert 0.4 <= float((c["radii"] > 0).double().mean()) <= 0.8
    if name == "ties":
        l = c["log_scales"]
        eq = lambda a, b: l[:, a] == l[:, b]
        assert int((eq(0, 1) & eq(1, 2)).sum()) == 2
        two = (eq(0, 1) | eq(1, 2) | eq(0, 2)) & ~(eq(0, 1) & eq(1, 2))
        hi = l.max(-1).values
        two_max = two & ((l == hi[:, None]).sum(-1) == 2)
        assert int((two_max & (ratio > R.RATIO)).sum()) == 3 and int((two_max & (ratio < R.RATIO)).sum()) == 3      # every position of the odd column
        assert int((two & ~two_max & (ratio > R.RATIO)).sum()) == 3 and int((two & ~two_max & (ratio < R.RATIO)).sum()) == 3
    if name.startswith("edges"):
        a = c["opacity_logits"].double().reshape(-1)
        o = torch.sigmoid(a)
        inside = (o >= 1e-6) & (o <= 1 - 1e-6)
        assert int(inside.sum()) == 9 and int((~inside).sum()) == 12                       # -13.7, 0, 13.7 inside; +-13.9, +-20 outside
        assert int((c["radii"] > 0).sum()) == dict(edges_all=c["N"], edges_none=0, edges_one=1)[name]


def test_tie_rules_of_the_reference_are_the_stated_ones():
    """Equal largest (smallest) columns share the sharp-shape gradient; the lowest index takes flatten's and max_s_square's."""
    c = dict(log_scales=torch.tensor([[1.5, 1.5, -2.0], [0.5, -3.0, -3.0], [0.25, 0.25, 0.25]]), opacity_logits=torch.zeros(3, 1), radii=torch.ones(3, dtype=torch.int32))
    one = (1.0, 1.0, 1.0, 1.0)
    g = R.regulation(c, dict(w_sharp=1.0, w_flatten=0.0, w_sparse=0.0, w_max_s_square=0.0, max_gauss_ratio=10.0), upstream=one)["d_log_scales"]
    r0, r1 = float(torch.exp(torch.tensor(3.5, dtype=torch.float64))) / 3, float(torch.exp(torch.tensor(3.5, dtype=torch.float64))) / 3
    assert torch.allclose(g[0], torch.tensor([r0 / 2, r0 / 2, -r0], dtype=torch.float64)) and torch.allclose(g[1], torch.tensor([r1, -r1 / 2, -r1 / 2], dtype=torch.float64))
    assert float(g[2].abs().max()) == 0.0
    g = R.regulation(c, dict(w_sharp=0.0, w_flatten=1.0, w_sparse=0.0, w_max_s_square=1.0, max_gauss_ratio=10.0), upstream=one)["d_log_scales"]
    e = lambda x: float(torch.exp(torch.tensor(x, dtype=torch.float64)))
    want = torch.tensor([[2 * e(3.0) / 3, 0.0, e(-2.0) / 3], [2 * e(1.0) / 3, e(-3.0) / 3, 0.0], [2 * e(0.5) / 3 + e(0.25) / 3, 0.0, 0.0]], dtype=torch.float64)
    assert torch.allclose(g, want, rtol=1e-12, atol=0)


# ---- the host side of the five entry points ---------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("emd_vanilla_forward", "emd_vanilla_backward", "emd_vanilla_reg_workspace_size", "emd_vanilla_reg_forward", "emd_vanilla_reg_backward")


def test_symbols_are_exported_and_abi_number_stays():
    lib = L.load()
    for n in NEW_SYMBOLS:
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n), n
    assert lib.emd_abi_version() == 31 == L.ABI_VERSION


def _good_args():
    """Arguments the forward would launch with (fake, aligned, non-NULL device addresses: nothing is launched by a refused call)."""
    a = L.EmdVanillaArgs()
    a.num_points, a.sh_coeffs, a.degree, a.sh_mode = 0, 16, 3, 1            # (an empty class: even an accepted call launches nothing)
    for i, (name, _) in enumerate(L.EmdVanillaArgs._fields_[4:16]):
        setattr(a, name, 0x10000 + 0x1000 * i)
    return a


@pytest.mark.parametrize("entry", ["emd_vanilla_forward", "emd_vanilla_backward"])
def test_dictionary_entry_points_refuse_bad_arguments_before_any_launch(entry):
    lib = L.load()
    fn = getattr(lib, entry)

    def refused(a, word):
        assert fn(C.byref(a), None) == L.EMD_ERR_INVALID
        assert word.encode() in lib.emd_last_error(), (word, lib.emd_last_error())
    assert fn(None, None) == L.EMD_ERR_INVALID
    a = _good_args(); a.num_points = -1; refused(a, "negative")
    for n in (2 ** 31 - 1, 2 ** 31 - 256):                                   # block * 256 + lane of the last block would wrap an int
        a = _good_args(); a.num_points = n; refused(a, "above")
    a = _good_args(); a.degree = -1; refused(a, "degree")
    a = _good_args(); a.degree = 4; refused(a, "degree")
    a = _good_args(); a.degree, a.sh_coeffs = 2, 8; refused(a, "coefficient rows")
    a = _good_args(); a.sh_coeffs = 17; refused(a, "sh_coeffs")
    a = _good_args(); a.sh_mode = 2; refused(a, "sh_mode")
    for name in ("means", "log_scales", "quats", "opacity_logits", "features_dc", "features_rest", "camera_center"):
        a = _good_args(); setattr(a, name, None); refused(a, "null")
    for name in ("means", "log_scales", "quats", "opacity_logits", "features_dc", "features_rest"):
        a = _good_args(); setattr(a, name, getattr(a, name) + 4); refused(a, "aligned")
    a = _good_args(); a.camera_center += 2; refused(a, "camera_center")
    if entry == "emd_vanilla_forward":
        for name in ("opacities", "scales", "quats_out", "rgbs"):
            a = _good_args(); setattr(a, name, None); refused(a, "null output")
            a = _good_args(); setattr(a, name, getattr(a, name) + 8); refused(a, "aligned")
    else:
        a = _good_args(); a.g_rgbs, a.clamp_mask = 0x90000, None; refused(a, "clamp_mask")
        a = _good_args(); a.dL_dfeatures_rest = 0x90004; refused(a, "aligned")
        # the upstream gradients are views at any row offset (a consumer's torch.cat): dword alignment, except g_quats, which is read as float4
        a = _good_args(); a.g_opacities, a.g_scales, a.g_rgbs = 0x90004, 0xa0008, 0xb000c
        assert fn(C.byref(a), None) == L.EMD_OK
        a = _good_args(); a.g_quats = 0x90004; refused(a, "aligned")
        for name in ("g_opacities", "g_scales", "g_rgbs"):
            a = _good_args(); setattr(a, name, 0x90002); refused(a, "aligned")
    # dc mode reads neither the camera nor features_rest; features_rest may be absent at degree 0; an empty class launches nothing
    assert fn(C.byref(_good_args()), None) == L.EMD_OK
    a = _good_args(); a.sh_mode, a.degree, a.camera_center, a.features_rest = 0, 0, None, None
    assert fn(C.byref(a), None) == L.EMD_OK
    a = _good_args(); a.degree, a.sh_coeffs, a.features_rest = 0, 1, None
    assert fn(C.byref(a), None) == L.EMD_OK


def test_regulariser_entry_points_refuse_bad_arguments_before_any_launch():
    lib = L.load()
    size = lib.emd_vanilla_reg_workspace_size
    assert size(0) == 0 and size(-5) == 0
    chunks = lambda n: (n + L.VANILLA_REG_CHUNK - 1) // L.VANILLA_REG_CHUNK
    for n in (1, L.VANILLA_REG_CHUNK, L.VANILLA_REG_CHUNK + 1, 300_000):
        assert size(n) == (16 + 36 * chunks(n) + 7) // 8 * 8                               # the head, four doubles and a count per chunk
    assert b"num_points" in lib.emd_last_error()
    assert size(2 ** 31 - 1) == 0 and size(2 ** 31 - 256) == 0 and size(2 ** 31 - 257) > 0

    def good():
        a = L.EmdVanillaRegArgs()
        a.num_points, a.log_scales, a.terms, a.g, a.dL_dlog_scales = 100, 0x10000, 0x20000, 0x30000, 0x40000
        a.w_sharp, a.max_gauss_ratio = 1.0, 10.0
        return a
    ws, nbytes = 0x50000, size(100)
    fwd = lambda a, w=ws, b=nbytes: lib.emd_vanilla_reg_forward(C.byref(a), w, b, None)
    bwd = lambda a, w=ws, b=nbytes: lib.emd_vanilla_reg_backward(C.byref(a), w, b, None)
    assert lib.emd_vanilla_reg_forward(None, ws, nbytes, None) == L.EMD_ERR_INVALID and lib.emd_vanilla_reg_backward(None, ws, nbytes, None) == L.EMD_ERR_INVALID
    for call in (fwd, bwd):
        a = good(); a.num_points = 0
        assert call(a) == L.EMD_ERR_INVALID and b"num_points" in lib.emd_last_error()
        a = good(); a.num_points = 2 ** 31 - 256
        assert call(a) == L.EMD_ERR_INVALID and b"above" in lib.emd_last_error()
        a = good(); a.log_scales = None
        assert call(a) == L.EMD_ERR_INVALID and b"log_scales" in lib.emd_last_error()
        a = good(); a.log_scales += 2
        assert call(a) == L.EMD_ERR_INVALID and b"aligned" in lib.emd_last_error()
        a = good(); a.max_gauss_ratio = 0.0
        assert call(a) == L.EMD_ERR_INVALID and b"max_gauss_ratio" in lib.emd_last_error()
        assert call(good(), None) == L.EMD_ERR_WORKSPACE and call(good(), ws + 4) == L.EMD_ERR_WORKSPACE and call(good(), ws, nbytes - 1) == L.EMD_ERR_WORKSPACE
    a = good(); a.terms = None
    assert fwd(a) == L.EMD_ERR_INVALID and b"terms" in lib.emd_last_error()
    a = good(); a.g = None
    assert bwd(a) == L.EMD_ERR_INVALID
    a = good(); a.dL_dlog_scales = None
    assert bwd(a) == L.EMD_ERR_INVALID
    a = good(); a.dL_dopacity_logits = 0x60002
    assert bwd(a) == L.EMD_ERR_INVALID and b"aligned" in lib.emd_last_error()


def test_python_entry_points_refuse_cpu_tensors_and_ball_gaussians():
    from emd_amd import nodes, vanilla
    z = torch.zeros
    with pytest.raises(L.EmdError, match="no CPU path"):
        nodes.vanilla_gaussians(z(4, 3), z(4, 4), z(4, 1), z(4, 3), z(4, 3), z(4, 15, 3), z(3))
    with pytest.raises(L.EmdError, match="no CPU path"):
        vanilla.gaussian_regulation(z(4, 3), w_flatten=1.0)
    node = vanilla.VanillaGaussians("Background", dict(sh_degree=3, ball_gaussians=True), reg=dict(flatten=dict(w=1.0)), device="cpu")
    assert node.cur_radii is None
    with pytest.raises(NotImplementedError, match="ball"):
        node.get_gaussians(None)
    with pytest.raises(NotImplementedError, match="ball"):
        node.compute_reg_loss()
    assert vanilla.VanillaGaussians("Background", dict(sh_degree=3), device="cpu").compute_reg_loss() == {}
