"""-m "not gpu": the image tail of an OmniRe step (emd_amd.trainer_loss, csrc/trainer_loss.hip) without a GPU -- the inputs of the GPU tests
validated (the fp32 torch formulation meets the criterion against the fp64 restatement on every case, so a failure on the GPU is the kernel's),
closed forms of the restatement, and the host layer: exported symbols, ABI, argument validation, the options that are not built and the refusal
of CPU tensors.  (The struct's layout and the constants: tests/test_abi.py.)"""
import ctypes as C
import math

import pytest
import torch

from emd_amd import _lib as L
from emd_amd import trainer_loss as TL
from tests import trainer_loss_ref as R


# ---- the reference and the cases -------------------------------------------------------------------------

def _fp32_meets(name, cfg):
    R.criterion(R.run(R.case(name), cfg, torch.float32, "cpu"), R.reference(name, cfg), cfg, f"{name} fp32 torch")


@pytest.mark.parametrize("mask_type", ["bce", "safe_bce"])
@pytest.mark.parametrize("name", R.SMOOTH_CASES)
def test_fp32_torch_formulation_meets_the_criterion(name, mask_type):
    _fp32_meets(name, R.config(mask_type=mask_type))
    _fp32_meets(name, R.config(mask_type=mask_type, w_ssim=0.0))           # the colour gradient without SSIM: the element-wise rule


@pytest.mark.parametrize("term", list(R.ONLY))
def test_fp32_torch_formulation_meets_the_criterion_on_the_edges_term_by_term(term):
    _fp32_meets("edges", R.only(term))


@pytest.mark.parametrize("opt", R.DEPTH_OPTIONS, ids=lambda o: f"{o['depth_type']}-n{int(o['normalize'])}-i{int(o['inverse'])}")
def test_fp32_torch_formulation_meets_the_criterion_on_every_depth_option(opt):
    _fp32_meets("12x13", R.config(**opt))


def test_cases_have_the_shapes_and_values_the_gpu_tests_rely_on():
    assert (R.CHUNK, R.TILE) == (L.TRAINER_LOSS_CHUNK, L.TRAINER_SSIM_TILE)
    shape = lambda n: tuple(R.case(n)["d"].shape)
    assert shape("11x11") == (11, 11) and shape("12x13") == (12, 13) and (3 * 13 * 4) % 16 != 0
    H, W = shape("tiles")
    # the SSIM map is [H-10] rows of 3 (W-10) interleaved floats, tiled TILE x TILE: one row and one float above whole tiles
    assert (H - 10) % R.TILE == 1 and (3 * (W - 10)) % R.TILE == 1 and H - 10 > R.TILE and 3 * (W - 10) > R.TILE
    assert -(-(H * W) // R.CHUNK) >= 3
    assert -(-(70 * 531) // R.CHUNK) >= 3 and shape("wide") == (70, 531)
    for name in R.CASES:
        c = R.case(name)
        H, W = c["d"].shape
        assert c["x"].shape == c["y"].shape == (H, W, 3) and all(c[k].shape == (H, W) for k in "osdl") and all(v.dtype == torch.float32 for v in c.values())
        assert set(c["s"].unique().tolist()) <= {0.0, 1.0}
    hit = lambda c: (c["s"] == 0) & (c["l"] > 0.01) & (c["l"] < 80.0) & (c["d"] > 1e-4)
    assert int(hit(R.case("empty_hits")).sum()) == 0
    for name in R.SMOOTH_CASES:
        c = R.case(name)
        if name != "empty_hits":
            assert int(hit(c).sum()) > 0 and int((~hit(c)).sum()) > 0
        # at least 1e-3 from every kink: |x - y|; the safe-BCE and entropy clips; the hit thresholds; the smoothness pairs
        assert float((c["x"] - c["y"]).abs().min()) >= 1e-3
        assert all(float((c["o"] - k).abs().min()) >= 1e-3 for k in (0.0, 1e-6, 0.1, 0.9, 1 - 1e-6, 1.0))
        lz = c["l"][c["l"] != 0]
        assert lz.numel() == 0 or (float((lz - 0.01).abs().min()) >= 1e-3 and float((lz - 80.0).abs().min()) >= 1e-3)
        assert float(c["d"].min()) >= 1.0
        assert float((c["d"][:, :-1] - c["d"][:, 1:]).abs().min()) >= 1e-3 and float((c["d"][:-1] - c["d"][1:]).abs().min()) >= 1e-3
    e = R.case("edges")
    assert int((e["x"] == e["y"]).all(-1).sum()) >= 13 * 16 // 5
    assert int((e["d"][:, :-1] == e["d"][:, 1:]).sum()) > 20 and int((e["d"][:-1] == e["d"][1:]).sum()) > 20
    for o in (0.0, 1e-7, 0.05, 0.95, 1.0):
        for s in (0.0, 1.0):
            assert int(((e["o"] == torch.tensor(o, dtype=torch.float32)) & (e["s"] == s)).sum()) > 0, (o, s)
    assert set(torch.tensor([0.0, 0.0101, 0.0099, 79.99, 80.01, 30.0]).tolist()) == set(e["l"].unique().tolist())


def test_depth_options_keep_the_error_away_from_its_kinks():
    """The hit pixels of the 12x13 case: d and l at least 0.1 apart (the sign of z = d' - l'), and ||z| - 1| (smooth-L1's beta) at least 1e-3 under
    every option, with pixels on both sides of beta where the option reaches it."""
    c = {k: v.double() for k, v in R.case("12x13").items()}
    v = (c["s"] == 0) & (c["l"] > 0.01) & (c["l"] < 80.0)
    assert float((c["d"][v] - c["l"][v]).abs().min()) >= 0.1
    z0 = (c["d"][v] - c["l"][v]).abs()
    assert int((z0 < 1).sum()) > 0 and int((z0 > 1).sum()) > 0
    for normalize in (False, True):
        for inverse in (False, True):
            a, b = c["d"][v], c["l"][v]
            if normalize:
                a, b = a / 80.0, b / 80.0
            if inverse:
                a, b = 1 / (a + 1e-5), 1 / (b + 1e-5)
            z = (a - b).abs()
            assert float((z - 1).abs().min()) >= 1e-3, (normalize, inverse, float((z - 1).abs().min()))


def test_restatement_closed_forms():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(14, 17, 3, generator=g, dtype=torch.float64)
    m = R.ssim_map(x, x)
    assert m.shape == (3, 4, 7) and float((m - 1).abs().max()) < 1e-12                      # SSIM(x, x) = 1, on the valid window only
    assert abs(float(R.gaussian_window(torch.float64, "cpu").sum()) - 1) < 1e-15
    y = torch.rand(9, 8, 3, generator=g, dtype=torch.float64)
    assert float(R.smoothness_loss(torch.full((9, 8), 3.25, dtype=torch.float64), y)) == 0.0   # constant depth
    assert abs(float(R.entropy_loss(torch.full((4, 5), math.exp(-1), dtype=torch.float64))) - math.exp(-1)) < 1e-15
    # safe-BCE: the value is the clipped one, the gradient is not zero at the clip
    o = torch.tensor([0.0, 0.05, 0.5, 1.0], dtype=torch.float64, requires_grad=True)
    v = R._SafeBCE.apply(o, torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float64), 0.1)
    assert torch.allclose(v, torch.tensor([-math.log(0.1), -math.log(0.1), -math.log(0.5), -math.log(0.1)], dtype=torch.float64))
    v.sum().backward()
    assert torch.allclose(o.grad, torch.tensor([-10.0, -10.0, 2.0, 10.0], dtype=torch.float64))
    # the depth term over an empty hit set
    z = torch.zeros(3, 4, dtype=torch.float64)
    assert float(R.depth_loss(z + 5, z, z + 1, "l1", False, False, 80.0)) == 0.0


# ---- host layer ------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("emd_affine_workspace_size", "emd_affine_forward", "emd_affine_backward", "emd_trainer_loss_workspace_size", "emd_trainer_loss")


def test_new_symbols_exported_and_abi_unchanged():
    lib = L.load()
    for n in NEW_SYMBOLS:
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n)
    assert lib.emd_abi_version() == L.ABI_VERSION == 31


FAKE = 0x1000        # a non-null, 16-byte aligned pointer value: every call below is refused on the host, before anything is launched or read


def _args(H=12, W=13, **over):
    a = L.EmdTrainerLossArgs()
    a.height, a.width = H, W
    for k in ("rgb", "gt_rgb", "opacity", "sky_mask", "depth", "lidar_depth", "losses", "dL_drgb", "dL_dopacity", "dL_ddepth"):
        setattr(a, k, FAKE)
    a.w_rgb, a.w_ssim, a.w_mask, a.safe_limit, a.w_depth, a.upper_bound, a.w_entropy, a.w_smooth = 0.8, 0.2, 0.05, 0.1, 0.1, 80.0, 0.03, 0.02
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_workspace_size_is_host_only_and_counts_chunks_and_tiles():
    lib = L.load()
    size = lambda *a, **k: lib.emd_trainer_loss_workspace_size(C.byref(_args(*a, **k)))
    cd = lambda a, b: -(-a // b)
    expect = lambda H, W: 8 * 8 * cd(H * W, R.CHUNK) + 8 * cd(H - 10, R.TILE) * cd(3 * (W - 10), R.TILE) + 16 + 4 * 3 * (H - 10) * 3 * (W - 10)
    for H, W in ((11, 11), (12, 13), (43, 53), (1066, 1600)):
        assert size(H, W) == expect(H, W)
    assert size(5, 7, w_ssim=0.0) == 8 * 8 + 16                                         # no window fits: the point-wise partials alone
    assert size(10, 20) == 0 and size(20, 10) == 0 and size(0, 5) == 0 and size(1 << 20, 4) == 0          # what the call refuses
    assert lib.emd_trainer_loss_workspace_size(None) == 0
    assert lib.emd_affine_workspace_size(1) == 96 and lib.emd_affine_workspace_size(R.CHUNK + 1) == 192 and lib.emd_affine_workspace_size(0) == 0


def test_argument_validation_reports_errors():
    lib = L.load()
    bad = lambda rc, word, code=L.EMD_ERR_INVALID: rc == code and word in lib.emd_last_error()
    call = lambda a, ws=FAKE, n=1 << 30: lib.emd_trainer_loss(C.byref(a), ws, n, None)
    assert bad(lib.emd_trainer_loss(None, FAKE, 1 << 30, None), b"null args")
    assert bad(call(_args(0, 13)), b"bad size") and bad(call(_args(12, 40000)), b"bad size")
    assert bad(call(_args(10, 13)), b"SSIM window needs 11 x 11") and bad(call(_args(12, 10)), b"SSIM window needs 11 x 11")
    assert bad(call(_args(1, 13, w_ssim=0.0)), b"smoothness term needs 2 x 2")
    assert bad(call(_args(w_mask=float("nan"))), b"not finite") and bad(call(_args(w_depth=float("inf"))), b"not finite")
    assert bad(call(_args(mask_type=2)), b"bad mask_type") and bad(call(_args(depth_type=3)), b"bad depth_type")
    assert bad(call(_args(mask_type=L.TL_MASK_SAFE_BCE, safe_limit=0.5)), b"safe_limit") and bad(call(_args(mask_type=L.TL_MASK_SAFE_BCE, safe_limit=0.0)), b"safe_limit")
    assert bad(call(_args(upper_bound=0.01)), b"upper_bound")
    for k in ("rgb", "gt_rgb", "losses"):
        assert bad(call(_args(**{k: None})), b"null rgb / gt_rgb / losses")
    assert bad(call(_args(opacity=None)), b"dL_dopacity without opacity") and bad(call(_args(depth=None)), b"dL_ddepth without depth")
    assert bad(call(_args(rgb=FAKE + 2)), b"4-byte aligned") and bad(call(_args(dL_ddepth=FAKE + 1)), b"4-byte aligned")
    need = lib.emd_trainer_loss_workspace_size(C.byref(_args()))
    assert bad(call(_args(), None), b"workspace", L.EMD_ERR_WORKSPACE) and bad(call(_args(), FAKE, need - 1), b"workspace", L.EMD_ERR_WORKSPACE)
    assert bad(call(_args(), FAKE + 4), b"workspace", L.EMD_ERR_WORKSPACE)
    # the affine entry points
    assert bad(lib.emd_affine_forward(0, FAKE, FAKE, FAKE, None), b"bad pixel count")
    assert bad(lib.emd_affine_forward(5, FAKE, None, FAKE, None), b"null or misaligned") and bad(lib.emd_affine_forward(5, FAKE + 2, FAKE, FAKE, None), b"null or misaligned")
    assert bad(lib.emd_affine_backward(5, FAKE, FAKE, FAKE, None, None, FAKE, 1 << 20, None), b"no output asked for")
    assert bad(lib.emd_affine_backward(5, None, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 20, None), b"dL_daffine without rgb")
    assert bad(lib.emd_affine_backward(5, FAKE, FAKE, FAKE, FAKE, FAKE, None, 0, None), b"workspace", L.EMD_ERR_WORKSPACE)
    assert bad(lib.emd_affine_backward(5, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 95, None), b"workspace", L.EMD_ERR_WORKSPACE)


def test_options_that_are_not_built_raise():
    c = R.case("12x13")
    with pytest.raises(NotImplementedError, match="depth_error_percentile"):
        TL.trainer_losses(c["x"], c["y"], depth_error_percentile=0.95)
    with pytest.raises(NotImplementedError, match="pixel_affine"):
        TL.apply_affine(c["x"], torch.eye(3, 4), pixel_affine=True)
    with pytest.raises(NotImplementedError, match="pixel_affine"):
        TL.apply_affine(c["x"], torch.eye(3, 4).expand(12, 13, 3, 4))                   # the same matrix on every pixel is not detected


def test_cpu_tensors_and_bad_shapes_are_refused():
    c = R.case("12x13")
    with pytest.raises(L.EmdError, match="no CPU path"):
        TL.trainer_losses(c["x"], c["y"], c["o"], c["s"])
    with pytest.raises(L.EmdError, match="no CPU path"):
        TL.apply_affine(c["x"], torch.eye(3, 4))
    with pytest.raises(L.EmdError, match="mask_type"):
        TL.trainer_losses(c["x"], c["y"], mask_type="focal")
    with pytest.raises(L.EmdError, match="depth_type"):
        TL.trainer_losses(c["x"], c["y"], depth_type="huber")
