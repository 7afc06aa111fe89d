"""-m "not gpu": the HexPlane regularisers (emd_amd.hexplane.plane_regulation, csrc/plane_reg.hip) without a GPU -- the inputs of the GPU tests
validated (the fp32 torch formulation meets the criterion against the fp64 restatement on every case), closed forms of the restatement, and the
host layer: exported symbols, argument validation, the refusal of CPU tensors, the GaussianModel methods without a network.  (The struct's
layout and the constants: tests/test_abi.py.)"""
import ctypes as C

import pytest
import torch

from emd_amd import _lib as L
from emd_amd import hexplane
from tests import plane_reg_ref as R


# ---- the reference and the cases -------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.CASES))
def test_fp32_torch_formulation_meets_the_criterion(name):
    """What validates the inputs: the reference's own fp32 arithmetic stays inside the criterion, so a failure on the GPU is the kernel's."""
    R.criterion(R.run(R.case(name), torch.float32, "cpu"), R.reference(name), name + " fp32 torch")


def test_cases_have_the_shapes_and_values_the_gpu_tests_rely_on():
    assert R.PAIRS == hexplane.PAIRS and R.SEG == L.PLANE_REG_SEG
    for name, (ch, resolutions, sigma) in R.CASES.items():
        grids = R.case(name)
        for g, res in zip(grids, resolutions):
            for p, (a, b) in enumerate(R.PAIRS):
                t = g[p]
                assert tuple(t.shape) == (1, ch, res[b], res[a]) and t.dtype == torch.float32
                assert t[0].permute(1, 2, 0).is_contiguous()                           # channel-last memory
                if p in R.TIME:
                    ones = int((t == 1).sum())
                    assert ones >= t.numel() // 10 and float((t - 1).abs().max()) < 6 * sigma
                else:
                    assert 0.1 <= float(t.min()) and float(t.max()) <= 0.5
    H = lambda name: sorted({res[k] for res in R.CASES[name][1] for k in (1, 2, 3)})
    assert H("tiny-s5e-2") == [3, 4] and H("tiny_h5-s5e-2") == [3, 4, 5]               # H = 5: the first with a fully interior gradient row
    for name in ("tiny-s5e-2", "tiny_h5-s5e-2"):
        assert sorted({t.shape[3] * t.shape[1] for g in R.case(name) for t in g}) == [15, 20, 25]           # W * C: tails, rows off 16-byte alignment
    assert H("segments-s5e-2") == [2 * R.SEG - 1, 2 * R.SEG, 2 * R.SEG + 1]           # one below, at, one above a multiple; the last spans 3 segments
    assert -(-(2 * R.SEG + 1) // R.SEG) >= 3


def test_restatement_closed_forms():
    """A plane quadratic along H has second difference 2 a everywhere; one linear along H has none; the L1 term of a plane at 1 + e is |e|."""
    h = torch.arange(7, dtype=torch.float64)[None, None, :, None].expand(1, 3, 7, 4)
    assert abs(float(R.compute_plane_smoothness(0.25 * h * h + 3 * h + 1)) - 0.25) < 1e-12
    assert float(R.compute_plane_smoothness(3 * h + 1)) == 0.0
    w = torch.arange(4, dtype=torch.float64)[None, None, None, :].expand(1, 3, 7, 4)
    assert float(R.compute_plane_smoothness(w * w)) == 0.0                              # along H only: curvature along W does not count
    grids = [[torch.full((1, 2, 5, 3), 1.0 + (0.5 if p in R.TIME else 7.0), dtype=torch.float64) for p in range(6)]]
    assert abs(float(R.l1_regulation(grids)) - 1.5) < 1e-12


# ---- host layer ------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("emd_plane_reg_workspace_size", "emd_plane_reg_forward", "emd_plane_reg_backward")


def test_new_symbols_exported():
    lib = L.load()
    for n in NEW_SYMBOLS:
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n)
    assert lib.emd_abi_version() == L.ABI_VERSION


FAKE = 0x1000        # a non-null, 16-byte aligned pointer value: every call below is refused on the host, before anything is launched or read


def _args(res=(5, 3, 4, 3), channels=5, scales=1):
    a = L.EmdPlaneRegArgs()
    a.channels, a.num_scales = channels, scales
    for s in range(min(scales, L.HEX_MAX_SCALES)):
        for k in range(4):
            a.res[s][k] = res[k]
        for p in range(6):
            a.planes[s][p], a.dL_dplanes[s][p] = FAKE, FAKE
    a.out, a.g = FAKE, FAKE
    return a


def test_workspace_size_is_host_only_and_counts_workgroups():
    lib = L.load()
    size = lambda *a, **k: lib.emd_plane_reg_workspace_size(C.byref(_args(*a, **k)))
    assert size() == 6 * 16                                                        # six planes, one workgroup each, two doubles per workgroup
    seg, chunk = L.PLANE_REG_SEG, 1024
    wg = lambda H, W, ch: -(-H // seg) * -(-(W * ch) // chunk)
    res, ch = (64, 2 * seg - 1, 2 * seg, 2 * seg + 1), 32
    assert size(res, ch) == 16 * sum(wg(res[b], res[a], ch) for a, b in R.PAIRS)
    assert size(res, ch, scales=2) == 2 * size(res, ch)
    assert size((5, 2, 4, 3)) == 0 and size(channels=0) == 0 and size(scales=L.HEX_MAX_SCALES + 1) == 0      # what the forward refuses
    assert lib.emd_plane_reg_workspace_size(None) == 0


@pytest.mark.parametrize("res", [(5, 2, 4, 3), (5, 3, 2, 3), (5, 3, 4, 2)])
def test_H_below_3_is_an_argument_error(res):
    """The reference returns NaN (the mean of no elements); here it is EMD_ERR_INVALID with a message, forward and backward."""
    lib = L.load()
    assert lib.emd_plane_reg_forward(C.byref(_args(res)), FAKE, 1 << 20, None) == L.EMD_ERR_INVALID
    assert b"H = 2 < 3" in lib.emd_last_error()
    assert lib.emd_plane_reg_backward(C.byref(_args(res)), None) == L.EMD_ERR_INVALID
    assert b"H = 2 < 3" in lib.emd_last_error()
    # W may be anything: res[0] is never an H
    assert lib.emd_plane_reg_workspace_size(C.byref(_args((1, 3, 3, 3)))) == 6 * 16


def test_argument_validation_reports_errors():
    lib = L.load()
    bad = lambda rc, word, code=L.EMD_ERR_INVALID: rc == code and word in lib.emd_last_error()
    assert bad(lib.emd_plane_reg_forward(None, FAKE, 1 << 20, None), b"null args")
    assert bad(lib.emd_plane_reg_forward(C.byref(_args(channels=0)), FAKE, 1 << 20, None), b"bad sizes")
    assert bad(lib.emd_plane_reg_forward(C.byref(_args(scales=0)), FAKE, 1 << 20, None), b"bad sizes")
    assert bad(lib.emd_plane_reg_forward(C.byref(_args((5, 0, 4, 3))), FAKE, 1 << 20, None), b"bad resolution")
    a = _args()
    a.planes[0][4] = None
    assert bad(lib.emd_plane_reg_forward(C.byref(a), FAKE, 1 << 20, None), b"null plane 4")
    a = _args()
    a.planes[0][1] = FAKE + 2
    assert bad(lib.emd_plane_reg_forward(C.byref(a), FAKE, 1 << 20, None), b"4-byte aligned")
    a = _args()
    a.out = None
    assert bad(lib.emd_plane_reg_forward(C.byref(a), FAKE, 1 << 20, None), b"null out")
    assert bad(lib.emd_plane_reg_forward(C.byref(_args()), None, 1 << 20, None), b"workspace", L.EMD_ERR_WORKSPACE)
    assert bad(lib.emd_plane_reg_forward(C.byref(_args()), FAKE, 6 * 16 - 1, None), b"workspace", L.EMD_ERR_WORKSPACE)
    assert bad(lib.emd_plane_reg_forward(C.byref(_args()), FAKE + 4, 1 << 20, None), b"workspace", L.EMD_ERR_WORKSPACE)
    a = _args()
    a.dL_dplanes[0][3] = None
    assert bad(lib.emd_plane_reg_backward(C.byref(a), None), b"null plane 3")
    a = _args()
    a.g = None
    assert bad(lib.emd_plane_reg_backward(C.byref(a), None), b"null g")


def test_cpu_tensors_are_refused():
    grids = R.case("tiny-s5e-2")
    with pytest.raises(L.EmdError, match="no CPU path"):
        hexplane.plane_regulation(grids, 1.0, 1.0, 1.0)
    field = hexplane.HexPlaneField(1.6, {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 4, "resolution": [4, 4, 4, 3]}, [1, 2])
    with pytest.raises(L.EmdError, match="no CPU path"):
        field.regulation(1.0, 1.0, 1.0, return_terms=True)


def test_gaussian_model_without_a_deformation_network_raises():
    from emd_amd.gaussian_model import GaussianModel
    gm = GaussianModel(device="cpu")
    for call in (gm._plane_regulation, gm._time_regulation, gm._l1_regulation, lambda: gm.compute_regulation(1.0, 1.0, 1.0)):
        with pytest.raises(RuntimeError, match="without a deformation network"):
            call()
