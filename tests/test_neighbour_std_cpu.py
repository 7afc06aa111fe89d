"""-m "not gpu": the segmented k-NN and the neighbour-std regulariser (emd_knn_segments, emd_neighbour_std_forward / _backward; DESIGN.md section
8.19) without a GPU: the fp64 restatement of tests/neighbour_std_ref.py against plain Python, the input conditions of every case the GPU tests
use, an fp32 emulation of the contract's operation order against the GPU tolerances on those inputs, and the host-only refusals (the struct
mirror: tests/test_abi.py)."""
import ctypes as C
import math
import os

import pytest
import torch

from emd_amd import _lib as L
from tests import knn_checks as kc
from tests import neighbour_std_cases as cases
from tests import neighbour_std_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("emd_knn_segments", "emd_neighbour_std_workspace_size", "emd_neighbour_std_forward", "emd_neighbour_std_backward")


def test_new_symbols_exported_and_constants_match_the_header():
    import re
    lib = L.load()
    for name in NEW:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    src = open(os.path.join(ROOT, "include", "emd_raster.h")).read()
    assert int(re.search(r"#define EMD_NSTD_MAX_BLOCKS (\d+)", src).group(1)) == L.NSTD_MAX_BLOCKS == 8
    assert int(re.search(r"#define EMD_NSTD_MAX_COLS (\d+)", src).group(1)) == L.NSTD_MAX_COLS == 64
    for name, code in L.NSTD_ACT.items():
        assert int(re.search(rf"#define EMD_NSTD_ACT_{name.upper()} (\d+)", src).group(1)) == code
    assert int(re.search(r"#define EMD_ABI_VERSION (\d+)", src).group(1)) == 31 == L.ABI_VERSION
    assert lib.emd_neighbour_std_workspace_size() >= 16


def _args(n=10, k=2, blocks=1, cols=4, act=0, weight=1.0):
    one = 256                                                            # a non-null pointer that is never dereferenced: every call below fails validation
    a = L.EmdNeighbourStdArgs()
    a.num_points, a.k, a.num_blocks = n, k, blocks
    a.idx = a.rev_start = a.rev_slot = a.stash = a.terms = a.g_terms = one
    for b in range(min(blocks, 8) if blocks > 0 else 0):
        a.x[b], a.dx[b], a.cols[b], a.act[b], a.weight[b] = one, one, cols, act, weight
    return a


def test_invalid_arguments_return_error_codes():
    lib = L.load()
    one = C.c_void_p(256)
    fwd = lambda a: lib.emd_neighbour_std_forward(C.byref(a), one, 1 << 20, None)
    bwd = lambda a: lib.emd_neighbour_std_backward(C.byref(a), None)
    for k in (0, 33, -1):
        assert lib.emd_knn_segments(10, 2, k, one, one, one, one, None) == L.EMD_ERR_INVALID
        assert b"1 <= k <= 32" in lib.emd_last_error()
        assert fwd(_args(k=k)) == L.EMD_ERR_INVALID and b"1 <= k <= 32" in lib.emd_last_error()
        assert bwd(_args(k=k)) == L.EMD_ERR_INVALID and b"1 <= k <= 32" in lib.emd_last_error()
    assert lib.emd_knn_segments(-1, 2, 3, one, one, one, one, None) == L.EMD_ERR_INVALID
    assert lib.emd_knn_segments(10, -1, 3, one, one, one, one, None) == L.EMD_ERR_INVALID and b"num_segments" in lib.emd_last_error()
    assert lib.emd_knn_segments(10, 2, 3, None, one, one, one, None) == L.EMD_ERR_INVALID and b"null points" in lib.emd_last_error()
    assert lib.emd_knn_segments(10, 2, 3, one, one, None, None, None) == L.EMD_ERR_INVALID and b"no output" in lib.emd_last_error()
    assert lib.emd_knn_segments(10, 2, 3, one, None, one, one, None) == L.EMD_ERR_INVALID and b"null segment_start" in lib.emd_last_error()
    assert lib.emd_knn_segments(0, 0, 3, None, None, None, None, None) == L.EMD_OK                     # zero points: nothing to do
    for blocks in (0, 9, -1):
        assert fwd(_args(blocks=blocks)) == L.EMD_ERR_INVALID and b"num_blocks" in lib.emd_last_error()
        assert bwd(_args(blocks=blocks)) == L.EMD_ERR_INVALID and b"num_blocks" in lib.emd_last_error()
    for cols in (0, 65, -3):
        assert fwd(_args(cols=cols)) == L.EMD_ERR_INVALID and b"columns, outside 1 .. 64" in lib.emd_last_error()
        assert bwd(_args(cols=cols)) == L.EMD_ERR_INVALID and b"columns, outside 1 .. 64" in lib.emd_last_error()
    assert fwd(_args(act=3)) == L.EMD_ERR_INVALID and b"activation" in lib.emd_last_error()
    assert lib.emd_neighbour_std_forward(None, one, 1 << 20, None) == L.EMD_ERR_INVALID and b"null args" in lib.emd_last_error()
    for field, msg in (("idx", b"null idx / stash"), ("stash", b"null idx / stash"), ("terms", b"null terms")):
        a = _args()
        setattr(a, field, None)
        assert fwd(a) == L.EMD_ERR_INVALID and msg in lib.emd_last_error(), field
    a = _args(blocks=2)
    a.x[1] = None
    assert fwd(a) == L.EMD_ERR_INVALID and b"null values of block 1" in lib.emd_last_error()
    a = _args(blocks=2)
    a.dx[1] = None
    assert bwd(a) == L.EMD_ERR_INVALID and b"null gradient of block 1" in lib.emd_last_error()
    a.weight[1] = 0.0                                                    # a skipped block's pointers are not looked at
    a.rev_slot = None
    assert bwd(a) == L.EMD_ERR_INVALID and b"null rev_start / rev_slot / g_terms" in lib.emd_last_error()
    a = _args()
    a.stash = 260
    assert fwd(a) == L.EMD_ERR_INVALID and b"8-byte aligned" in lib.emd_last_error()
    assert lib.emd_neighbour_std_forward(C.byref(_args()), None, 0, None) == L.EMD_ERR_WORKSPACE
    assert lib.emd_neighbour_std_forward(C.byref(_args()), one, 64, None) == L.EMD_ERR_WORKSPACE
    assert bwd(_args(n=0)) == L.EMD_OK                                   # zero points: nothing to do


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    from emd_amd import knn as K
    from emd_amd.nodes import SMPLNodes
    p = torch.rand(50, 3)
    with pytest.raises(L.EmdError, match="no CPU path"):
        K.knn_segments(p, torch.tensor([0, 50]), 3)
    with pytest.raises(L.EmdError, match="no CPU path"):
        K.KnnTable(p, k=2, segment_start=torch.tensor([0, 50]))
    with pytest.raises(L.EmdError, match="no CPU path"):
        K.neighbour_std([torch.zeros(50, 4)], None, [1.0], ["identity"])
    with pytest.raises(ValueError, match="knn_neighbors"):
        SMPLNodes("SMPLNodes", dict(sh_degree=1, knn_neighbors=1), device="cpu")
    node = SMPLNodes("SMPLNodes", dict(sh_degree=1), device="cpu")
    assert node.knn_neighbors == 3 and node.knn_update_interval == 100
    assert set(SMPLNodes.NODE_PARAM_GROUPS) >= {"ins_rotation", "smpl_rotation", "ins_translation"}
    assert list(SMPLNodes.KNN_REG_BLOCKS) == ["lambda_std_q", "lambda_std_s", "lambda_std_o", "lambda_std_shs_dc", "lambda_std_shs_rest"]


# ---- the checkers themselves ---------------------------------------------------------------------------------------------------------------------
def _plain(blocks, idx, weights, acts):
    """Plain Python: per block the mean over points and columns of the sample standard deviation of the group's activated values, and its
    gradient by the textbook formula d sigma / d v_j = (v_j - mean) / ((g - 1) sigma)."""
    fn = {"identity": (lambda x: x, lambda x: 1.0), "exp": (math.exp, math.exp),
          "sigmoid": (lambda x: 1 / (1 + math.exp(-x)), lambda x: math.exp(-x) / (1 + math.exp(-x)) ** 2)}
    n = len(idx)
    terms, grads = [], []
    for x, w, a in zip(blocks, weights, acts):
        rows = [[float(t) for t in r] for r in x.reshape(n, -1).tolist()]
        cols = len(rows[0])
        f, df = fn[a]
        total, grad = 0.0, [[0.0] * cols for _ in range(n)]
        for p in range(n):
            group = [p] + [m for m in idx[p] if m >= 0]
            if len(group) < 2:
                continue
            for c in range(cols):
                vals = [f(rows[m][c]) for m in group]
                mean = sum(vals) / len(vals)
                sigma = math.sqrt(sum((t - mean) ** 2 for t in vals) / (len(vals) - 1))
                total += sigma
                if sigma > 0:
                    for m, t in zip(group, vals):
                        grad[m][c] += (t - mean) / ((len(vals) - 1) * sigma) * df(rows[m][c])
        terms.append(w * total / (n * cols))
        grads.append(torch.tensor(grad, dtype=torch.float64) * w / (n * cols))
    return terms, grads


def test_reference_agrees_with_plain_python_on_12_points():
    g = torch.Generator().manual_seed(3)
    pts = torch.rand(12, 3, generator=g)
    idx, _ = R.segment_knn(pts, torch.tensor([0, 7, 8, 12]), 3)             # segments of 7, 1 and 4: -1 slots and a group of one
    assert (idx[7] == -1).all() and (idx[8:, 2] >= 0).all() and int((idx == -1).sum()) == 3
    blocks = [torch.randn(12, 4, generator=g), torch.randn(12, 3, generator=g) * 0.3 - 2, torch.randn(12, 1, generator=g), torch.randn(12, 2, 3, generator=g)]
    blocks[0][:7] = blocks[0][0]                                          # a constant group: sigma 0, gradient 0
    acts, weights = ["identity", "exp", "sigmoid", "identity"], [1.0, 0.5, 2.0, 0.25]
    terms, grads = R.reference(blocks, idx, weights, acts)
    pterms, pgrads = _plain(blocks, idx.tolist(), weights, acts)
    for b in range(4):
        assert abs(float(terms[b]) - pterms[b]) <= 1e-13 * abs(pterms[b]), b
        assert torch.allclose(grads[b].reshape(12, -1), pgrads[b], rtol=1e-10, atol=1e-15), b
    assert torch.count_nonzero(grads[0][:7]) == 0 and torch.count_nonzero(grads[0][8:]) > 0
    # upstream scalars scale the gradients block by block; a zero weight gives no gradient at all
    gt = torch.tensor([2.0, -1.0, 0.5, 3.0])
    terms2, grads2 = R.reference(blocks, idx, [1.0, 0.0, 2.0, 0.25], acts, gt)
    assert float(terms2[1]) == 0.0 and grads2[1] is None and torch.allclose(grads2[3], 3.0 * grads[3], rtol=1e-12)


def test_segment_knn_agrees_with_the_brute_force_per_segment():
    pts = kc.clustered_points(400, seed=4, clusters=4, copies=20)
    seg = torch.tensor([3, 3, 4, 6, 120, 390])
    idx, d2 = R.segment_knn(pts, seg, 8)
    assert R.check_segments(pts, seg, idx.int(), d2.float(), 8) <= kc.D2_RTOL
    assert (idx[:3] == -1).all() and (idx[390:] == -1).all() and (idx[3] == -1).all()
    assert idx[4].tolist() == [5] + [-1] * 7 and idx[5].tolist() == [4] + [-1] * 7
    # each kind of defect is caught
    bad = idx.clone()
    bad[200, 0] = 100                                                    # a neighbour from another segment
    with pytest.raises(AssertionError):
        R.check_segments(pts, seg, bad.int(), d2.float(), 8)
    bad = idx.clone()
    bad[1, 0] = 0
    with pytest.raises(AssertionError):
        R.check_segments(pts, seg, bad.int(), d2.float(), 8)
    # ties: the lower row first
    lat = torch.tensor([[0., 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0]])
    ti, td = R.segment_knn(lat, torch.tensor([0, 5]), 3)
    assert ti[0].tolist() == [1, 2, 3] and td[0].tolist() == [1.0, 1.0, 1.0]


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_gpu_case_meets_the_input_conditions_and_the_fp32_emulation_meets_the_gpu_tolerances(name):
    c = cases.build(name)
    assert c["idx"].shape == (cases.N, c["K"] - 1)
    if c["tight"]:
        # every value within a factor 2 of every other: all differences are exact (Sterbenz), the bound is relative to sigma itself
        for x in c["blocks"]:
            assert float(x.min()) > 0 and float(x.max()) < 2 * float(x.min())
        ratio = []
        for x, bad in zip(c["blocks"], R.conditions(c["blocks"], c["idx"], c["acts"], floor=1e-5)):
            ratio.append(int(bad.sum()))
        print(f"{name}: (group, column) pairs below 1e-5 max|v|: {ratio}")
    else:
        R.assert_conditions(c["blocks"], c["idx"], c["acts"])
    terms, grads = R.reference(c["blocks"], c["idx"], c["weights"], c["acts"], c["g_terms"])
    eterms, egrads = R.emulate_fp32(c["blocks"], c["idx"], c["weights"], c["acts"], c["g_terms"])
    R.terms_close(eterms, terms, c["acts"], c["weights"], name, rtol=R.TIGHT_RTOL if c["tight"] else None)
    for b, (ge, gr) in enumerate(zip(egrads, grads)):
        assert (ge is None) == (gr is None) == (c["weights"][b] == 0)
        if gr is not None:
            R.grad_close(ge, gr, f"{name} block {b}")
    assert int((c["idx"] == -1).sum()) > 0 and int(((c["idx"] >= 0).sum(dim=1) == 0).sum()) > 0      # -1 slots and groups of one
