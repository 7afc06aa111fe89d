"""-m "not gpu": the k-NN / embedding-regulariser entry points (ABI 28) are exported and validate their arguments without a GPU; the Python
layer refuses CPU tensors; and the torch checkers that tests/test_knn_gpu.py relies on agree with a plain brute force on 500 points."""
import ctypes as C
import math

import pytest
import torch

from emd_amd import _lib as L
from tests import knn_checks as kc

NEW = ("emd_knn_workspace", "emd_knn", "emd_knn_reverse_workspace", "emd_knn_reverse", "emd_embed_reg_forward", "emd_embed_reg_backward")


def test_new_symbols_exported_and_abi_28():
    lib = L.load()
    for name in NEW:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.emd_abi_version() == L.ABI_VERSION >= 28


def test_header_constants_match_binding():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "emd_raster.h")).read()
    assert int(re.search(r"#define EMD_KNN_MAX_K (\d+)", src).group(1)) == L.KNN_MAX_K == 32
    assert int(re.search(r"#define EMD_EMBED_REG_SCRATCH_WORDS (\d+)", src).group(1)) == L.EMBED_REG_SCRATCH_WORDS


def test_workspace_queries_host_only():
    lib = L.load()
    assert lib.emd_knn_workspace(10, 0) == 0 and lib.emd_knn_workspace(10, 33) == 0 and lib.emd_knn_workspace(-1, 3) == 0
    assert lib.emd_knn_workspace(2 ** 30, 32) == 0                       # N * k must fit 31 bits
    a, b = lib.emd_knn_workspace(1000, 3), lib.emd_knn_workspace(2_000_000, 20)
    assert 0 < a < b and b >= 2_000_000 * (16 + 5 * 4)                   # sorted float4 points + keys / values
    assert lib.emd_knn_workspace(0, 3) > 0
    assert lib.emd_knn_reverse_workspace(10, 0) == 0
    assert lib.emd_knn_reverse_workspace(2_000_000, 20) >= 2_000_000 * 20 * 12


def test_invalid_arguments_return_error_codes():
    lib = L.load()
    one = C.c_void_p(256)                                                # a non-null pointer that is never dereferenced: every call below fails validation
    for k in (0, 33, -1):
        assert lib.emd_knn(10, k, one, one, one, None, one, 1 << 20, None) == L.EMD_ERR_INVALID
        assert b"k" in lib.emd_last_error()
        assert lib.emd_knn_reverse(10, k, one, one, one, one, 1 << 20, None) == L.EMD_ERR_INVALID
        assert lib.emd_embed_reg_forward(10, k, 4, one, one, None, None, one, one, None) == L.EMD_ERR_INVALID
        assert lib.emd_embed_reg_backward(10, k, 4, one, one, None, None, one, one, one, one, one, 0, None) == L.EMD_ERR_INVALID
    assert lib.emd_knn(-5, 3, one, one, one, None, one, 1 << 20, None) == L.EMD_ERR_INVALID
    assert lib.emd_knn(10, 3, None, one, one, None, one, 1 << 20, None) == L.EMD_ERR_INVALID          # null points
    assert b"null" in lib.emd_last_error()
    assert lib.emd_knn(10, 3, one, None, None, None, one, 1 << 20, None) == L.EMD_ERR_INVALID          # no output at all
    assert lib.emd_knn(10, 3, one, one, one, None, None, 0, None) == L.EMD_ERR_WORKSPACE               # null workspace
    assert lib.emd_knn(10, 3, one, one, one, None, one, 16, None) == L.EMD_ERR_WORKSPACE               # too small
    assert lib.emd_knn(0, 3, None, None, None, None, None, 0, None) == L.EMD_OK                        # zero points: nothing to do
    assert lib.emd_knn_reverse(10, 3, None, one, one, one, 1 << 20, None) == L.EMD_ERR_INVALID
    assert lib.emd_knn_reverse(10, 3, one, None, one, one, 1 << 20, None) == L.EMD_ERR_INVALID
    assert lib.emd_knn_reverse(10, 3, one, one, one, None, 0, None) == L.EMD_ERR_WORKSPACE
    for dim in (0, 3, 5, 64):
        assert lib.emd_embed_reg_forward(10, 20, dim, one, one, None, None, one, one, None) == L.EMD_ERR_INVALID
        assert b"embed_dim" in lib.emd_last_error()
    assert lib.emd_embed_reg_forward(10, 20, 4, None, one, None, None, one, one, None) == L.EMD_ERR_INVALID
    assert lib.emd_embed_reg_forward(10, 20, 4, one, one, None, None, None, one, None) == L.EMD_ERR_INVALID     # null loss
    assert lib.emd_embed_reg_forward(10, 20, 4, one, one, None, None, one, None, None) == L.EMD_ERR_INVALID     # null scratch
    assert lib.emd_embed_reg_forward(10, 20, 4, C.c_void_p(260), one, None, None, one, one, None) == L.EMD_ERR_INVALID   # misaligned rows
    assert lib.emd_embed_reg_backward(10, 20, 4, one, one, None, None, None, one, one, one, one, 0, None) == L.EMD_ERR_INVALID
    assert lib.emd_embed_reg_backward(10, 20, 4, one, one, None, None, one, one, one, one, None, 0, None) == L.EMD_ERR_INVALID
    assert lib.emd_embed_reg_backward(0, 20, 4, None, None, None, None, None, None, None, None, None, 0, None) == L.EMD_OK


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    from emd_amd import knn as K
    p = torch.rand(50, 3)
    with pytest.raises(L.EmdError, match="no CPU path"):
        K.knn(p, 3)
    with pytest.raises(L.EmdError, match="no CPU path"):
        K.distCUDA2(p)
    with pytest.raises(L.EmdError, match="no CPU path"):
        K.KnnTable(p, k=20)

    class _T:                                                            # the fields embedding_reg looks at before it touches the device
        N, k = 50, 20
    with pytest.raises(L.EmdError, match="no CPU path"):
        K.embedding_reg(torch.zeros(50, 4), _T())


# ---- the checkers themselves ---------------------------------------------------------------------------------------------------------------------
def _plain_brute(points, k):
    """30 lines of Python: every distance in double, self skipped by index, sorted by (distance, index)."""
    pts = [[float(v) for v in row] for row in points.tolist()]
    n = len(pts)
    idx, d2 = [], []
    for a in range(n):
        cand = []
        for b in range(n):
            if b == a:
                continue
            dx, dy, dz = pts[a][0] - pts[b][0], pts[a][1] - pts[b][1], pts[a][2] - pts[b][2]
            cand.append((dx * dx + dy * dy + dz * dz, b))
        cand.sort()
        idx.append([c[1] for c in cand[:k]])
        d2.append([c[0] for c in cand[:k]])
    return torch.tensor(idx), torch.tensor(d2, dtype=torch.float64)


def _cloud():
    g = torch.Generator().manual_seed(5)
    p = torch.rand(500, 3, generator=g)
    p[:20] = p[20:40]                                                    # coincident pairs: distance 0, ties
    return p


def test_brute_knn_checker_agrees_with_plain_python():
    p = _cloud()
    pi21, pd21 = _plain_brute(p, 21)
    pi, pd = pi21[:, :20].contiguous(), pd21[:, :20].contiguous()
    ti, td = kc.brute_knn(p, torch.arange(500), 20, chunk=128)
    assert torch.allclose(td, pd, rtol=1e-14, atol=0)                    # the same fp64 arithmetic up to the order of three additions
    untied = (pd21[:, 1:] > pd21[:, :-1]).all(dim=1)                     # (the 21st included: a tie across the cut is a tie)
    assert untied.sum() > 150 and torch.equal(ti[untied], pi[untied])
    # the plain result, rounded to fp32 as a device would return it, passes the checks ...
    idx32, d32 = pi.int(), pd.float()
    kc.check_invariants(p, idx32, d32)
    assert kc.check_against_brute(p, idx32, d32, torch.arange(500), 20) <= kc.D2_RTOL
    # ... and each kind of defect is caught
    bad = d32.clone(); bad[7, 3] *= 1 + 5e-6
    with pytest.raises(AssertionError):
        kc.check_against_brute(p, idx32, bad, torch.arange(500), 20)
    row = int(torch.nonzero((pd[:, 1:] - pd[:, :-1] > 1e-4 * pd[:, 1:]).all(dim=1) & (pd[:, 0] > 0))[0])     # a row far from any tie
    bad = idx32.clone(); bad[row, 0], bad[row, 1] = idx32[row, 1], idx32[row, 0]
    with pytest.raises(AssertionError):
        kc.check_against_brute(p, bad, d32, torch.arange(500), 20)
    with pytest.raises(AssertionError):
        kc.check_invariants(p, bad, d32)                                 # d2 no longer belongs to idx
    bad = idx32.clone(); bad[9, 5] = 9
    with pytest.raises(AssertionError, match="itself"):
        kc.check_invariants(p, bad, d32)
    bad = idx32.clone(); bad[9, 5] = bad[9, 4]
    with pytest.raises(AssertionError):
        kc.check_invariants(p, bad, d32)
    # an approximate answer (the true 20th neighbour replaced by the 21st) is refused
    bad_i, bad_d = pi21[:, :20].clone().int(), pd21[:, :20].clone().float()
    bad_i[:, 19], bad_d[:, 19] = pi21[:, 20].int(), pd21[:, 20].float()
    with pytest.raises(AssertionError):
        kc.check_against_brute(p, bad_i, bad_d, torch.arange(500), 20)


def test_brute_knn_handles_short_and_non_finite_rows():
    p = torch.tensor([[0., 0, 0], [1, 0, 0], [0, 2, 0], [float("nan"), 0, 0], [0, 0, 3]])
    ri, rd = kc.brute_knn(p, torch.arange(5), 20)
    assert ri.shape == (5, 4) and rd[0].tolist() == [1.0, 4.0, 9.0, math.inf]
    idx = torch.full((5, 20), -1, dtype=torch.int32)
    d2 = torch.full((5, 20), math.inf)
    for r in (0, 1, 2, 4):
        idx[r, :3], d2[r, :3] = ri[r, :3].int(), rd[r, :3].float()
    kc.check_invariants(p, idx, d2)
    kc.check_against_brute(p, idx, d2, torch.arange(5), 20)
    idx[3, 0], d2[3, 0] = 0, 1.0                                         # the NaN row must stay empty
    with pytest.raises(AssertionError):
        kc.check_against_brute(p, idx, d2, torch.arange(5), 20)


def test_reverse_checker():
    idx = torch.tensor([[1, 2], [0, 2], [0, -1]], dtype=torch.int32)
    start, slot = torch.tensor([0, 2, 3, 5]), torch.tensor([2, 4, 0, 1, 3, 0])
    kc.check_reverse(idx, start, slot)
    with pytest.raises(AssertionError):
        kc.check_reverse(idx, start, torch.tensor([4, 2, 0, 1, 3, 0]))   # not ascending inside point 0
    with pytest.raises(AssertionError):
        kc.check_reverse(idx, torch.tensor([0, 1, 3, 5]), slot)          # slot 4 filed under point 1


def test_reg_reference_agrees_with_plain_python():
    g = torch.Generator().manual_seed(11)
    p = _cloud()
    idx, d2 = _plain_brute(p, 6)
    idx[3, 4:] = -1
    e = torch.randn(500, 4, generator=g)
    w = torch.exp(-d2 * 30).float()
    loss, grad = kc.reg_reference(e, idx, w)
    ed, wd = e.double(), w.double()
    total, pairs, gref = 0.0, 0, torch.zeros(500, 4, dtype=torch.float64)
    for n in range(500):
        for j in range(6):
            m = int(idx[n, j])
            if m < 0:
                continue
            diff = ed[n] - ed[m]
            v = math.sqrt(float(wd[n, j]) * float((diff * diff).sum()) + 1e-20)
            total += v
            pairs += 1
            gref[n] += float(wd[n, j]) / v * diff
            gref[m] -= float(wd[n, j]) / v * diff
    assert pairs == 500 * 6 - 2
    assert abs(float(loss) - total / pairs) <= 1e-12 * total / pairs
    assert torch.allclose(grad, gref / pairs, rtol=1e-9, atol=1e-15)
    # the all-zero embedding: every pair contributes sqrt(1e-20), the gradient is exactly zero
    loss0, grad0 = kc.reg_reference(torch.zeros(500, 4), idx, w)
    assert abs(float(loss0) - 1e-10) <= 1e-16 and torch.count_nonzero(grad0) == 0


def test_clustered_generator_is_seeded_and_has_copies():
    a, b = kc.clustered_points(5000, 3, copies=100), kc.clustered_points(5000, 3, copies=100)
    assert torch.equal(a, b) and torch.equal(a[:100], a[100:200]) and a.dtype == torch.float32
    assert a[:, 2].std() < a[:, 0].std() / 4                            # flat in z
