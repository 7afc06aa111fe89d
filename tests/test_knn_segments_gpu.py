"""-m gpu: emd_knn_segments (knn.knn_segments, KnnTable(..., segment_start=)) on an MI355X: the exact k-NN restricted to the rows of a point's own
segment, against the fp64 brute force per segment (tests/neighbour_std_ref.py on tests/knn_checks.py, pinned by tests/test_neighbour_std_cpu.py).
About 1 500 clustered points in ten segments of the sizes 0, 1, 2, 3, 63, 64, 65, 257, 300 and the rest, with rows in front of the first and
behind the last segment that belong to nobody; D2_RTOL and the near-tie rule are the project's."""
import pytest
import torch

from tests import knn_checks as kc
from tests import neighbour_std_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 1500


def _run(points, seg, k):
    from emd_amd.knn import knn_segments
    idx, d2 = knn_segments(points.to(DEV), seg.to(DEV), k)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (points.shape[0], k)
    return idx.cpu(), d2.cpu()


@pytest.fixture(scope="module")
def cloud():
    return kc.clustered_points(N, seed=31, clusters=6, copies=100), R.segment_table(N)


@pytest.mark.parametrize("k", [1, 2, 8, 32])
def test_every_row_against_the_brute_force_of_its_segment(cloud, k):
    p, seg = cloud
    idx, d2 = _run(p, seg, k)
    worst = R.check_segments(p, seg, idx, d2, k)
    print(f"segments, k={k}: worst relative d2 error {worst:.3e}")
    # exactly the empty slots the contract says: the sizes 0, 1, 2 and 3 give 0, 0, 1 and 2 neighbours, the rows of nobody none
    ref_idx, _ = R.segment_knn(p, seg, k)
    assert torch.equal(idx == -1, ref_idx == -1)
    s = seg.tolist()
    assert s[1] - s[0] == 0 and s[2] - s[1] == 1 and s[3] - s[2] == 2 and s[4] - s[3] == 3
    filled = (idx >= 0).sum(dim=1)
    assert int(filled[s[1]]) == 0 and filled[s[2]:s[3]].tolist() == [min(k, 1)] * 2 and filled[s[3]:s[4]].tolist() == [min(k, 2)] * 3
    assert int(filled[:s[0]].sum()) == 0 and int(filled[s[-1]:].sum()) == 0 and s[0] > 0 and s[-1] < N
    assert torch.isinf(d2[idx == -1]).all() and (d2[idx == -1] > 0).all()
    # deterministic: a second call returns the same bits
    idx2, d22 = _run(p, seg, k)
    assert torch.equal(idx, idx2) and torch.equal(d2, d22)


def test_instances_do_not_see_each_other():
    """Two people standing in the same place: every point has a twin at distance 0 in the other segment, and must not find it."""
    from emd_amd.knn import knn
    a = kc.clustered_points(300, seed=32, clusters=3, copies=10)
    both = torch.cat([a, a])
    seg = torch.tensor([0, 300, 600])
    idx, d2 = _run(both, seg, 3)
    ia, da = knn(a.to(DEV), 3)
    ia, da = ia.cpu(), da.cpu()
    assert torch.equal(d2[:300], da) and torch.equal(d2[300:], da)       # the same fp32 expression: the same bits
    untied = (da[:, 1:] > da[:, :-1]).all(dim=1)
    assert int(untied.sum()) > 250
    assert torch.equal(idx[:300][untied], ia[untied]) and torch.equal(idx[300:][untied] - 300, ia[untied])
    assert ((idx[:300] >= 0) & (idx[:300] < 300)).all() and (idx[300:] >= 300).all()
    lonely = torch.ones(300, dtype=torch.bool)
    lonely[:20] = False                                                  # the 10 coincident pairs inside a segment
    assert (d2[:300][lonely, 0] > 0).all() and (d2[300:][lonely, 0] > 0).all() and (d2[:20, 0] == 0).all()
    wi, wd = knn(both.to(DEV), 3)                                        # the search over the whole cloud returns the twin at distance 0
    assert (wd.cpu()[:, 0] == 0).all()
    twin = torch.cat([torch.arange(300, 600), torch.arange(0, 300)])
    assert (wi.cpu()[:, 0].long()[torch.cat([lonely, lonely])] == twin[torch.cat([lonely, lonely])]).all()


@pytest.mark.parametrize("k", [3, 8, 32])
def test_ties_put_the_lower_row_first(k):
    """Integer lattice points: every squared distance is exact in fp32, so the table must equal the brute force with lower-row-first ties."""
    g = torch.Generator().manual_seed(33)
    r = torch.arange(6.0)
    lattice = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), dim=-1).reshape(-1, 3)[torch.randperm(216, generator=g)].contiguous()
    seg = torch.tensor([0, 100, 216])
    idx, d2 = _run(lattice, seg, k)
    ref_idx, ref_d2 = R.segment_knn(lattice, seg, k)
    assert int((ref_d2[:, 1:] == ref_d2[:, :-1]).sum()) > 216            # ties everywhere
    assert torch.equal(d2.double(), ref_d2)
    assert torch.equal(idx.long(), ref_idx)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_row_is_empty_and_nobodys_neighbour(cloud, bad):
    p, seg = cloud
    p = p.clone()
    rows = [2, int(seg[4]) + 5, int(seg[8]) + 17, N - 3]                 # nobody's row, a 63-row segment, the 300-row segment, nobody's row
    for i, r in enumerate(rows):
        p[r, i % 3] = bad
    idx, d2 = _run(p, seg, 8)
    for r in rows:
        assert (idx[r] == -1).all() and torch.isinf(d2[r]).all() and (d2[r] > 0).all()
        assert (idx != r).all()
    R.check_segments(p, seg, idx, d2, 8)
    assert torch.equal(idx == -1, R.segment_knn(p, seg, 8)[0] == -1)


def test_no_points_no_segments_and_clamped_bounds(cloud):
    from emd_amd.knn import knn_segments
    e_idx, e_d2 = knn_segments(torch.empty(0, 3, device=DEV), torch.tensor([0, 0], device=DEV), 3)
    assert e_idx.shape == (0, 3) and e_d2.shape == (0, 3)
    p, seg = cloud
    idx, d2 = _run(p[:100], torch.tensor([0]), 3)                        # S == 0: every row belongs to nobody
    assert (idx == -1).all() and torch.isinf(d2).all()
    idx, d2 = _run(p, torch.tensor([-7, 40, 5000]), 3)                   # bounds clamped to [0, N]
    ref_idx, _ = R.segment_knn(p, torch.tensor([0, 40, N]), 3)
    R.check_segments(p, torch.tensor([0, 40, N]), idx, d2, 3)
    assert torch.equal(idx == -1, ref_idx == -1)
    with pytest.raises(ValueError):
        knn_segments(p.to(DEV), seg.to(DEV), 33)


def test_table_with_segments_reverse_and_embedding_reg(cloud):
    from emd_amd.knn import KnnTable, embedding_reg, knn
    p, seg = cloud
    t = KnnTable(p.to(DEV), k=8, weight_fn=lambda d2: torch.exp(-0.5 * d2).clamp_min(1e-6), segment_start=seg.to(DEV))
    torch.cuda.synchronize()
    idx, d2 = _run(p, seg, 8)
    assert torch.equal(t.idx.cpu(), idx) and torch.equal(t.d2.cpu(), d2)
    kc.check_reverse(t.idx, t.rev_start, t.rev_slot)
    assert int(t.rev_start[-1]) == int((idx >= 0).sum()) < N * 8
    e = (torch.randn(N, 8, generator=torch.Generator().manual_seed(34)) * 0.3).to(DEV).requires_grad_(True)
    loss = embedding_reg(e, t)
    (loss * 1.75).backward()
    ref_loss, ref_grad = kc.reg_reference(e, t.idx, t.w)
    assert abs(float(loss.detach()) - float(ref_loss)) <= 1e-5 * float(ref_loss)
    R.grad_close(e.grad, ref_grad * 1.75, "embedding_reg on a segmented table")
    # refresh keeps the segmented path, and a table without segments is the search over the whole cloud, as before
    moved = p + 0.01
    t.refresh(moved.to(DEV))
    mi, md = _run(moved, seg, 8)
    assert torch.equal(t.idx.cpu(), mi) and torch.equal(t.d2.cpu(), md)
    kc.check_reverse(t.idx, t.rev_start, t.rev_slot)
    whole = KnnTable(p.to(DEV), k=8)
    wi, wd = knn(p.to(DEV), 8)
    assert whole.segment_start is None and torch.equal(whole.idx, wi) and torch.equal(whole.d2, wd)
    whole.refresh(moved.to(DEV))
    wi, wd = knn(moved.to(DEV), 8)
    assert torch.equal(whole.idx, wi) and torch.equal(whole.d2, wd)
