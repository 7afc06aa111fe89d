"""-m gpu: the exact k-NN search (emd_knn), its transposed adjacency (emd_knn_reverse), distCUDA2 / create_from_pcd, and the embedding
regulariser (emd_embed_reg_forward / backward, embedding_reg) on an MI355X.

Reference: a brute force in fp64 on the CPU from the same fp32 coordinates (tests/knn_checks.py, itself pinned by tests/test_knn_cpu.py), never
the code under test.  At size the brute force runs on a seeded subsample of the queries against all N; the invariants (distinct, in range,
never the row itself, ascending, d2 = the fp64 distance to idx) run on every row.  Tolerance of a squared distance: 1e-6 relative, exactly 0
where the reference is 0 (derived in knn_checks.D2_RTOL).  Indices are compared exactly wherever a row has no ties.

The 2 M-point cases are in the class `TestTwoMillion`, so that a driver can give them a pytest invocation (and a time limit) of their own."""
import math

import pytest
import torch

from tests import knn_checks as kc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(points, k):
    from emd_amd.knn import knn
    idx, d2 = knn(points.to(DEV), k)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (points.shape[0], k)
    return idx.cpu(), d2.cpu()


def _sample(n, q, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:q].sort().values


@pytest.mark.parametrize("k", [1, 3, 8, 20, 32])
def test_uniform_2000_every_row_brute_forced(k):
    p = torch.rand(2000, 3, generator=torch.Generator().manual_seed(1))
    idx, d2 = _run(p, k)
    kc.check_invariants(p, idx, d2)
    worst = kc.check_against_brute(p, idx, d2, torch.arange(2000), k)
    print(f"uniform 2000, k={k}: worst relative d2 error {worst:.3e}")


@pytest.fixture(scope="module")
def clustered():
    return kc.clustered_points(200_000, seed=2)


@pytest.mark.parametrize("k", [3, 20])
def test_clustered_200k_with_coincident_points(clustered, k):
    p = clustered
    idx, d2 = _run(p, k)
    kc.check_invariants(p, idx, d2)
    assert (d2[:2000, 0] == 0).all()                                     # the 2 000 zero-distance pairs
    partner = torch.cat([torch.arange(1000, 2000), torch.arange(0, 1000)])
    assert (idx[:2000, 0].long() == partner).all()
    q = torch.cat([torch.arange(0, 2000, 7), _sample(200_000, 4096 - 286, 3)]).unique()
    worst = kc.check_against_brute(p, idx, d2, q, k)
    print(f"clustered 200k, k={k}: worst relative d2 error {worst:.3e}")
    # deterministic: a second call returns the same bits
    idx2, d22 = _run(p, k)
    assert torch.equal(d2, d22) and torch.equal(idx, idx2)


def test_points_on_one_plane():
    p = torch.rand(30_000, 3, generator=torch.Generator().manual_seed(4)) * torch.tensor([50.0, 80.0, 0.0])
    assert (p[:, 2] == 0).all()
    idx, d2 = _run(p, 20)
    kc.check_invariants(p, idx, d2)
    kc.check_against_brute(p, idx, d2, _sample(30_000, 2048, 5), 20)


def test_all_points_identical():
    p = torch.full((100, 3), 1.25)
    idx, d2 = _run(p, 20)
    kc.check_invariants(p, idx, d2)
    assert (d2 == 0).all() and (idx >= 0).all()
    kc.check_against_brute(p, idx, d2, torch.arange(100), 20)


def test_fewer_points_than_neighbours():
    p = torch.rand(5, 3, generator=torch.Generator().manual_seed(6))
    idx, d2 = _run(p, 20)
    kc.check_invariants(p, idx, d2)
    kc.check_against_brute(p, idx, d2, torch.arange(5), 20)
    assert (idx[:, 4:] == -1).all() and torch.isinf(d2[:, 4:]).all() and (idx[:, :4] >= 0).all()
    idx1, d21 = _run(p[:1], 3)                                           # a single point has no neighbour at all
    assert (idx1 == -1).all() and torch.isinf(d21).all()
    from emd_amd.knn import knn
    e_idx, e_d2 = knn(torch.empty(0, 3, device=DEV), 3)
    assert e_idx.shape == (0, 3) and e_d2.shape == (0, 3)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_row_is_empty_and_nobodys_neighbour(bad):
    p = torch.rand(3000, 3, generator=torch.Generator().manual_seed(7))
    p[1234, 1] = bad
    idx, d2 = _run(p, 20)
    assert (idx[1234] == -1).all() and torch.isinf(d2[1234]).all() and (d2[1234] > 0).all()
    assert (idx != 1234).all()
    kc.check_invariants(p, idx, d2)
    kc.check_against_brute(p, idx, d2, torch.arange(3000), 20)
    from emd_amd.knn import distCUDA2
    m = distCUDA2(p.to(DEV)).cpu()
    assert math.isinf(float(m[1234])) and torch.isfinite(m[torch.arange(3000) != 1234]).all()


def test_distCUDA2_is_the_mean_of_the_three_nearest(clustered):
    from emd_amd.knn import distCUDA2
    p = clustered
    got = distCUDA2(p.to(DEV)).cpu().double()
    assert got.shape == (200_000,)
    q = _sample(200_000, 4096, 8)
    _, rd = kc.brute_knn(p, q, 3)
    ref = rd.mean(dim=1)
    assert (torch.abs(got[q] - ref) <= 1e-6 * ref).all(), float((torch.abs(got[q] - ref) / ref.clamp_min(1e-300)).max())
    assert torch.equal(got[:1000], got[1000:2000])


def test_create_from_pcd_matches_create_from_tensors(clustered):
    from emd_amd.gaussian_model import GaussianModel
    p = clustered[:50_000].clone()
    rgb = torch.rand(50_000, 3, generator=torch.Generator().manual_seed(9))
    _, rd = kc.brute_knn(p, torch.arange(0, 50_000, 13), 3)
    ref = torch.log(torch.sqrt(torch.clamp_min(rd.mean(dim=1), 1e-7)))
    a = GaussianModel(device=DEV)
    a.create_from_pcd(p, rgb, 2.5)
    assert a.spatial_lr_scale == 2.5 and a._scaling.shape == (50_000, 3)
    got = a._scaling.detach().cpu().double()
    assert (got[:, 0] == got[:, 1]).all() and (got[:, 0] == got[:, 2]).all()
    assert (torch.abs(got[::13, 0] - ref) <= 1e-6).all(), float(torch.abs(got[::13, 0] - ref).max())
    b = GaussianModel(device=DEV)
    b.create_from_tensors(p, rgb, a._scaling.detach().clone(), 2.5)
    for name in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_embedding", "max_radii2D", "_deformation_table"):
        assert torch.equal(getattr(a, name).detach(), getattr(b, name).detach()), name
        assert getattr(a, name).requires_grad == getattr(b, name).requires_grad, name
    assert a.active_sh_degree == b.active_sh_degree and a.spatial_lr_scale == b.spatial_lr_scale


@pytest.fixture(scope="module")
def table_200k(clustered):
    from emd_amd.knn import KnnTable
    t = KnnTable(clustered.to(DEV), k=20, weight_fn=lambda d2: torch.exp(-0.5 * d2).clamp_min(1e-6))      # in (0, 1]
    torch.cuda.synchronize()
    return t


def test_reverse_table(table_200k):
    t = table_200k
    assert t.rev_start.dtype == torch.int32 and t.rev_slot.dtype == torch.int32
    kc.check_reverse(t.idx, t.rev_start, t.rev_slot)
    # with empty slots: 5 points, 20 columns
    from emd_amd.knn import KnnTable
    s = KnnTable(torch.rand(5, 3, generator=torch.Generator().manual_seed(10)).to(DEV), k=20)
    kc.check_reverse(s.idx, s.rev_start, s.rev_slot)
    assert int(s.rev_start[5]) == 20


def _reverse_of(idx):
    """emd_knn_reverse on a table of the test's own making; -> (rev_start, rev_slot), pre-filled with -7 where the call writes nothing."""
    from emd_amd import _lib as L
    lib = L.load()
    n, k = idx.shape
    idx = idx.to(torch.int32).to(DEV).contiguous()
    rev_start = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    rev_slot = torch.full((n * k,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.emd_knn_reverse_workspace(n, k), dtype=torch.uint8, device=DEV)
    L.check(lib.emd_knn_reverse(n, k, idx.data_ptr(), rev_start.data_ptr(), rev_slot.data_ptr(), ws.data_ptr(), ws.numel(),
                                torch.cuda.current_stream().cuda_stream), "emd_knn_reverse")
    torch.cuda.synchronize()
    return rev_start.cpu(), rev_slot.cpu()


def test_reverse_of_synthetic_tables():
    """emd_knn_reverse takes any idx: tables no point cloud produces.  One hub that every filled slot targets (one digit holds every key of
    the sort), no filled slot at all (everything dropped), the last point only, and 257 points (nine target bits: two passes)."""
    g = torch.Generator().manual_seed(30)
    n, k = 3000, 20
    empty = torch.rand(n, k, generator=g) < 0.2
    tables = {
        "hub": torch.where(empty, -1, 0),
        "empty": torch.full((n, k), -1),
        "last": torch.where(empty, -1, n - 1),
        "uniform_257": torch.randint(0, 257, (257, k), generator=g),
    }
    for name, idx in tables.items():
        rev_start, rev_slot = _reverse_of(idx)
        kc.check_reverse(idx, rev_start, rev_slot)
        m = int((idx >= 0).sum())
        assert int(rev_start[-1]) == m, name
        assert (rev_slot[m:] == -7).all(), f"{name}: slots behind the {m} filled ones were written"
    assert int((tables["uniform_257"] == 256).sum()) > 0             # the ninth bit is in use


def _grad_close(got, ref):
    got, ref = got.detach().cpu().double(), ref.double()
    err = torch.abs(got - ref)
    bound = 1e-4 * torch.abs(ref) + 1e-6 * torch.abs(ref).max()         # the standing gradient criterion
    l2 = float(torch.linalg.norm(got - ref) / torch.linalg.norm(ref))
    print(f"gradient: worst err / bound {float((err / bound).max()):.3f}, relative L2 {l2:.3e}")
    assert (err <= bound).all(), float((err / bound).max())
    assert l2 <= 1e-5, l2


@pytest.mark.parametrize("E", [4, 32])
@pytest.mark.parametrize("store", [False, True])
def test_regulariser_against_fp64_autograd(table_200k, E, store):
    from emd_amd.knn import embedding_reg
    t = table_200k
    assert 0 < float(t.w.min()) and float(t.w.max()) <= 1.0
    t.store_factors = store
    t.factors = torch.empty_like(t.w) if store else None
    try:
        e = (torch.randn(200_000, E, generator=torch.Generator().manual_seed(12)) * 0.3).to(DEV).requires_grad_(True)
        loss = embedding_reg(e, t)
        (loss * 1.75).backward()
        ref_loss, ref_grad = kc.reg_reference(e, t.idx, t.w)
        rel = abs(float(loss.detach()) - float(ref_loss)) / float(ref_loss)
        print(f"E={E} store={store}: loss {float(loss):.8e} ref {float(ref_loss):.8e} rel {rel:.3e}")
        assert rel <= 1e-5
        _grad_close(e.grad, ref_grad * 1.75)
        # bit-identical from run to run
        e2 = e.detach().clone().requires_grad_(True)
        loss2 = embedding_reg(e2, t)
        (loss2 * 1.75).backward()
        assert torch.equal(loss, loss2) and torch.equal(e.grad, e2.grad)
    finally:
        t.store_factors, t.factors = False, None


def test_regulariser_counts_only_filled_slots():
    from emd_amd.knn import KnnTable, embedding_reg
    p = torch.rand(12, 3, generator=torch.Generator().manual_seed(13))
    p[5, 0] = float("nan")
    t = KnnTable(p.to(DEV), k=20, weight_fn=lambda d2: torch.exp(-d2))
    e = torch.randn(12, 8, generator=torch.Generator().manual_seed(14)).to(DEV).requires_grad_(True)
    loss = embedding_reg(e, t)
    loss.backward()
    ref_loss, ref_grad = kc.reg_reference(e, t.idx, t.w)
    assert int((t.idx >= 0).sum()) == 11 * 10
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * float(ref_loss)
    _grad_close(e.grad, ref_grad)
    assert (e.grad[5] == 0).all()


def test_zero_embedding_gives_1e_minus_10_and_a_zero_gradient():
    from emd_amd.gaussian_model import GaussianModel
    from emd_amd.knn import embedding_reg
    m = GaussianModel(device=DEV)
    m.create_from_pcd(kc.clustered_points(20_000, seed=15), torch.rand(20_000, 3), 1.0)
    t = m.knn_table(20)
    assert m.knn_table(20) is t                                          # cached
    loss = embedding_reg(m.get_embedding, t)
    loss.backward()
    assert abs(float(loss) - 1e-10) <= 1e-5 * 1e-10, float(loss)
    g = m._embedding.grad
    assert torch.isfinite(g).all() and torch.count_nonzero(g) == 0


def test_accumulate_flag_adds_to_a_prefilled_buffer(table_200k):
    from emd_amd import knn as K
    t = table_200k
    e = (torch.randn(200_000, 4, generator=torch.Generator().manual_seed(16)) * 0.3).to(DEV)
    g = torch.full((1,), 0.5, device=DEV)
    fwd = K.embed_reg_forward(e, t)
    fresh = K.embed_reg_backward(e, t, fwd, g, torch.full_like(e, 7.0), accumulate=False)
    base = torch.randn(200_000, 4, generator=torch.Generator().manual_seed(17)).to(DEV)
    added = K.embed_reg_backward(e, t, fwd, g, base.clone(), accumulate=True)
    assert torch.equal(added, base + fresh)                              # one fp32 add per element on top of the same gradient bits
    assert float(fresh.abs().max()) > 0


def test_capture_and_replay_matches_eager_bit_for_bit(table_200k):
    from emd_amd.knn import embedding_reg
    t = table_200k
    gen = torch.Generator().manual_seed(18)
    values = [(torch.randn(200_000, 4, generator=gen) * 0.3).to(DEV) for _ in range(3)]
    eager = []
    for v in values:
        e = v.clone().requires_grad_(True)
        loss = embedding_reg(e, t)
        loss.backward()
        eager.append((loss.detach().clone(), e.grad.clone()))
    static_e = values[0].clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                       # warm-up on the capture stream (allocator, autograd)
        embedding_reg(static_e, t).backward()
        static_e.grad = None
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static_loss = embedding_reg(static_e, t)
        static_loss.backward()
    for v, (ref_loss, ref_grad) in zip(values, eager):
        with torch.no_grad():
            static_e.copy_(v)                                            # the embedding changes in place between replays
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_loss.detach(), ref_loss) and torch.equal(static_e.grad, ref_grad)


def test_stale_table_raises_after_prune():
    from emd_amd.gaussian_model import GaussianModel
    from emd_amd.knn import embedding_reg
    m = GaussianModel(device=DEV)
    m.create_from_pcd(torch.rand(4000, 3, generator=torch.Generator().manual_seed(19)), torch.rand(4000, 3), 1.0)
    t = m.knn_table(20)
    embedding_reg(m.get_embedding, t)
    mask = torch.zeros(4000, dtype=torch.bool)
    mask[::4] = True
    m.prune_points(mask.to(DEV))
    assert m._xyz.shape[0] == 3000 and m._knn_table is None
    with pytest.raises(ValueError, match="stale table"):
        embedding_reg(m.get_embedding, t)
    t2 = m.knn_table(20)                                                 # the trainer's decision: build a new one
    assert t2 is not t and t2.N == 3000
    assert torch.isfinite(embedding_reg(m.get_embedding, t2))
    t.refresh(m.get_xyz)                                                 # or refresh the old one: N changed, so it reallocates
    assert t.N == 3000 and torch.equal(t.idx, t2.idx)


class TestTwoMillion:
    """N = 2 000 000 uniform in a 200 x 200 x 20 box: invariants on all rows, brute force on 1 024 queries."""

    @pytest.fixture(scope="class")
    def cloud(self):
        p = torch.rand(2_000_000, 3, generator=torch.Generator().manual_seed(20)) * torch.tensor([200.0, 200.0, 20.0])
        q = _sample(2_000_000, 1024, 21)
        return p.contiguous(), q

    @pytest.mark.parametrize("k", [3, 20])
    def test_two_million_uniform(self, cloud, k):
        p, q = cloud
        idx, d2 = _run(p, k)
        kc.check_invariants(p, idx, d2)
        worst = kc.check_against_brute(p, idx, d2, q, k)
        print(f"uniform 2M, k={k}: worst relative d2 error {worst:.3e}")
