"""-m gpu: the role x mode x kind table of `emd_densify_gather` (csrc/densify.hip), driven directly with hand-written src / kind / split_rank
at the smallest shape that reaches every cell: 7 source rows, one call with COPY tensors of width 1 and 48, XYZ, SCALING, STATE (width 3) and a
ZERO column.  Expected values are a float64 restatement of the rules at EmdDensifyGather / EmdRefineArgs in include/emd_raster.h.  Copied
values, moments, statistics and unreduced scales bit-exact; reduced scales to rtol = atol = 2e-6 and sample coordinates to rtol 2e-6, atol 2e-5
(the bounds test_vanilla_refine_gpu.py's at-scale test applies to the same two quantities drawn from the same distributions)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N = 7
# mode -> (src, kind, split_rank, n_split, replicas)
#   DENSIFY: survivors 0 and 2, a clone of 2, the samples of the split rows 4 and 5: replica 0, then replica 1; rank inside the replica
#   PRUNE:   three survivors
#   REFINE:  unsplit original 0, split original 4, its three samples, a duplicate of the unsplit row 5, a duplicate of the split row 4
CASES = {"DENSIFY": ([0, 2, 2, 4, 5, 4, 5], [0, 0, 1, 2, 2, 3, 3], [0, 0, 0, 0, 1, 0, 1], 2, 2),
         "PRUNE": ([1, 3, 6], [0, 0, 0], [0, 0, 0], 0, 2),
         "REFINE": ([0, 4, 4, 4, 4, 5, 4], [0, 16, 2 | 16, 3 | 16, 4 | 16, 1, 1 | 16], [0] * 7, 1, 3)}
ROLES = ("COPY", "COPY", "XYZ", "SCALING", "STATE", "ZERO")
WIDTHS = (1, 48, 3, 3, 3, 1)


@pytest.fixture(scope="module")
def source():
    """The six source tensors (parameters drawn as the at-scale refinement test draws them) and a recorded draw [3, 2, 3]."""
    g = torch.Generator().manual_seed(5)
    xyz = torch.randn(N, 3, generator=g) * 4
    scaling = torch.log(torch.tensor(1e-3)) + torch.rand(N, 3, generator=g) * 8.0 - 1.0
    rotation = torch.randn(N, 4, generator=g)
    tensors = [torch.randn(N, 1, generator=g), torch.randn(N, 48, generator=g), xyz, scaling, torch.randn(N, 3, generator=g), torch.rand(N, 1, generator=g) + 0.5]
    return [t.to(DEV).contiguous() for t in tensors], rotation.to(DEV).contiguous(), torch.randn(3, 2, 3, generator=g).to(DEV)


def gather(source, mode, samples=None, seed=0, with_rank=True):
    """-> (return code, outputs); `samples` [replicas, n_split, 3] or None for the Philox draw."""
    from emd_amd import _lib as L
    tensors, rotation, _ = source
    src, kind, rank, n_split, _ = CASES[mode]
    I = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    src, kind, rank = I(src), I(kind), I(rank)
    a = L.EmdDensifyGather()
    a.num_out, a.num_tensors, a.mode, a.num_split = src.numel(), len(tensors), getattr(L, "DENSIFY_MODE_" + mode), n_split
    a.src, a.kind, a.scaling, a.rotation, a.seed = src.data_ptr(), kind.data_ptr(), tensors[3].data_ptr(), rotation.data_ptr(), seed
    if samples is not None:
        a.samples = samples.data_ptr()
    if with_rank:
        a.split_rank = rank.data_ptr()
    outs = [torch.full((src.numel(), w), float("nan"), device=DEV) for w in WIDTHS]
    for k, (t, out) in enumerate(zip(tensors, outs)):
        a.tensors[k].src, a.tensors[k].dst, a.tensors[k].width, a.tensors[k].role = t.data_ptr(), out.data_ptr(), WIDTHS[k], getattr(L, "DENSIFY_ROLE_" + ROLES[k])
    rc = L.load().emd_densify_gather(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, outs


def expected(source, mode, samples):
    """The header's rules in float64 -> (values per tensor, mask per tensor of the elements that are computed rather than copied)."""
    tensors, rotation, _ = source
    src, kind, rank, n_split, _ = CASES[mode]
    src, kind, rank = torch.tensor(src, device=DEV), torch.tensor(kind, device=DEV), torch.tensor(rank, device=DEV)
    base = kind & 15
    fresh, sample = (base != 0)[:, None], base >= 2
    reduced = ((kind & 16) != 0) if mode == "REFINE" else sample
    vals = [t.double()[src] for t in tensors]
    soft = [torch.zeros_like(v, dtype=torch.bool) for v in vals]
    q = rotation.double()[src]
    w, x, y, z = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    n = samples.double()[(base - 2).clamp(min=0), rank.clamp(max=max(n_split - 1, 0))] if n_split else torch.zeros_like(vals[2])
    moved = torch.bmm(R, (torch.exp(vals[3]) * n)[..., None]).squeeze(-1) + vals[2]          # from the scale BEFORE its reduction
    vals[2] = torch.where(sample[:, None], moved, vals[2])
    vals[3] = torch.where(reduced[:, None], torch.log(torch.exp(vals[3]) / 1.6), vals[3])
    soft[2], soft[3] = sample[:, None].expand(-1, 3), reduced[:, None].expand(-1, 3)
    vals[4] = torch.where(fresh, 0.0, vals[4])
    vals[5] = torch.zeros_like(vals[5]) if mode == "DENSIFY" else torch.where(fresh, 0.0, vals[5])
    return vals, soft


@pytest.mark.parametrize("mode", list(CASES))
def test_gather_table_with_recorded_samples(source, mode):
    from emd_amd import _lib as L
    n_split, replicas = CASES[mode][3:]
    samples = source[2][:replicas, :max(n_split, 1)].contiguous()
    rc, outs = gather(source, mode, samples)
    assert rc == L.EMD_OK
    vals, soft = expected(source, mode, samples)
    for k, (got, ref, s) in enumerate(zip(outs, vals, soft)):
        assert torch.equal(got[~s], ref.float()[~s]), (mode, k, ROLES[k])
        if s.any():
            assert ROLES[k] in ("XYZ", "SCALING")
            torch.testing.assert_close(got.double()[s], ref[s], rtol=2e-6, atol=2e-6 if ROLES[k] == "SCALING" else 2e-5, msg=lambda m: f"{mode} {ROLES[k]}: {m}")
    n_soft = {"DENSIFY": (12, 12), "PRUNE": (0, 0), "REFINE": (9, 15)}[mode]          # the table's cells are all reached
    assert (int(soft[2].sum()), int(soft[3].sum())) == n_soft


def test_philox_samples_repeat_and_are_one_path_for_both_projects(source):
    """samples = NULL: the draw is a function of (seed, source row, replica) alone -- two calls agree bit for bit, and a DENSIFY sample (kind 2 / 3)
    and a REFINE sample (kind 2|16 / 3|16) of the same source row 4 and replica receive the same coordinates."""
    from emd_amd import _lib as L
    (rc0, d0), (rc1, d1), (rc2, r) = gather(source, "DENSIFY", seed=99), gather(source, "DENSIFY", seed=99), gather(source, "REFINE", seed=99)
    assert rc0 == rc1 == rc2 == L.EMD_OK
    assert all(torch.equal(a, b) for a, b in zip(d0, d1))
    assert torch.equal(d0[2][3], r[2][2]) and torch.equal(d0[2][5], r[2][3])
    xyz = source[0][2]
    assert not torch.equal(d0[2][3], xyz[4]) and not torch.equal(d0[2][3], d0[2][5]) and bool(torch.isfinite(r[2]).all())
    assert not torch.equal(gather(source, "DENSIFY", seed=100)[1][2][3], d0[2][3])


def test_samples_without_split_rank_are_refused(source):
    from emd_amd import _lib as L
    rc, _ = gather(source, "DENSIFY", source[2][:2].contiguous(), with_rank=False)
    assert rc == L.EMD_ERR_INVALID
