"""Checkers of the k-NN / embedding-regulariser tests: restatements in torch fp64 on the CPU, never the code under test.  tests/test_knn_cpu.py
pins them against a plain-Python brute force; tests/test_knn_gpu.py uses them on the HIP results."""
import math

import torch

# fp32 d2 = dx^2 + dy^2 + dz^2 from fp32 coordinates against its fp64 value: one rounding of each difference (relative 2^-24, doubled by the
# square), one of each product and sum, no cancellation after the subtraction: at most about 4 * 2^-24 = 2.4e-7.  4 x headroom.
D2_RTOL = 1e-6


def brute_knn(points, queries, k, chunk=256):
    """points [N,3] fp32 (CPU), queries: LongTensor of row numbers -> (idx [Q,k'], d2 [Q,k'] fp64) with k' = min(k, N - 1), rows ascending;
    self excluded by index; rows with a non-finite coordinate are nobody's neighbour."""
    p = points.double()
    bad = ~torch.isfinite(p).all(dim=1)
    kk = min(k, p.shape[0] - 1)
    out_i, out_d = [], []
    for s in range(0, len(queries), chunk):
        q = queries[s:s + chunk]
        d = ((p[q][:, None, :] - p[None, :, :]) ** 2).sum(-1)
        d[:, bad] = math.inf
        d[torch.arange(len(q)), q] = math.inf
        dv, di = d.topk(kk, dim=1, largest=False)
        out_i.append(di)
        out_d.append(dv)
    return torch.cat(out_i), torch.cat(out_d)


def check_invariants(points, idx, d2):
    """What every row must satisfy whatever the ties: idx distinct, in range, never the row itself; d2 ascending and equal to the fp64 distance
    to idx within D2_RTOL (exactly 0 where that is 0); empty slots (-1, +inf) only at the end of a row."""
    p = points.double()
    n, k = idx.shape
    idx, d2 = idx.long().cpu(), d2.double().cpu()
    valid = idx >= 0
    assert (idx[valid] < n).all(), "index out of range"
    assert (idx != torch.arange(n)[:, None]).all(), "a row lists itself"
    assert torch.isinf(d2[~valid]).all() and (d2[~valid] > 0).all(), "an empty slot must hold +inf"
    assert (valid[:, :-1] | ~valid[:, 1:]).all(), "an empty slot in front of a filled one"
    assert (d2[:, 1:] >= d2[:, :-1]).all(), "a row does not ascend"
    srt = torch.where(valid, idx, -1 - torch.arange(k)[None, :].expand(n, k)).sort(dim=1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), "a row lists a point twice"
    for s in range(0, n, 1 << 18):
        i, v = idx[s:s + (1 << 18)], valid[s:s + (1 << 18)]
        ref = ((p[s:s + (1 << 18)][:, None, :] - p[i.clamp_min(0)]) ** 2).sum(-1)
        got = d2[s:s + (1 << 18)]
        assert (torch.abs(got - ref)[v] <= D2_RTOL * ref[v]).all(), "d2 is not the distance to idx"


def check_against_brute(points, idx, d2, queries, k):
    """The rows `queries` of (idx, d2) against the fp64 brute force: every distance within D2_RTOL, and where a row's reference distances
    (the k+1-th included) lie further apart than the tolerance the indices are the reference's exactly.  Returns the worst relative error."""
    n = points.shape[0]
    ri, rd = brute_knn(points, queries, k + 1)
    kk = min(k, n - 1, int(torch.isfinite(points).all(dim=1).sum().item()) - 1)
    gi, gd = idx[queries].long().cpu(), d2[queries].double().cpu()
    finite_q = torch.isfinite(points[queries]).all(dim=1)
    assert (gi[~finite_q] == -1).all() and torch.isinf(gd[~finite_q]).all(), "a non-finite query must get an empty row"
    gi, gd, ri, rd = gi[finite_q], gd[finite_q], ri[finite_q], rd[finite_q]
    kk = max(kk, 0)
    assert (gi[:, kk:] == -1).all() and torch.isinf(gd[:, kk:]).all(), "slots beyond the available neighbours must be empty"
    if kk == 0:
        return 0.0
    ref = rd[:, :kk]
    err = torch.abs(gd[:, :kk] - ref)
    assert (err <= D2_RTOL * ref).all(), f"d2 off by {float((err / ref.clamp_min(1e-300)).max()):.3e} relative"
    assert (gd[:, kk - 1] <= ref[:, kk - 1] * (1 + D2_RTOL)).all()
    gaps = rd[:, 1:] - rd[:, :-1]                                  # (k+1 reference distances where they exist: inf - x = inf is "apart")
    ng = min(kk, gaps.shape[1])
    apart = (gaps[:, :ng] > 2 * D2_RTOL * rd[:, :ng]).all(dim=1)
    assert (gi[apart][:, :kk] == ri[apart][:, :kk]).all(), "indices differ from the brute force on rows without ties"
    rel = err / ref.clamp_min(1e-300)
    return float(rel[ref > 0].max()) if (ref > 0).any() else 0.0


def check_reverse(idx, rev_start, rev_slot):
    idx, rev_start, rev_slot = idx.long().cpu(), rev_start.long().cpu(), rev_slot.long().cpu()
    n, k = idx.shape
    flat = idx.flatten()
    m = int((flat >= 0).sum())
    assert rev_start.shape[0] == n + 1 and rev_start[0] == 0 and rev_start[n] == m
    assert (rev_start[1:] >= rev_start[:-1]).all()
    slots = rev_slot[:m]
    assert torch.equal(slots.sort().values, torch.nonzero(flat >= 0).flatten()), "rev_slot is not a permutation of the filled slots"
    owner = torch.repeat_interleave(torch.arange(n), rev_start[1:] - rev_start[:-1])
    assert torch.equal(flat[slots], owner), "a slot is filed under the wrong point"
    same = owner[1:] == owner[:-1]
    assert (slots[1:][same] > slots[:-1][same]).all(), "slots do not ascend inside a point's list"


def reg_reference(e, idx, w):
    """weighted_l2_loss_v2(e[:, None, :], e[idx], w) in fp64 with autograd; entries with idx < 0 neither contribute nor count.
    -> (loss, dloss/de), both fp64."""
    e = e.detach().double().cpu().requires_grad_(True)
    idx, w = idx.long().cpu(), w.double().cpu()
    valid = idx >= 0
    diff2 = ((e[:, None, :] - e[idx.clamp_min(0)]) ** 2).sum(-1)
    terms = torch.sqrt(diff2 * w + 1e-20)
    loss = (terms * valid).sum() / valid.sum()
    loss.backward()
    return loss.detach(), e.grad


def clustered_points(n, seed, clusters=64, copies=1000):
    """The non-uniform cloud of the tests: `clusters` anisotropic clusters (sigma about 40 x 40 x 2 per centre, per-point spread 0 - 3), and the
    first `copies` points exact copies of the next `copies`."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(clusters, 3, generator=g) * torch.tensor([40.0, 40.0, 2.0])
    which = torch.randint(0, clusters, (n,), generator=g)
    spread = torch.rand(n, 1, generator=g) * 3.0
    p = (centres[which] + torch.randn(n, 3, generator=g) * spread).float()
    if copies:
        p[:copies] = p[copies:2 * copies]
    return p.contiguous()
