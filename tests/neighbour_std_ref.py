"""Checkers of the neighbour-std regulariser and the segmented k-NN (EmdNeighbourStdArgs / emd_knn_segments, include/emd_raster.h): restatements
in torch fp64 on the CPU, never the code under test.  tests/test_neighbour_std_cpu.py pins them against plain Python; the GPU tests use them on the
HIP results.

Tolerance of a term.  u = 2^-24.  The kernel works on v = fp32 act(x) where the reference has the exact V: |v - V| <= A u |V| with A = 0
(identity), 2 (expf: 1 ulp) and 4 (sigmoid = 1 / (1 + expf(-x)): expf 2u, the sum and the quotient u each).  A difference d_m = fl(v_m - v_n) adds
one rounding of |v_m - v_n| <= 2 max|v|.  The standard deviation does not see a common shift, so the members' perturbations are at most
(A + 2) u max|v| each, and sigma moves by at most sqrt(g / (g - 1)) <= sqrt(2) times that.  What follows (the mean -- its own error is a shift,
second order --, g differences to it, squares, g additions, a quotient, a root) is (g / 2 + 3) u RELATIVE TO sigma: with the input condition
sigma >= 2^-10 max|v| below 0.02 of the unit u max|v| for g <= 33, counted as 1 together with the fp64 sum and the final rounding to fp32.
    roundings(act) = ceil(sqrt(2) (A + 2) + 1) = 4, 7, 10        of size u max|v| <= 2^-14 sigma
and a term, a mean of sigmas that are either exactly 0 (bit-identical members) or satisfy the input condition, is checked relative to the
reference at FOUR times that: term_rtol(act) = 4 roundings 2^-14 (9.8e-4, 1.7e-3, 2.4e-3).
The tight case (identity, all values within a factor 2 of each other, so every difference is exact by Sterbenz) has no such unit: its bound is
the (g / 2 + 3) u relative to sigma, 8 roundings for g <= 10, checked at 4 * 8 * 2^-24 = 1.9e-6.
Gradients: the project's rule, element-wise 1e-4 |ref| + 1e-6 max|ref| and relative L2 <= 1e-5, per block."""
import math

import torch

from tests import knn_checks as kc

ACT = {"identity": lambda x: x, "exp": torch.exp, "sigmoid": torch.sigmoid}
ACT_INV = {"identity": lambda v: v, "exp": torch.log, "sigmoid": torch.logit}
ROUNDINGS = {"identity": 4, "exp": 7, "sigmoid": 10}
FLOOR = 2.0 ** -10                      # the input condition: sigma >= FLOOR * max|v| over the group, or bit-identical members
TIGHT_RTOL = 4 * 8 * 2.0 ** -24


def term_rtol(act):
    return 4 * ROUNDINGS[act] * 2.0 ** -14


def _groups(idx):
    """idx [N,k] -> members [N,1+k] (self first, the filled slots next in their order, clamped fillers last), g [N]."""
    idx = idx.long().cpu()
    n = idx.shape[0]
    valid = (idx >= 0) & (idx < n)
    order = torch.argsort((~valid).long(), dim=1, stable=True)
    idx, valid = torch.gather(idx, 1, order), torch.gather(valid, 1, order)
    members = torch.cat([torch.arange(n)[:, None], idx.clamp(0, max(n - 1, 0))], dim=1)
    return members, 1 + valid.sum(dim=1)


def _sigma(v, members, g):
    """v [N,C] fp64 -> sigma [N,C]: torch.std over each group's members, groups of one give 0."""
    out = torch.zeros_like(v)
    for size in torch.unique(g).tolist():
        if size < 2:
            continue
        rows = torch.nonzero(g == size).flatten()
        out = out.index_add(0, rows, v[members[rows, :size]].std(dim=1))       # (std_backward returns 0 for a constant group)
    return out


def reference(blocks, idx, weights, acts, g_terms=None):
    """-> (terms [B] fp64, [d loss / d block or None where the weight is 0]) with loss = sum g_terms[b] terms[b] (g_terms default ones)."""
    members, g = _groups(idx)
    n = members.shape[0]
    xs = [b.detach().double().cpu().reshape(n, -1).requires_grad_(True) for b in blocks]
    terms = []
    for x, w, a in zip(xs, weights, acts):
        terms.append(float(w) * _sigma(ACT[a](x), members, g).sum() / (n * x.shape[1]) if w != 0 else torch.zeros((), dtype=torch.float64))
    terms = torch.stack(terms)
    gt = torch.ones(len(xs), dtype=torch.float64) if g_terms is None else g_terms.detach().double().cpu()
    loss = (terms * gt).sum()
    if loss.requires_grad:
        loss.backward()
    grads = [None if w == 0 else (x.grad if x.grad is not None else torch.zeros_like(x)).reshape(b.shape) for x, w, b in zip(xs, weights, blocks)]
    return terms.detach(), grads


def emulate_fp32(blocks, idx, weights, acts, g_terms=None):
    """The contract's operation order in torch fp32 on the CPU (the point first, then ascending j; the shifted two-pass form; no fused
    multiply-adds; the sigmas added in fp64).  The backward adds a point's own group first and the others slot column by slot column, which is
    not the ascending order of rev(j): an emulation of the arithmetic, not of the bits.  -> (terms [B] fp64, grads fp32)."""
    idx = idx.long().cpu()
    n, k = idx.shape
    valid = (idx >= 0) & (idx < n)
    g = (1 + valid.sum(dim=1)).float()[:, None]
    gt = torch.ones(len(blocks)) if g_terms is None else g_terms.detach().float().cpu()
    terms, grads = [], []
    for bi, (b, w, a) in enumerate(zip(blocks, weights, acts)):
        if w == 0:
            terms.append(0.0)
            grads.append(None)
            continue
        x = b.detach().float().cpu().reshape(n, -1)
        C = x.shape[1]
        v = {"identity": x, "exp": torch.exp(x), "sigmoid": 1.0 / (1.0 + torch.exp(-x))}[a]
        d = [torch.where(valid[:, j:j + 1], v[idx[:, j].clamp(0, n - 1)] - v, torch.zeros_like(v)) for j in range(k)]
        s = torch.zeros_like(v)
        for j in range(k):
            s = s + d[j]
        mu = s / g
        q = (0.0 - mu) * (0.0 - mu)
        for j in range(k):
            e = d[j] - mu
            q = q + torch.where(valid[:, j:j + 1], e * e, torch.zeros_like(e))
        many = (g >= 2).expand_as(q)
        sigma = torch.where(many, torch.sqrt(q / (g - 1).clamp_min(1)), torch.zeros_like(q))
        mu = torch.where(many, mu, torch.zeros_like(mu))
        inv = torch.where(sigma > 0, 1.0 / ((g - 1) * sigma), torch.zeros_like(sigma))
        terms.append(float(w) * float(sigma.double().sum()) / (n * C))
        acc = (0.0 - mu) * inv
        for j in range(k):
            rows = torch.nonzero(valid[:, j]).flatten()
            tgt = idx[rows, j]
            acc = acc.index_add(0, tgt, ((v[tgt] - v[rows]) - mu[rows]) * inv[rows])
        scale = torch.tensor(float(gt[bi]) * float(w) / (n * C), dtype=torch.float64).float()
        da = {"identity": torch.ones_like(v), "exp": v, "sigmoid": v * (1.0 - v)}[a]
        grads.append((da * (scale * acc)).reshape(b.shape))
    return torch.tensor(terms, dtype=torch.float64), grads


def conditions(blocks, idx, acts, floor=FLOOR):
    """-> per block a bool [N,C]: True where the group of (n, c) is neither bit-identical nor at sigma >= floor * max|v| (fp32 activations, as the
    kernel sees them; sigma and the maximum in fp64)."""
    members, g = _groups(idx)
    n = members.shape[0]
    pos = torch.arange(members.shape[1])[None, :] < g[:, None]
    out = []
    for b, a in zip(blocks, acts):
        v = ACT[a](b.detach().float().cpu().reshape(n, -1)).double()
        vm = v[members]                                                        # [N,1+k,C]
        same = ((vm == vm[:, :1]) | ~pos[:, :, None]).all(dim=1)
        big = torch.where(pos[:, :, None], vm.abs(), torch.zeros_like(vm)).amax(dim=1)
        out.append(~same & (_sigma(v, members, g) < floor * big))
    return out


def assert_conditions(blocks, idx, acts, floor=FLOOR):
    for bi, bad in enumerate(conditions(blocks, idx, acts, floor)):
        assert not bool(bad.any()), f"block {bi}: {int(bad.sum())} (group, column) pairs below sigma >= {floor:.3e} max|v| and not identical"


def settle(blocks, idx, acts, floor=FLOOR, rounds=40, seed=0):
    """Move the owners of the offending (group, column) pairs -- in the activated value, by +-4 floor max|v| sqrt(g) -- until `conditions` holds
    everywhere.  -> new fp32 tensors of the same shapes.  A block whose members are all identical is never touched."""
    members, g = _groups(idx)
    n = members.shape[0]
    pos = torch.arange(members.shape[1])[None, :] < g[:, None]
    gen = torch.Generator().manual_seed(seed)
    out = [b.detach().float().cpu().clone() for b in blocks]
    for _ in range(rounds):
        bad = conditions(out, idx, acts, floor)
        if not any(bool(b.any()) for b in bad):
            return out
        for bi, (x, a) in enumerate(zip(out, acts)):
            if not bool(bad[bi].any()):
                continue
            flat = x.reshape(n, -1)
            v = ACT[a](flat.double())
            big = torch.where(pos[:, :, None], v[members].abs(), torch.zeros(1, dtype=torch.float64)).amax(dim=1)
            sign = torch.where(torch.rand(flat.shape, generator=gen) < 0.5, -1.0, 1.0).double()
            if a != "identity":
                sign = torch.where(v + 4 * floor * big * g[:, None].double().sqrt() * sign <= 0, torch.ones_like(sign), sign)      # stay inside the range
                if a == "sigmoid":
                    sign = torch.where(v + 4 * floor * big * g[:, None].double().sqrt() * sign >= 1, -torch.ones_like(sign), sign)
            moved = ACT_INV[a](v + 4 * floor * big * g[:, None].double().sqrt() * sign).float()
            out[bi] = torch.where(bad[bi], moved, flat).reshape(x.shape)
    raise AssertionError("settle did not converge")


def grad_close(got, ref, what=""):
    got, ref = got.detach().cpu().double(), ref.double()
    if float(ref.abs().max()) == 0.0:                                        # (a block of identical members: exactly zero, not merely small)
        assert torch.count_nonzero(got) == 0, what
        return 0.0
    err = torch.abs(got - ref)
    bound = 1e-4 * torch.abs(ref) + 1e-6 * torch.abs(ref).max()              # the standing gradient criterion
    l2 = float(torch.linalg.norm(got - ref) / torch.linalg.norm(ref))
    worst = float((err / bound).max())
    print(f"{what}: gradient worst err / bound {worst:.3f}, relative L2 {l2:.3e}")
    assert (err <= bound).all(), (what, worst)
    assert l2 <= 1e-5, (what, l2)
    return worst


def terms_close(got, ref, acts, weights, what="", rtol=None):
    got, ref = got.detach().cpu().double(), ref.double()
    for b, (a, w) in enumerate(zip(acts, weights)):
        tol = term_rtol(a) if rtol is None else rtol
        rel = abs(float(got[b]) - float(ref[b])) / abs(float(ref[b])) if float(ref[b]) != 0 else abs(float(got[b]))
        print(f"{what}: term {b} ({a}, w={w}) {float(got[b]):.9e} ref {float(ref[b]):.9e} rel {rel:.3e} (tolerance {tol:.3e})")
        if w == 0:
            assert float(got[b]) == 0.0
        assert rel <= tol, (what, b, rel, tol)


# ---- segments -------------------------------------------------------------------------------------------------------------------------------------
SEGMENT_SIZES = (0, 1, 2, 3, 63, 64, 65, 257, 300)          # and the rest


def segment_table(n=1500, lead=5, tail=7):
    """The table of the tests: `lead` rows in front of the first segment and `tail` behind the last belong to nobody; ten segments of the sizes
    0, 1, 2, 3, 63, 64, 65, 257, 300 and the rest.  -> LongTensor [11]."""
    rest = n - lead - tail - sum(SEGMENT_SIZES)
    assert rest > 300
    sizes = torch.tensor(SEGMENT_SIZES + (rest,))
    return torch.cat([torch.tensor([lead]), lead + sizes.cumsum(0)])


def segment_knn(points, segment_start, k):
    """The contract of emd_knn_segments in fp64: -> (idx [N,k] int64, d2 [N,k] fp64), -1 / +inf in the empty slots, global row numbers, the lower
    row first among equidistant candidates (a stable sort of distances listed in row order)."""
    n = points.shape[0]
    p = points.double()
    finite = torch.isfinite(p).all(dim=1)
    idx = torch.full((n, k), -1, dtype=torch.int64)
    d2 = torch.full((n, k), math.inf, dtype=torch.float64)
    seg = segment_start.long().clamp(0, n).tolist()
    for lo, hi in zip(seg[:-1], seg[1:]):
        if hi - lo < 2:
            continue
        q = p[lo:hi]
        d = ((q[:, None, :] - q[None, :, :]) ** 2).sum(-1)
        d[:, ~finite[lo:hi]] = math.inf
        d[~finite[lo:hi], :] = math.inf
        d.fill_diagonal_(math.inf)
        dv, di = torch.sort(d, dim=1, stable=True)
        kk = min(k, hi - lo - 1)
        filled = torch.isfinite(dv[:, :kk])
        idx[lo:hi, :kk] = torch.where(filled, di[:, :kk] + lo, -1)
        d2[lo:hi, :kk] = dv[:, :kk]
    return idx, d2


def check_segments(points, segment_start, idx, d2, k):
    """emd_knn_segments' result against the project's checkers, segment by segment: the invariants on every row, every neighbour inside its
    row's segment, `check_against_brute` (D2_RTOL, the near-tie rule) on each segment's own cloud, rows outside the segments empty.
    Returns the worst relative distance error."""
    n = points.shape[0]
    idx, d2 = idx.long().cpu(), d2.cpu()
    kc.check_invariants(points, idx, d2)
    seg = segment_start.long().clamp(0, n).tolist()
    owned = torch.zeros(n, dtype=torch.bool)
    worst = 0.0
    for lo, hi in zip(seg[:-1], seg[1:]):
        if hi <= lo:
            continue
        owned[lo:hi] = True
        rows = idx[lo:hi]
        assert ((rows == -1) | ((rows >= lo) & (rows < hi))).all(), f"a neighbour outside the segment [{lo}, {hi})"
        local = torch.where(rows >= 0, rows - lo, rows)
        worst = max(worst, kc.check_against_brute(points[lo:hi], local, d2[lo:hi], torch.arange(hi - lo), k))
    assert (idx[~owned] == -1).all() and torch.isinf(d2[~owned]).all(), "a row outside every segment must be empty"
    return worst
