"""float64 reference of the HexPlane lookup, with per-entry error bounds, and the exact-lattice cases that the edge tests run.
TEST INFRASTRUCTURE ONLY (tests/test_hexplane_ref_cpu.py proves it, tests/test_hexplane_edges_gpu.py uses it).

The definition (S3Gaussian/scene/hexplane.py:18-110, grid_sample with bilinear taps, align_corners, border padding), written out with explicit taps:
    q      = (p - lo) * (2 / (hi - lo)) - 1                    the time is used as given
    v      = (q + 1) * (size - 1) / 2                          per axis and scale
    v      clipped to [0, size - 1]; the slope dv/dq is (size - 1) / 2, and 0 where clipped (v <= 0 or v >= size - 1)
    i0     = floor(v), i1 = min(i0 + 1, size - 1), f = v - i0
    f_p    = sum_k w_k tap_k                                   plane p = (ax, ay) of PAIRS, [1, C, H = size_ay, W = size_ax]; the four taps (x0|x1, y0|y1)
                                                               with weights (1-fx)(1-fy), fx (1-fy), (1-fx) fy, fx fy
    out    = prod_p f_p, the scales side by side
Inputs are the float32 arrays the kernels get, converted to float64; nothing is rounded afterwards.

Beside every result stands its MAGNITUDE: the same expression with every term taken absolute (a feature: prod_p sum_k |w_k tap_k|; a gradient entry:
sum |term|, each factor f_q of a term replaced by sum_k |w_k tap_k|).  Rounding errors of fp32 arithmetic are relative to the magnitude, not to the
value: with signed planes, or in dL/dpts, whose terms are differences of taps, the value may cancel to far less.

The bounds, u = 2^-24 (`bound_feature`, `bound_point`, `bound_plane`, `bound_time_sum`):
    feature entry                          |got - ref| <= K_FEATURE  u magnitude
    dL/dpts, dL/dtimes entry               |got - ref| <= K_GRADIENT u magnitude
    plane entry reached by m taps          |got - ref| <= (K_GRADIENT + m) u sum |term|
    the sum of dL/dtimes over N points     |got - ref| <= (K_GRADIENT + N) u sum |term|
m (N) bounds the rounding of an fp32 sum of m (N) terms in ANY order -- float atomics give none.  A tap whose term is exactly zero (weight 0: the
clamped neighbour at a face, a point on a node; or a zero row of dL/dout) adds nothing and is not counted; an entry without a counted tap has magnitude
0, so its bound is 0: it must be exactly zero.  Likewise a dL/dpts / dL/dtimes entry whose coordinate is clipped on every scale.

The count behind K (first order in u; every rounding is taken at its worst, relative to the magnitude of what it rounds; a fused multiply-add only
removes roundings).  On the lattice inputs q, v, f and 1 - f are exact; off the lattice 1 - f costs one rounding more per weight, which the margins hold.
  one plane, f_p:         a weight (1-fx)(1-fy): 1 product (+ 2 for 1 - f off the lattice) = 3; tap * weight: 1; the three adds of the four products: 3   ->  7
                          (through the time tables: blend v0 (1-ft) + v1 ft = 3, then t0 (1-fx) + t1 fx = 3                                              ->  6)
  a feature:              six f_p: 42; the five products (and the one by 1): 6                                                                        ->  48 <= K_FEATURE = 64
  gi_p = go (pre suf):    five f_q: 35; four products inside pre / suf, their product, the one by go: 6                                               ->  41
  a plane term gi_p w_k:  gi_p: 41; the weight: 3; their product: 1                                                                                   ->  45
                          (the aggregating kernel forms the row as gi - gi fx, then x - x fy, each ONE fused multiply-add under the default contraction
                          -- as a product and a subtraction the row would be rounded relative to gi, not to itself --: 2 instead of 4; its windows
                          are fp64, their sum is rounded to fp32 once: 1; the marginal flush multiplies by 1 - ft: 2.  Its f_p are two levels of
                          a + f (b - a): the difference is rounded relative to |a| + |b|, the fused sum to the result: (2 + r) a level against the
                          level's magnitude, r = max |tap| / min |tap| of the footprint, for taps of one sign; r <= 4.4 for planes in [0.3, 1.3]:
                          f_p 12.8, five of them and the six products 70, the row 5: 75; its point term 70 + 22 = 92                           ->  <= K_GRADIENT.
                          For signed planes r has no bound: there the count does not cover that kernel's worst case, and the signed case
                          measures what it does -- DESIGN.md section 8.17)
  a point term gi_p slope: gi_p: 41; the slope ((ne - nw)(1 - fy) + (se - sw) fy) ds: 2 differences, 2 weights, 2 products, 1 add, 1 product = 5
                          (the roundings of a line in parallel count once); the product: 1; the sum over planes, scales (3 S <= 9 adds) and channel
                          lanes (log2 C <= 6 adds): 15; the product with 2 / (hi - lo): 1                                                            ->  63 <= K_GRADIENT = 96
K_FEATURE = 64 and K_GRADIENT = 96 are the next round figures above the counts; they are not fitted to any kernel's output.
"""
import itertools
import types

import numpy as np

PAIRS = list(itertools.combinations(range(4), 2))
U = 2.0 ** -24
K_FEATURE = 64
K_GRADIENT = 96


def bound_feature(mag):
    return K_FEATURE * U * mag


def bound_point(mag):
    return K_GRADIENT * U * mag


def bound_plane(mag, m):
    return (K_GRADIENT + m) * U * mag


def bound_time_sum(mag, n_points):
    return (K_GRADIENT + n_points) * U * mag


def axis_taps(q, size):
    """One axis of a tap for coordinates q (float64): i0, i1, f and the slope dv/dq (0 where clipped)."""
    s = 0.5 * (size - 1)
    v = (q + 1.0) * s
    low = ~(v > 0.0)
    high = ~low & ~(v < size - 1.0)
    v = np.where(low, 0.0, np.where(high, size - 1.0, v))
    ds = np.where(low | high, 0.0, s)
    i0 = np.floor(v)
    f = v - i0
    i0 = i0.astype(np.int64)
    return i0, np.minimum(i0 + 1, size - 1), f, ds


def normalise(pts, times, lo, hi):
    """[N, 4] float64: box-normalised x, y, z and the time (one timestamp is broadcast)."""
    pts = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    lo, hi = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    t = np.asarray(times, np.float32).astype(np.float64).reshape(-1)
    if t.size == 1 and pts.shape[0] != 1:
        t = np.broadcast_to(t, (pts.shape[0],))
    return np.concatenate([(pts - lo) * (2.0 / (hi - lo)) - 1.0, t[:, None]], axis=1)


def hexplane_ref(pts, times, lo, hi, res, planes, gout, terms=False):
    """pts [N, 3], times [N] / [N, 1] or ONE timestamp, lo / hi [3] (aabb[0] / aabb[1]), res[s] = [rx, ry, rz, rt], planes[s][p] = [1, C, H, W],
    gout [N, S C] = dL/dout.  Returns a namespace:
      feat, feat_mag [N, S C];  dpts, dpts_mag [N, 3];  dtimes, dtimes_mag [N];  dtime_sum, dtime_sum_mag (the broadcast form)
      clipped [N, 4]: the (point, axis) pairs clipped on every scale
      planes[s][p] = namespace(g, mag [1, C, H, W], m int64 [1, C, H, W] (taps with a non-zero term), untouched = (m == 0))
      with `terms`: planes[s][p].terms = (flat entry index into [C, H, W], |term|) of every counted tap."""
    q = normalise(pts, times, lo, hi)
    N, S = q.shape[0], len(res)
    C = planes[0][0].shape[1]
    gout = np.asarray(gout, np.float32).astype(np.float64).reshape(N, S * C)
    lo64, hi64 = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    chain = np.concatenate([2.0 / (hi64 - lo64), [1.0]])
    feat, feat_mag = np.zeros((N, S * C)), np.zeros((N, S * C))
    dq, dq_mag = np.zeros((N, 4)), np.zeros((N, 4))
    clipped = np.ones((N, 4), bool)
    out_planes = []
    for s in range(S):
        ax_t = [axis_taps(q[:, k], int(res[s][k])) for k in range(4)]
        for k in range(4):
            clipped[:, k] &= ax_t[k][3] == 0.0
        f, fm, taps, wts, locs = [], [], [], [], []
        for p, (ax, ay) in enumerate(PAIRS):
            P = np.asarray(planes[s][p], np.float32).astype(np.float64)[0]              # [C, H, W]
            assert P.shape == (C, int(res[s][ay]), int(res[s][ax])), (s, p, P.shape)
            x0, x1, fx, _ = ax_t[ax]
            y0, y1, fy, _ = ax_t[ay]
            loc = [(x0, y0), (x1, y0), (x0, y1), (x1, y1)]
            w = [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]
            T = [P[:, y, x].T for x, y in loc]                                           # [N, C] each
            f.append(sum(wk[:, None] * Tk for wk, Tk in zip(w, T)))
            fm.append(sum(wk[:, None] * np.abs(Tk) for wk, Tk in zip(w, T)))
            taps.append(T); wts.append(w); locs.append(loc)
        go = gout[:, s * C:(s + 1) * C]
        feat[:, s * C:(s + 1) * C] = np.prod(f, axis=0)
        feat_mag[:, s * C:(s + 1) * C] = np.prod(fm, axis=0)
        row = []
        for p, (ax, ay) in enumerate(PAIRS):
            others = [r for r in range(6) if r != p]
            gi = go * np.prod([f[r] for r in others], axis=0)
            gim = np.abs(go) * np.prod([fm[r] for r in others], axis=0)
            H, W = int(res[s][ay]), int(res[s][ax])
            G, M, cnt = np.zeros((H, W, C)), np.zeros((H, W, C)), np.zeros((H, W, C), np.int64)
            tl = []
            for (x, y), wk in zip(locs[p], wts[p]):
                np.add.at(G, (y, x), gi * wk[:, None])
                am = gim * wk[:, None]
                np.add.at(M, (y, x), am)
                np.add.at(cnt, (y, x), (am != 0.0).astype(np.int64))
                if terms:
                    flat = (np.arange(C)[None, :] * H + y[:, None]) * W + x[:, None]
                    keep = am != 0.0
                    tl.append((flat[keep], am[keep]))
            rec = types.SimpleNamespace(g=G.transpose(2, 0, 1)[None], mag=M.transpose(2, 0, 1)[None], m=cnt.transpose(2, 0, 1)[None])
            rec.untouched = rec.m == 0
            if terms:
                rec.terms = (np.concatenate([t[0] for t in tl]), np.concatenate([t[1] for t in tl]))
            row.append(rec)
            # the slopes along the plane's two axes: differences of taps, blended along the other axis, times the clip mask
            T00, T10, T01, T11 = taps[p]
            fx, dsx, fy, dsy = ax_t[ax][2][:, None], ax_t[ax][3][:, None], ax_t[ay][2][:, None], ax_t[ay][3][:, None]
            a00, a10, a01, a11 = (np.abs(t) for t in taps[p])
            dq[:, ax] += (gi * ((T10 - T00) * (1 - fy) + (T11 - T01) * fy) * dsx).sum(1)
            dq[:, ay] += (gi * ((T01 - T00) * (1 - fx) + (T11 - T10) * fx) * dsy).sum(1)
            dq_mag[:, ax] += (gim * ((a10 + a00) * (1 - fy) + (a11 + a01) * fy) * dsx).sum(1)
            dq_mag[:, ay] += (gim * ((a01 + a00) * (1 - fx) + (a11 + a10) * fx) * dsy).sum(1)
        out_planes.append(row)
    dq, dq_mag = dq * chain, dq_mag * np.abs(chain)
    return types.SimpleNamespace(feat=feat, feat_mag=feat_mag, dpts=dq[:, :3], dpts_mag=dq_mag[:, :3], dtimes=dq[:, 3], dtimes_mag=dq_mag[:, 3],
                                 dtime_sum=dq[:, 3].sum(), dtime_sum_mag=dq_mag[:, 3].sum(), clipped=clipped, planes=out_planes, N=N, C=C, S=S)


def check_against(ref, feat, dpts, dtimes, planes, what=""):
    """Every entry of a result (numpy arrays, or None for what was not computed; `dtimes`: [N] values or the one sum) against `ref` under the bounds, no
    entry left out, and the two exact-zero conditions.  Returns the worst error / bound per quantity (entries with bound 0 must be exact and count as 0)."""
    worst = {}

    def one(name, got, want, bound, zero=None):
        got = np.asarray(got, np.float64).reshape(want.shape)
        err = np.abs(got - want)
        assert np.isfinite(got).all(), (what, name, "non-finite")
        bad = err > bound
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
        if zero is not None:
            assert (got[zero] == 0.0).all(), (what, name, "an entry that must be exactly zero is", got[zero][got[zero] != 0.0][:4])
        if bad.any():
            i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0.0)), err.shape)
            raise AssertionError((what, name, "entry", i, "got", got[i], "ref", want[i], "error", err[i], "bound", bound[i], "entries outside", int(bad.sum())))
        worst[name] = max(worst.get(name, 0.0), float(ratio.max()) if ratio.size else 0.0)

    if feat is not None:
        one("feat", feat, ref.feat, bound_feature(ref.feat_mag))
    if dpts is not None:
        one("dpts", dpts, ref.dpts, bound_point(ref.dpts_mag), ref.clipped[:, :3])
    if dtimes is not None:
        dtimes = np.asarray(dtimes, np.float64).reshape(-1)
        if dtimes.size == ref.N:
            one("dtimes", dtimes, ref.dtimes, bound_point(ref.dtimes_mag), ref.clipped[:, 3])
        else:
            assert dtimes.size == 1
            one("dtimes", dtimes, np.array([ref.dtime_sum]), np.array([bound_time_sum(ref.dtime_sum_mag, ref.N)]), np.array([bool(ref.clipped[:, 3].all())]))
    if planes is not None:
        for s in range(ref.S):
            for p in range(6):
                r = ref.planes[s][p]
                one("planes", planes[s * 6 + p], r.g, bound_plane(r.mag, r.m), r.untouched)
    return worst


# ---- inputs on an exact lattice ----------------------------------------------------------------------------------------------------------------
# Box extents are powers of two, box-normalised coordinates and times are k / 1024, resolutions are <= 129: q, v = (q + 1)(size - 1) / 2, floor(v) and
# the fraction are then exact in float32, with or without a fused multiply-add in q (`lattice_is_exact`), so kernel and reference see the same cell and
# the same fraction at every point and no tolerance has to absorb a coordinate's rounding.
LATTICE = 1024
BOX_INVERTED = ((2.0, -1.0, 4.0), (-2.0, 3.0, -4.0))       # HexPlaneField's orientation (aabb[0] = +bounds), non-cubic
BOX_FORWARD = ((-1.0, -2.0, 0.0), (1.0, 2.0, 8.0))         # lo < hi, non-cubic


def _cell(res_axis):
    """lattice steps per cell of an axis of that resolution"""
    assert (2 * LATTICE) % (res_axis - 1) == 0
    return 2 * LATTICE // (res_axis - 1)


def _nodes_faces(rng):
    nodes = [-LATTICE + 128 * j for j in range(17)]                        # the nodes of res - 1 = 16 (and of 8, 4, 2, 1), both faces among them
    cand = nodes + [-LATTICE + 1, -LATTICE - 1, LATTICE - 1, LATTICE + 1, -3000, 3000, -2 * LATTICE, 2 * LATTICE, 64, -192, 341]
    tcand = [-LATTICE, -512, 0, 512, LATTICE, -LATTICE - 1, LATTICE + 1, -LATTICE + 1, LATTICE - 1, -1100, 1100, -2048, 2048, -256, 768, 100]
    L, n = len(cand), 1024
    k = np.zeros((n, 4), np.int64)
    i = np.arange(n)
    for a, shift in enumerate((0, 5, 11)):                                    # every candidate on every axis ...
        k[:, a] = np.asarray(cand)[(i + shift) % L]
    k[:, 3] = np.asarray(tcand)[i % len(tcand)]
    free = rng.random((n, 4)) < 0.5                                           # ... among points whose other coordinates are anywhere on the lattice
    free[:L] = False
    free[L:2 * L, 0] = False
    free[2 * L:3 * L, 1] = False
    free[3 * L:4 * L, 2] = False
    return np.where(free, rng.integers(-1100, 1101, (n, 4)), k)


def _run(start, step, count=256):
    return start + step * np.arange(count)


def _layout(name, rng):
    """-> (box, res, k [N, 4] lattice numerators of x, y, z, t, identity: whether the seam needs the points visited as laid out)"""
    if name in ("nodes_inverted", "nodes_forward"):
        # res - 1: 16, 8, 4, 2 | 32, 1, 6, 0 (one axis of six cells, a time axis of ONE node) | 2, 16, 8, 4
        return (BOX_INVERTED if name == "nodes_inverted" else BOX_FORWARD), [[17, 9, 5, 3], [33, 2, 7, 1], [3, 17, 9, 5]], _nodes_faces(rng), False
    if name.startswith("window_"):
        # a run of 256 points along one axis over ten cells (2 .. 11) of a resolution-17 axis: the 7 x 7 window of the block holds cells 2 .. 8, a footprint
        # with x0 = 8 straddles its edge, cells 9 .. 11 lie outside; the other axes stay within two cells.  A second block: the same, half a cell on
        axis = "xyz".index(name[-1])
        c = _cell(17)
        k = np.zeros((512, 4), np.int64)
        for b in range(2):
            sl = slice(256 * b, 256 * b + 256)
            for a in range(3):
                k[sl, a] = _run(-LATTICE + 2 * c + 3 + b * (c // 2), 5) if a == axis else -LATTICE + 5 * c + 7 + 37 * ((np.arange(256) * (3 + a)) % 6)
            k[sl, 3] = np.asarray([-700, -300, 40, 0, 512, 900])[np.arange(256) % 6]
        return BOX_INVERTED, [[17, 17, 17, 5], [5, 5, 5, 3]], k, True
    if name == "time_uniform":
        # blocks with ONE time each over 24 cells of resolution-33 axes (marginal windows hold 19): the time on a node (ft == 0), inside a cell, on the
        # upper face (clipped, i1 == i0)
        k = np.zeros((768, 4), np.int64)
        for b, t in enumerate((0, 100, LATTICE)):
            for a in range(3):
                k[256 * b:256 * b + 256, a] = _run(-LATTICE + (2 + a) * _cell(33) + 5 + 3 * b, 6)
            k[256 * b:256 * b + 256, 3] = t
        return BOX_INVERTED, [[33, 33, 33, 5]], k, True
    if name == "time_mixed":
        # times over all four cells of a resolution-5 time axis, on its faces and beyond, in a block that spans 12 cells of resolution-33 axes: rows leave
        # the 9 x 2 windows in x and in t
        k = np.zeros((512, 4), np.int64)
        for b in range(2):
            for a in range(3):
                k[256 * b:256 * b + 256, a] = _run(-LATTICE + (3 + a) * _cell(33) + 9 + b, 3)
            k[256 * b:256 * b + 256, 3] = np.asarray([-900, -300, 200, 700, LATTICE, -LATTICE, 1500, 0, -512])[(np.arange(256) * 5 + b) % 9]
        return BOX_INVERTED, [[33, 33, 33, 5], [9, 9, 9, 3]], k, True
    if name in ("zero_uniform", "zero_signed"):
        # one time, 0.0, for the whole block; `zero_signed` writes ONE of them as -0.0 (`make_case`): two keys in the block's min / max, the mixed-time path
        k = np.zeros((256, 4), np.int64)
        for a in range(3):
            k[:, a] = _run(-LATTICE + (4 + a) * _cell(17) + 11, 2)
        return BOX_INVERTED, [[17, 17, 17, 5], [9, 9, 9, 3]], k, True
    if name == "deferred_time":
        # a deferred scale: 80 cells of resolution-129 axes in a run of 256 (its time windows hold 68)
        k = np.zeros((512, 4), np.int64)
        for b in range(2):
            for a in range(3):
                k[256 * b:256 * b + 256, a] = _run(-LATTICE + (5 + 3 * a) * _cell(129) + 3 + 7 * b, 5)
            k[256 * b:256 * b + 256, 3] = 300 if b == 0 else np.asarray([-600, 300, 1024])[np.arange(256) % 3]
        return BOX_INVERTED, [[129, 129, 129, 5]], k, True
    if name == "plane_window":
        # 256 consecutive points over 21 cells of each axis of a resolution-33 plane, scattered in the plane: the per-plane pass's 12 x 12 window holds
        # cells 0 .. 11 from the block's smallest tap; footprints straddle its last row and column
        k = np.zeros((512, 4), np.int64)
        i = np.arange(256)
        for b in range(2):
            for a, mul in enumerate((1, 37, 101)):
                k[256 * b:256 * b + 256, a] = -LATTICE + (3 + a) * _cell(33) + 60 + 5 * ((i * mul + 17 * b) % 256)
            k[256 * b:256 * b + 256, 3] = 200
        return BOX_INVERTED, [[33, 33, 33, 3], [9, 9, 9, 3]], k, True
    if name == "piled":
        # every point of the block in ONE cell of every plane, one time: every tap collides
        k = np.zeros((256, 4), np.int64)
        i = np.arange(256)
        for a, mul in enumerate((1, 7, 13)):
            k[:, a] = -LATTICE + 5 * _cell(17) + 1 + ((i * mul) % 127)
        k[:, 3] = 300
        return BOX_INVERTED, [[17, 17, 17, 5], [5, 5, 5, 3]], k, True
    if name.startswith("tile_"):
        n = int(name[5:])
        return BOX_INVERTED, [[9, 5, 17, 3], [5, 3, 9, 2]], rng.integers(-1100, 1101, (n, 4)), False
    raise KeyError(name)


LAYOUTS = ["nodes_inverted", "nodes_forward", "window_x", "window_y", "window_z", "time_uniform", "time_mixed", "zero_uniform", "zero_signed", "deferred_time",
           "plane_window", "piled"]


def make_case(layout, C, signed=False):
    """The float32 inputs of a lattice case: namespace(lo, hi, res, pts [N, 3], times [N, 1], planes[s][p] [1, C, H, W], gout [N, S C], k, identity)."""
    rng = np.random.default_rng(sum(map(ord, layout)) * 131 + C)
    (lo, hi), res, k, identity = _layout(layout, rng)
    lo64, hi64 = np.asarray(lo), np.asarray(hi)
    q = k / float(LATTICE)
    pts = (lo64 + (q[:, :3] + 1.0) * ((hi64 - lo64) / 2.0)).astype(np.float32)
    times = q[:, 3:4].astype(np.float32)
    if layout == "zero_signed":
        times[129, 0] = -0.0
    N, S = k.shape[0], len(res)
    planes = []
    for s in range(S):
        row = []
        for ax, ay in PAIRS:
            shape = (1, C, res[s][ay], res[s][ax])
            row.append((rng.standard_normal(shape) if signed else rng.random(shape) + 0.3).astype(np.float32))
        planes.append(row)
    gout = rng.standard_normal((N, S * C)).astype(np.float32)
    if N:
        gout[rng.random(N) < 0.05] = 0.0                                       # zero rows: the kernels skip their taps
    return types.SimpleNamespace(layout=layout, C=C, lo=lo, hi=hi, res=res, pts=pts, times=times, planes=planes, gout=gout, k=k, identity=identity, N=N, S=S)


def lattice_is_exact(case):
    """q and v recomputed in float32, q both plain and through a fused multiply-add, equal the float64 values bit for bit."""
    f32 = np.float32
    lo, hi = np.asarray(case.lo, f32), np.asarray(case.hi, f32)
    scale = f32(2.0) / (hi - lo)
    d = case.pts - lo                                                         # float32
    plain = d * scale - f32(1.0)
    fused = (d.astype(np.float64) * scale.astype(np.float64) - 1.0).astype(f32)      # one rounding: the product of two floats is exact in float64
    q64 = normalise(case.pts, case.times, case.lo, case.hi)
    want = case.k / float(LATTICE)
    ok = np.array_equal(plain.astype(np.float64), q64[:, :3]) and np.array_equal(fused.astype(np.float64), q64[:, :3]) and np.array_equal(q64, want)
    q32 = np.concatenate([plain, case.times.reshape(-1, 1)], axis=1)
    for r in case.res:
        for a in range(4):
            s32 = f32(0.5) * f32(r[a] - 1)
            v32 = (q32[:, a] + f32(1.0)) * s32
            ok = ok and v32.dtype == f32 and np.array_equal(v32.astype(np.float64), (q64[:, a] + 1.0) * (0.5 * (r[a] - 1)))
    return bool(ok)
