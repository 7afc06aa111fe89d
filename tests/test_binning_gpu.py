"""-m gpu: the binning stage between the projection and the render kernels (csrc/binning.hip), called directly (emd_raster_binning) on records placed
where its kernels have seams, against the numpy reference of tests/binning_checks.py (pinned by tests/test_binning_cpu.py, written from the contract).

Everything is integer and deterministic: every comparison is exact and covers every position.  For every call `_bin_and_check` asserts (a) the return
code, (b) the four status words, (c) tile id, depth bits, Gaussian id and quadrant mask at every one of the D positions, (d) every tile range, (e) the
tile_order contract, (f) the 4096-word guards behind geom_ws, bin_ws, status and tile_order, (g) that depth_key and binrec were not written.  Both
workspaces arrive filled with 0xDEADBEEF.  A failure names the first differing position, its window of 2048 slots, the owning Gaussian, its block of
256 and the offset within its run.  Sizes are the smallest at which each mechanism exists: 256 depth-ordered Gaussians per block, 2048 output slots
per window, 1024 block sums per chunk and 8192 per trip of the block-sum scan, 1 048 576 list positions per sweep of the range kernel, 8192 tiles kept
in registers and 1024 buckets of 16 entries in the dispatch order.

Where the record format cannot hold a case as the issue states it, the nearest case that it can hold is used:
  * a Gaussian's pairs are width x height with both below the grid's 128 x 64 (and below 1024 on any grid): runs of 257, 2049 and 3 * 2048 + 7 = 6151
    pairs (two primes and 3 x 683) do not exist; 258, 2050 and 6156 = 3 * 2048 + 12 stand in, and instead of relying on three orders alone, every run
    length is also placed with its first slot on a window's first and last slot and its last slot on a window's last and first slot (asserted);
  * a grid has fewer than 1024 tiles along each axis: T = 8193 = 3 x 2731 and T = 65 537 (a prime) do not exist; 8194 = 34 x 241 and 65 538 = 198 x 331
    stand in.  With 8194 tiles two tiles lie past 8192 (they hold long lists in two distinct buckets); the eight distinct buckets past tile 8192 are
    asserted at T = 65 536."""
import ctypes as C

import numpy as np
import pytest
import torch

from emd_amd import _lib as L
from tests import binning_checks as bc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xDEADBEEF             # pre-fill of every workspace and guard
GUARD = 4096
KEY0 = 0x3F000000             # bits of 0.5f: the nearest depth the builders use (near plane 0.2: the narrow range ends 2^27 above 0x3E4CCCCD)


def _filled(words):
    return torch.full((words + GUARD,), SENT - (1 << 32), dtype=torch.int32, device=DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)


def _host(t):
    return t.cpu().numpy().view(np.uint32)


class Workspaces:
    """geom_ws and bin_ws of one shape, sentinel-filled, each followed by a guard."""
    def __init__(self, N, H, W, capacity):
        self.geom_bytes, self.bin_bytes, _, _ = L.workspace_sizes(N, H, W, capacity)
        self.geom, self.bin = _filled(self.geom_bytes // 4), _filled(self.bin_bytes // 4)


def _bin_and_check(depth_key, binrec, *, H, W, capacity, near_plane=0.2, wide=False, ws=None, ref=None, label=""):
    """One emd_raster_binning call on the current stream, checked in full -> (reference, dict of what the device returned)."""
    depth_key = np.ascontiguousarray(depth_key, np.uint32)
    binrec = np.ascontiguousarray(binrec, np.uint32).reshape(-1, 2)
    N = len(depth_key)
    label = f"{label} [N={N} H={H} W={W} capacity={capacity} near={near_plane} wide={wide}]"
    if ref is None:
        ref = bc.binning_reference(depth_key, binrec, H=H, W=W, capacity=capacity, near_plane=near_plane, wide=wide)
    T = ref["T"]
    ws = ws or Workspaces(N, H, W, capacity)
    dk, br = _dev(depth_key) if N else None, _dev(binrec) if N else None
    status, order = _filled(4), _filled(T)
    lib = L.load()
    a = L.EmdBinningArgs()
    a.num_gaussians, a.image_height, a.image_width, a.flags = N, H, W, L.FLAG_WIDE_DEPTH_SORT if wide else 0
    a.near_plane, a.bin_capacity = near_plane, capacity
    a.depth_key, a.binrec = L.ptr(dk), L.ptr(br)
    a.geom_ws, a.geom_bytes, a.bin_ws, a.bin_bytes = ws.geom.data_ptr(), ws.geom_bytes, ws.bin.data_ptr(), ws.bin_bytes
    a.status, a.tile_order = status.data_ptr(), order.data_ptr()
    rc = lib.emd_raster_binning(C.byref(a), L.stream())
    assert rc == 0, f"{label}: (a) returned {rc}: {lib.emd_last_error()}"
    st = _host(status)                                       # (the copy synchronises with the stream)
    got = dict(status=tuple(int(x) for x in st[:4]))
    assert got["status"] == ref["status"], f"{label}: (b) status (num_rendered, overflow, num_visible, reserved) {got['status']}, expected {ref['status']}"
    # the list and the ranges, through the export of the parity tests
    D = 0 if ref["overflow"] else ref["D"]
    dims = L.EmdDims(N, H, W, capacity, 0, 0)
    keys = torch.zeros(max(D, 1), dtype=torch.int64, device=DEV)
    ids, masks = (torch.zeros(max(D, 1), dtype=torch.int32, device=DEV) for _ in range(2))
    ranges = torch.full((T, 2), -1, dtype=torch.int32, device=DEV)
    rc = lib.emd_raster_export_binning(C.byref(dims), ws.geom.data_ptr(), ws.geom_bytes, ws.bin.data_ptr(), ws.bin_bytes, D, keys.data_ptr(), ids.data_ptr(),
                                       ranges.data_ptr(), masks.data_ptr(), L.stream())
    assert rc == 0, f"{label}: export returned {rc}: {lib.emd_last_error()}"
    got["ranges"], got["order"] = _host(ranges).reshape(T, 2), _host(order)[:T]
    if not ref["overflow"]:
        k = keys.cpu().numpy().view(np.uint64)[:D]
        got["tiles"], got["depth"], got["ids"], got["masks"] = (k >> np.uint64(32)).astype(np.uint32), k.astype(np.uint32), _host(ids)[:D], _host(masks)[:D]
        bc.assert_list(f"{label}: (c) tile ids", got["tiles"], ref["tiles"], ref)
        bc.assert_list(f"{label}: (c) Gaussian ids", got["ids"], ref["ids"], ref)
        bc.assert_list(f"{label}: (c) quadrant masks", got["masks"], ref["masks"], ref)
        bc.assert_list(f"{label}: (c) depth bits of the keys", got["depth"], ref["keys"].astype(np.uint32), ref)
    bc.assert_ranges(f"{label}: (d) ranges", got["ranges"], ref["ranges"])
    bc.assert_tile_order(f"{label}: (e) tile_order", got["order"], ref)
    for name, t in (("geom_ws", ws.geom), ("bin_ws", ws.bin), ("status", status), ("tile_order", order)):
        tail = _host(t[-GUARD:])
        assert (tail == SENT).all(), f"{label}: (f) guard behind {name}: word {int(np.flatnonzero(tail != SENT)[0])} of {GUARD} holds 0x{int(tail[tail != SENT][0]):X}"
    if N:
        assert np.array_equal(_host(dk), depth_key), f"{label}: (g) depth_key was written to"
        assert np.array_equal(_host(br).reshape(-1, 2), binrec), f"{label}: (g) binrec was written to"
    return ref, got


# ---- builders ---------------------------------------------------------------------------------------------------------------------------------
def _scene(rects, rng, cull_every=0, shuffle=True, step=5):
    """rects: (x0, y0, w, h, skip) arrays of the VISIBLE Gaussians in depth order (nearest first).  -> (depth_key [N], binrec [N][2]): the ids are a
    random permutation of the depth ranks, distinct keys `step` apart from 0.5f up, and with cull_every = c every c-th id is a culled one whose
    record (a 1023 x 1023 rectangle) must never be read."""
    rec = bc.make_binrec(*rects)
    V = len(rec)
    N = V + (V // (cull_every - 1) + 3 if cull_every else 0)
    culled = np.zeros(N, bool)
    if cull_every:
        culled[::cull_every] = True
        culled[np.flatnonzero(~culled)[V:]] = True           # (whatever is left over behind the V visible ids)
    vis_ids = np.flatnonzero(~culled)
    assert len(vis_ids) == V and KEY0 + V * step < 0x3E4CCCCD + (1 << 27)
    id_of_rank = rng.permutation(vis_ids) if shuffle else vis_ids
    depth_key = np.full(N, bc.CULLED, np.uint32)
    depth_key[id_of_rank] = KEY0 + step * np.arange(V, dtype=np.uint32)
    binrec = np.empty((N, 2), np.uint32)
    binrec[:] = bc.make_binrec(0, 0, 1023, 1023, 15)[0]
    binrec[id_of_rank] = rec
    return depth_key, binrec


def _rect_for(count, gx, gy, k=0):
    """(w, h) with w * h == count inside a gx x gy grid (the widest such rectangle); the two zero forms alternate with k."""
    if count == 0:
        return ((0, 3), (5, 0), (0, 0))[k % 3]
    for w in range(min(gx, count), 0, -1):
        if count % w == 0 and count // w <= gy:
            return w, count // w
    raise ValueError(f"no rectangle of {count} tiles inside {gx} x {gy}")


def _rects_from_counts(counts, gx, gy, rng, skip=None):
    wh = np.array([_rect_for(int(c), gx, gy, k) for k, c in enumerate(counts)], dtype=np.int64).reshape(-1, 2)
    w, h = wh[:, 0], wh[:, 1]
    x0 = rng.integers(0, gx - w + 1)
    y0 = rng.integers(0, gy - h + 1)
    return x0, y0, w, h, (rng.integers(0, 16, len(w)) if skip is None else skip)


def _small_rects(counts, gx, gy, rng):
    """Rectangles for counts in {0, 1, 2} (2 = two tiles side by side), fast for millions."""
    counts = np.asarray(counts, np.int64)
    w, h = counts.copy(), (counts > 0).astype(np.int64)
    zero = np.flatnonzero(counts == 0)
    w[zero[1::2]], h[zero[1::2]] = 3, 0                       # both zero forms: width 0 and height 0
    x0 = rng.integers(0, gx - np.maximum(w, 1) + 1)
    y0 = rng.integers(0, gy, len(w))
    return x0, y0, w, h, rng.integers(0, 16, len(w))


# ---- run lengths at the window seams ------------------------------------------------------------------------------------------------------------
RUNS = (0, 1, 2, 255, 256, 258, 2047, 2048, 2050, 4096, 3 * 2048 + 12)
ALIGNMENTS = {"first slot on a window's first": (0, 0), "first slot on a window's last": (0, 2047), "last slot on a window's last": (1, 0),
              "last slot on a window's first": (1, 1)}          # (0 = the run's start, 1 = its end) % 2048 == value


@pytest.mark.parametrize("order", ("ascending", "descending", "rotated"))
def test_run_lengths_at_the_window_seams(order):
    """Grid 128 x 64.  The run lengths once in the given order, then every length four more times behind pads (runs themselves) that put its first /
    last slot on a window's first / last slot."""
    gx, gy = 128, 64
    base = list(RUNS)
    base = base[::-1] if order == "descending" else base[4:] + base[:4] if order == "rotated" else base
    counts, pos = list(base), sum(base)
    for run in base:
        for which, value in ALIGNMENTS.values():
            if run == 0:
                continue
            pad = (value - (pos + which * run)) % 2048
            counts += [c for c in (pad // 128 * 128, pad % 128) if c] + [run]
            pos += pad + run
    rng = np.random.default_rng(900 + len(order))
    dk, br = _scene(_rects_from_counts(counts, gx, gy, rng), rng, cull_every=5)
    D = sum(counts)
    ref, _ = _bin_and_check(dk, br, H=16 * gy, W=16 * gx, capacity=D, label=f"seams {order}")
    assert ref["T"] == 8192 and ref["D"] == D and ref["counts"].tolist() == counts
    starts, ends = ref["starts"], ref["starts"] + ref["counts"]
    for run in RUNS[1:]:
        mine = ref["counts"] == run
        for name, (which, value) in ALIGNMENTS.items():
            assert ((ends if which else starts)[mine] % 2048 == value).any(), f"no run of {run} pairs has its {name} slot"
    assert (starts[ref["counts"] > 0] % 2048 == 0).any() and (ends[ref["counts"] > 0] % 2048 == 0).any()


def test_one_rectangle_of_the_whole_1023_x_1023_grid():
    """1 046 529 pairs from one Gaussian: 511 windows walk the same block of Gaussians, three tile passes, the identity order above 65 536 tiles."""
    rng = np.random.default_rng(910)
    # (a zero-pair Gaussian in front of it and one behind it)
    dk, br = _scene((np.zeros(3, int), np.zeros(3, int), np.array([0, 1023, 5]), np.array([7, 1023, 0]), np.array([15, 15, 15])), rng, cull_every=2)
    ref, _ = _bin_and_check(dk, br, H=16 * 1023, W=16 * 1023, capacity=1023 * 1023, label="1023 x 1023")
    assert ref["D"] == 1046529 == ref["T"] and ref["V"] == 3 and ref["identity_order"] and (ref["D"] + 2047) // 2048 == 512


# ---- zero-pair visible Gaussians ----------------------------------------------------------------------------------------------------------------
def _zero_layouts():
    rng = np.random.default_rng(920)
    some = lambda n: rng.integers(1, 21, n).tolist()
    yield "whole blocks of zeros in front of, between and behind the runs", [0] * 512 + some(300) + [0] * 768 + some(300) + [0] * 512
    yield "zeros behind exactly one block of runs", some(256) + [0] * 256 + some(256) + [0] * 256
    yield "alternating by lane with one pair", [0, 1] * 1500
    yield "alternating by lane, the zeros on the odd lanes", [1, 0] * 1500 + [1]
    yield "only the last visible Gaussian emits pairs", [0] * 1000 + [5000]
    yield "only the last visible Gaussian emits pairs, it opens a block", [0] * 1024 + [3]
    yield "no visible Gaussian emits pairs", [0] * 700
    # the window that starts at slot 2048: its first slot belongs to a Gaussian that 300 zero-count ones follow, at lane 0 / 100 / 255 of its block,
    # with its run starting in front of the window and exactly on it
    for lane in (0, 100, 255):
        for lead in (2040, 2048):
            front = [0] * (256 + lane - 16)                  # (16 Gaussians emit the `lead` pairs in front of the owner)
            yield (f"first slot of a window owned by lane {lane}, {2048 - lead} slots into its run, 300 zeros behind it",
                   front + [128] * (lead // 128) + [lead % 128] * (lead % 128 > 0) + [20] + [0] * 300 + some(40) + [0] * 300 + [2048 + 77] + [0] * 5)


@pytest.mark.parametrize("name, counts", list(_zero_layouts()), ids=lambda v: v.replace(" ", "_")[:60] if isinstance(v, str) else None)
def test_zero_pair_visible_gaussians(name, counts):
    gx, gy = 128, 64
    rng = np.random.default_rng(921 + len(counts))
    dk, br = _scene(_rects_from_counts(counts, gx, gy, rng), rng, cull_every=3)
    ref, _ = _bin_and_check(dk, br, H=16 * gy, W=16 * gx, capacity=sum(counts) + 100, label=name)
    assert ref["V"] == len(counts) and ref["D"] == sum(counts)
    if "first slot of a window" in name:
        owner = int(ref["own"][2048])
        assert ref["counts"][owner] == 20 and owner % 256 == int(name.split("lane ")[1].split(",")[0]) and not ref["counts"][owner + 1:owner + 301].any()
        assert 2048 - int(ref["starts"][owner]) == int(name.split(", ")[1].split(" ")[0])


# ---- visible-count thresholds ---------------------------------------------------------------------------------------------------------------------
def _threshold_scene(V, rng, gx=64, gy=64, boundary_at=None):
    """V visible Gaussians of 0 / 1 / 2 pairs; the run of the first Gaussian of the last block of 256 starts exactly on a window (so that a window's
    first slot belongs to that block); boundary_at: the pairs of the tile rows above the grid's middle add up to exactly this many."""
    counts = rng.integers(0, 3, V)
    last_block = (V - 1) // 256 * 256
    lo = 0
    if boundary_at is not None:
        cum = np.cumsum(counts)
        lo = int(np.searchsorted(cum, boundary_at))
        if cum[lo] != boundary_at:                           # (the prefix sums step over it: 2^20 - 1, 2^20 + 1)
            counts[lo] = 1
        lo += 1
        assert counts[:lo].sum() == boundary_at and lo < last_block
    if last_block >= 8192:                                  # (below that the pairs in front of the last block do not fill a window)
        counts[last_block] = 1 + counts[last_block] % 2
        short = int(-counts[:last_block].sum() % 2048)
        zeros = lo + np.flatnonzero(counts[lo:last_block] == 0)[:short]
        assert len(zeros) == short
        counts[zeros] = 1
    x0, y0, w, h, skip = _small_rects(counts, gx, gy, rng)
    if boundary_at is not None:                              # the first `lo` Gaussians in the upper half of the grid, the others below
        y0 = np.where(np.arange(V) < lo, y0 % (gy // 2), gy // 2 + y0 % (gy // 2))
    return counts, (x0, y0, w, h, skip)


@pytest.mark.parametrize("V", [1, 255, 256, 257, 262143, 262145])
def test_visible_count_thresholds(V):
    """One block, 1024 block sums (one chunk of the scan) and one more; culled keys interleaved, so N > V."""
    rng = np.random.default_rng(930 + V)
    counts, rects = _threshold_scene(V, rng)
    dk, br = _scene(rects, rng, cull_every=7)
    ref, _ = _bin_and_check(dk, br, H=1024, W=1024, capacity=int(counts.sum()), label=f"V={V}")
    assert ref["V"] == V < ref["N"] and ref["D"] == counts.sum()
    if V > 8192:
        firsts = ref["own"][::2048] // 256                  # the block of 256 that owns every window's first slot
        assert firsts.max() == (V - 1) // 256, "no window's first slot belongs to the last block"
        assert V < 262145 or firsts.max() >= 1024


def test_second_trip_of_the_block_sum_scan():
    """V = 2 097 152 + 257: 8194 block sums, the scan's second trip of 8192; a window's first slot belongs to block 8192; a tile boundary at list
    position 1 048 576, where the range kernel's second sweep begins."""
    V = 2097152 + 257
    rng = np.random.default_rng(940)
    counts, rects = _threshold_scene(V, rng, boundary_at=1 << 20)
    dk, br = _scene(rects, rng, cull_every=9, step=7)
    ref, _ = _bin_and_check(dk, br, H=1024, W=1024, capacity=int(counts.sum()), label=f"V={V}")
    assert ref["V"] == V < ref["N"] and ref["D"] == counts.sum() > 2 * (1 << 20)          # (more than one sweep of the range kernel)
    assert (ref["own"][::2048] // 256).max() >= 8192, "no window's first slot belongs to a block of the scan's second trip"
    assert ref["tiles"][(1 << 20) - 1] < 2048 <= ref["tiles"][1 << 20], "no tile boundary at list position 1 048 576"


# ---- capacity and overflow --------------------------------------------------------------------------------------------------------------------------
def test_capacity_and_overflow():
    gx, gy = 128, 64
    rng = np.random.default_rng(950)
    counts = rng.integers(0, 13, 900).tolist()
    pad = -(sum(counts) + 5) % 2048                          # D = a multiple of 2048, the deepest Gaussian holds 5 pairs of it
    counts += [c for c in (pad // 128 * 128, pad % 128) if c] + [5]
    V = len(counts)
    dk, br = _scene(_rects_from_counts(counts, gx, gy, rng), rng, cull_every=4)
    D = sum(counts)
    assert D % 2048 == 0 and D >= 4096
    for capacity, bit in ((D, 0), (D + 1, 0), (D - 1, 1), (D + 2048, 0), (D - 2048, 1), (D + 1000, 0), (1, 1), (0, 1)):
        ref, got = _bin_and_check(dk, br, H=16 * gy, W=16 * gx, capacity=capacity, label=f"D={D}")
        assert ref["overflow"] == bit and ref["status"] == (D, bit, V, V)
    # one Gaussian fewer: D is no multiple of 2048 any more
    vis = np.flatnonzero(dk != bc.CULLED)
    dk2 = dk.copy()
    dk2[vis[np.argmax(dk[vis])]] = bc.CULLED
    D2 = D - 5
    for capacity, bit in ((D2, 0), (D2 + 1, 0), (D2 - 1, 1), (0, 1)):
        ref, _ = _bin_and_check(dk2, br, H=16 * gy, W=16 * gx, capacity=capacity, label=f"D={D2}")
        assert ref["status"] == (D2, bit, V - 1, V - 1) and D2 % 2048
    # bit 1 alone: one narrow key 2^27 past the near plane's bits (the same key sorts fine when wide); bits 0 and 1 together
    far = dk.copy()
    far[vis[17]] = bc.near_bits(0.2) + (1 << 27)
    for capacity, wide, word in ((D, False, 2), (D + 5, False, 2), (D - 1, False, 3), (0, False, 3), (D, True, 0), (D - 1, True, 1)):
        ref, _ = _bin_and_check(far, br, H=16 * gy, W=16 * gx, capacity=capacity, wide=wide, label="one key beyond the narrow range")
        assert ref["status"] == (D, word, V, V)
    far[vis[17]] -= 1
    assert _bin_and_check(far, br, H=16 * gy, W=16 * gx, capacity=D, label="the last key of the narrow range")[0]["overflow"] == 0
    # a zero-pair scene: capacity 0 holds it
    ref, _ = _bin_and_check(dk, bc.make_binrec(1, 2, 0, 3, n=len(dk)), H=16 * gy, W=16 * gx, capacity=0, label="capacity 0, D 0")
    assert ref["status"] == (0, 0, V, V)


# ---- tile counts and ranges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gx, gy", [(1, 1), (3, 1), (257, 1), (1, 257), (257, 257)], ids=lambda v: str(v))
def test_tile_counts_and_ranges(gx, gy):
    """T = 1, 3, 257 (as a row and as a column) and 66 049: zero, one, two and three tile passes.  All pairs in tile 0, all in tile T - 1, every other
    tile empty, and rectangles all over the grid."""
    T = gx * gy
    rng = np.random.default_rng(960 + T + gx)
    n = 3000
    one = np.ones(n, np.int64)
    skip = rng.integers(0, 16, n)
    layouts = {"all pairs in tile 0": (0 * one, 0 * one, one, one, skip), f"all pairs in tile {T - 1}": ((gx - 1) * one, (gy - 1) * one, one, one, skip)}
    t = rng.integers(0, (T + 1) // 2, n) * 2
    layouts["every other tile empty"] = (t % gx, t // gx, one, one, skip)
    w, h = rng.integers(0, min(gx, 6) + 1, n), rng.integers(0, min(gy, 6) + 1, n)
    layouts["rectangles all over the grid"] = (rng.integers(0, gx - w + 1), rng.integers(0, gy - h + 1), w, h, skip)
    for name, rects in layouts.items():
        dk, br = _scene(rects, rng, cull_every=6)
        ref, _ = _bin_and_check(dk, br, H=16 * gy, W=16 * gx, capacity=int((rects[2] * rects[3]).sum()) + 3, label=f"T={T}: {name}")
        assert ref["T"] == T and ref["identity_order"] == (T > 65536)
        if name.startswith("all pairs"):
            only = 0 if name.endswith(" 0") else T - 1
            assert ref["ranges"][only].tolist() == [0, n] and ref["ranges"].sum() == n
        if name.startswith("every other"):
            assert not ref["ranges"][1::2].any() and ref["ranges"][::2].any()


# ---- dispatch order -------------------------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 15, 16, 17, 32, 48, 64, 80, 1600, 3200, 16367, 16368, 16369, 20000)        # the last four sit at the bucket cap: 1022, 1023, 1023, 1023


@pytest.mark.parametrize("gx, gy", [(32, 32), (41, 25), (128, 64), (34, 241), (256, 256), (198, 331)], ids=lambda v: str(v))
def test_dispatch_order(gx, gy):
    """T = 1024, 1025, 8192, 8194, 65 536 (one workgroup, the first 8192 tiles kept in registers, the others re-read) and 65 538 (the identity).  Lists
    of the lengths above twice: from tile 0 up, and -- reversed -- down from tile T - 1, which lies past tile 8192 where there is one; every other tile
    holds 0 .. 3 entries."""
    T = gx * gy
    rng = np.random.default_rng(970 + T)
    length = rng.integers(0, 4, T)
    spot = np.arange(len(LENGTHS)) * 3
    length[spot] = LENGTHS
    past = T - 1 - np.arange(len(LENGTHS)) * (1 if T < 8192 + 3 * len(LENGTHS) else 3)
    length[past] = LENGTHS[::-1][:len(past)] if T != 8194 else (3200, 16367) + LENGTHS[2:]
    tile = rng.permutation(np.repeat(np.arange(T), length))
    n = len(tile)
    one = np.ones(n, np.int64)
    dk, br = _scene((tile % gx, tile // gx, one, one, rng.integers(0, 16, n)), rng, cull_every=8)
    ref, _ = _bin_and_check(dk, br, H=16 * gy, W=16 * gx, capacity=n, label=f"T={T}")
    assert ref["T"] == T and ((ref["ranges"][:, 1] - ref["ranges"][:, 0]) == length).all()
    assert ref["identity_order"] == (T > 65536)
    assert set(ref["bucket"][spot]) == {0, 1, 2, 3, 4, 5, 100, 200, 1022, 1023}
    if T == 8194:
        assert ref["bucket"][8192:].tolist() == [1022, 200]
    if T == 65536:
        assert len(set(ref["bucket"][8192:]) - {0}) >= 8, "fewer than 8 distinct buckets of long lists past tile 8192"


# ---- masks ----------------------------------------------------------------------------------------------------------------------------------------------
def test_every_skip_combination_on_small_rectangles():
    """All 16 skip-bit combinations x (w, h) in {1, 2, 3}^2, every mask compared exactly; every mask value a pair can carry occurs."""
    rng = np.random.default_rng(980)
    skip, w, h = (v.ravel() for v in np.meshgrid(np.arange(16), np.arange(1, 4), np.arange(1, 4), indexing="ij"))
    rects = (rng.integers(0, 8 - w + 1), rng.integers(0, 8 - h + 1), w, h, skip)
    dk, br = _scene(rects, rng, cull_every=3)
    ref, got = _bin_and_check(dk, br, H=128, W=128, capacity=int((w * h).sum()), label="masks")
    assert len(w) == 144 and ref["D"] == 16 * 36
    assert set(ref["masks"].tolist()) == {0, 1, 2, 3, 4, 5, 8, 10, 12, 15}          # (columns kept) x (rows kept): the other six are no products
    by_id = {int(i): (int(s), int(a), int(b)) for i, s, a, b in zip(ref["perm"], skip, w, h)}
    lone = [m for i, m in zip(got["ids"], got["masks"]) if by_id[int(i)] == (15, 1, 1)]
    assert lone == [0], "w == h == 1 with all four skip bits carries no quadrant"


# ---- depth ----------------------------------------------------------------------------------------------------------------------------------------------
def test_depth_ties_narrow_and_wide_agree():
    """6000 ids on four depths (thousands of ties: the order inside a depth is the id order), a fifth of them culled; the narrow and the wide sort of
    the same in-range keys give the same list."""
    n, gx, gy = 6000, 16, 16
    rng = np.random.default_rng(990)
    dk = np.array([0.25, 0.5, 3.0, 700.0], np.float32).view(np.uint32)[rng.integers(0, 4, n)]
    dk[rng.random(n) < 0.2] = bc.CULLED
    w, h = rng.integers(0, 4, n), rng.integers(0, 4, n)
    br = bc.make_binrec(rng.integers(0, gx - w + 1), rng.integers(0, gy - h + 1), w, h, rng.integers(0, 16, n), upper=rng.integers(0, 1 << 20, n))
    D = int((w * h)[dk != bc.CULLED].sum())
    ref_n, narrow = _bin_and_check(dk, br, H=16 * gy, W=16 * gx, capacity=D, label="ties, narrow")
    ref_w, wide = _bin_and_check(dk, br, H=16 * gy, W=16 * gx, capacity=D, wide=True, label="ties, wide")
    assert ref_n["D"] == D and ref_n["overflow"] == ref_w["overflow"] == 0
    for name in ("tiles", "depth", "ids", "masks", "ranges", "status"):
        assert np.array_equal(narrow[name], wide[name]), name
    same = ref_n["keys"][1:] == ref_n["keys"][:-1]
    assert same.sum() > 2000 and (ref_n["ids"][1:][same] > ref_n["ids"][:-1][same]).all()


def test_nothing_visible_and_no_gaussians():
    rec = bc.make_binrec(0, 0, 3, 3, n=1000)
    for wide in (False, True):
        ref, _ = _bin_and_check(np.full(1000, bc.CULLED, np.uint32), rec, H=100, W=200, capacity=500, wide=wide, label="all culled")
        assert ref["status"] == (0, 0, 0, 0) and not ref["identity_order"]
        ref, _ = _bin_and_check(np.full(1000, bc.CULLED, np.uint32), rec, H=100, W=200, capacity=0, wide=wide, label="all culled, capacity 0")
        assert ref["status"] == (0, 0, 0, 0) and ref["identity_order"]
        for capacity in (0, 500):
            ref, _ = _bin_and_check(np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32), H=100, W=200, capacity=capacity, wide=wide, label="N = 0")
            assert ref["status"] == (0, 0, 0, 0) and ref["identity_order"] and ref["T"] == 7 * 13


# ---- dirty workspaces -----------------------------------------------------------------------------------------------------------------------------------
def test_small_call_on_the_workspaces_of_a_larger_one():
    """D = 300 k on 8192 tiles, then D = 3 k on the same tiles in the same, uncleared workspaces (its own, smaller carve of them), then the small call
    on fresh sentinel-filled ones: the same, correct results both times."""
    gx, gy = 128, 64
    rng = np.random.default_rng(1000)
    big = rng.integers(0, 25, 25000)
    small = rng.integers(0, 7, 1000)
    big_dk, big_br = _scene(_rects_from_counts(big, gx, gy, rng), rng, cull_every=5)
    small_dk, small_br = _scene(_rects_from_counts(small, gx, gy, rng), rng, cull_every=3)
    ws = Workspaces(len(big_dk), 16 * gy, 16 * gx, int(big.sum()))
    ref, _ = _bin_and_check(big_dk, big_br, H=16 * gy, W=16 * gx, capacity=int(big.sum()), ws=ws, label="the large call")
    assert 280_000 < ref["D"] < 320_000
    ref, dirty = _bin_and_check(small_dk, small_br, H=16 * gy, W=16 * gx, capacity=int(small.sum()), ws=ws, label="the small call on the large call's workspaces")
    assert 2_500 < ref["D"] < 3_500
    _, fresh = _bin_and_check(small_dk, small_br, H=16 * gy, W=16 * gx, capacity=int(small.sum()), ref=ref, label="the small call on fresh workspaces")
    for name in ("status", "tiles", "depth", "ids", "masks", "ranges"):
        assert np.array_equal(dirty[name], fresh[name]), name
    # and an overflowing small call on them reports and leaves every range (0, 0)
    _bin_and_check(small_dk, small_br, H=16 * gy, W=16 * gx, capacity=int(small.sum()) - 1, ws=ws, label="the small call, one slot short, on the large call's workspaces")


# ---- bad arguments ----------------------------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_leave_every_buffer_untouched():
    N, H, W, capacity = 1000, 64, 96, 5000
    rng = np.random.default_rng(1010)
    ws = Workspaces(N, H, W, capacity)
    dk, br = _scene(_rects_from_counts(rng.integers(0, 5, N), 6, 4, rng), rng)
    bufs = dict(depth_key=_dev(dk), binrec=_dev(br), geom_ws=ws.geom, bin_ws=ws.bin, status=_filled(4), tile_order=_filled(24))
    before = {k: _host(v).copy() for k, v in bufs.items()}
    lib = L.load()
    for kw, code, text in bc.BAD_ARGUMENTS:
        a = L.EmdBinningArgs()
        a.num_gaussians, a.image_height, a.image_width, a.flags, a.near_plane, a.bin_capacity = N, H, W, 0, 0.2, capacity
        for k, v in bufs.items():
            setattr(a, k, v.data_ptr())
        a.geom_bytes, a.bin_bytes = ws.geom_bytes, ws.bin_bytes
        for k, v in kw.items():
            setattr(a, k, v(ws.geom_bytes, ws.bin_bytes) if callable(v) else v)
        assert lib.emd_raster_binning(C.byref(a), L.stream()) == code, kw
        assert text in lib.emd_last_error(), (kw, lib.emd_last_error())
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert np.array_equal(_host(v), before[k]), f"{k} was written to by a rejected call"
    # ... and the same buffers serve a valid call
    _bin_and_check(dk, br, H=H, W=W, capacity=capacity, ws=ws, label="after the rejected calls")
