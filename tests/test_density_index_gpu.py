"""-m gpu: the first three links of a density-control event (csrc/densify.hip) called by name -- emd_densify_decide / emd_refine_decide,
emd_densify_scan, emd_densify_index / emd_refine_index, emd_densify_split_rank -- and emd_after_train_stats, against tests/density_ref.py (a numpy
float64 restatement of the contract in include/emd_raster.h, itself checked against the reference programs' order of operations by
tests/test_density_ref_cpu.py).  The last link, the gather, has tests/test_densify_gather_gpu.py.

Every buffer handed to a kernel, input or output, is followed by a guard of 4 096 words holding a sentinel, and outputs are prefilled with the same
sentinel: each test checks that every element that must be written was written and that nothing beside it was (inputs and guards unchanged).
Every comparison is bit-exact except grad_norm of emd_after_train_stats (rtol 1e-6 against float64 hypot, the bound tests/test_vanilla_refine_gpu.py
applies to it)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import density_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 4096
SENTINEL = -1515870811          # 0xA5A5A5A5: the same byte everywhere, no legal count, offset, row index or kind


class Buffers:
    """Device buffers of one call, each with its guard; `check()` proves that only the expected bytes changed."""

    def __init__(self):
        self.items = []

    def put(self, array):
        """An input: the array's bytes, then the guard."""
        raw = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).ravel().copy()).to(DEV)
        t = torch.full(((raw.numel() + 3) // 4 + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        t.view(torch.uint8)[:raw.numel()] = raw
        self.items.append((t, raw.numel(), raw))
        return t

    def out(self, n):
        """An int32 output of n words, prefilled with the sentinel (its content is the caller's to check)."""
        t = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.items.append((t, 4 * n, None))
        return t

    def check(self):
        torch.cuda.synchronize()
        for t, nbytes, content in self.items:
            raw = t.view(torch.uint8)
            assert bool((raw[nbytes:] == 0xA5).all()), "a kernel wrote behind a buffer"
            assert content is None or torch.equal(raw[:nbytes], content), "a kernel changed an input"


def _read(t, n, dtype=np.int32):
    return t[:n].cpu().numpy().view(dtype) if n else np.zeros(0, dtype)


def _expect(t, want, msg):
    """The first want.size words of `t` are `want`, bit for bit (compared on the device; numpy writes the report when they differ)."""
    want = np.ascontiguousarray(want, np.int32)
    if not torch.equal(t[:want.size], torch.from_numpy(want.ravel()).to(DEV)):
        np.testing.assert_array_equal(_read(t, want.size).reshape(want.shape), want, err_msg=msg)
        raise AssertionError(msg)


def _lib():
    from emd_amd import _lib as L
    return L, L.load()


# ---- scan alone ----------------------------------------------------------------------------------------------------------------------------------
def _scan_contents(rng, cols, blocks):
    yield "random", rng.integers(0, 257, (cols, blocks))
    yield "all 256", np.full((cols, blocks), 256)
    yield "all 0", np.zeros((cols, blocks), np.int64)
    for at in sorted({0, 63, 64, 1023, 1024, blocks - 1}):
        if at < blocks:
            one = np.zeros((cols, blocks), np.int64)
            one[:, at] = 1
            yield f"a single 1 at {at}", one


@pytest.mark.parametrize("blocks", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3001])
def test_scan_alone(blocks):
    """k_densify_scan walks a column in trips of 1 024 blocks with a carry: one trip up to 1 024 blocks, two up to 2 048, three beyond."""
    L, lib = _lib()
    rng = np.random.default_rng(blocks)
    for cols in (1, 3, 4, 8):
        for name, counts in _scan_contents(rng, cols, blocks):
            want, want_totals = R.exclusive_offsets(counts)
            for num_points in (256 * blocks, 256 * blocks - 255):
                b = Buffers()
                col, tot = b.out(cols * blocks), b.out(cols)
                col[:cols * blocks] = torch.from_numpy(counts.astype(np.int32).ravel()).to(DEV)
                assert lib.emd_densify_scan(num_points, cols, col.data_ptr(), tot.data_ptr(), L.stream()) == L.EMD_OK
                b.check()
                _expect(col, want, f"{name}, {cols} columns, N {num_points}")
                _expect(tot, want_totals, f"totals: {name}, {cols} columns, N {num_points}")


def test_scan_of_no_points_zeroes_the_totals_and_bad_arguments_are_refused():
    L, lib = _lib()
    for cols in (1, 3, 8):
        b = Buffers()
        col, tot = b.out(8), b.out(8)
        assert lib.emd_densify_scan(0, cols, col.data_ptr(), tot.data_ptr(), L.stream()) == L.EMD_OK
        b.check()
        assert _read(tot, 8).tolist() == [0] * cols + [SENTINEL] * (8 - cols) and (_read(col, 8) == SENTINEL).all()
    for num_points, cols, with_totals in ((300, 0, True), (300, 9, True), (300, 3, False), (0, 3, False), (-1, 3, True)):
        b = Buffers()
        col, tot = b.out(32), b.out(16)
        assert lib.emd_densify_scan(num_points, cols, col.data_ptr(), tot.data_ptr() if with_totals else None, L.stream()) == L.EMD_ERR_INVALID
        b.check()
        assert (_read(col, 32) == SENTINEL).all() and (_read(tot, 16) == SENTINEL).all()


# ---- index alone ---------------------------------------------------------------------------------------------------------------------------------
INDEX_N = [1, 63, 64, 65, 255, 256, 257, 1000, 262145]
DENSIFY_LEGAL = [1, 3, 4]                                                                                       # keep, keep | clone, split
REFINE_LEGAL = [k | d | s for k in (0, 1) for d in (0, 2) for s in (0, 8, 12)][1:]                              # samples only of a split source


def _patterns(n, rng):
    """name -> the rows that carry flags."""
    i = np.arange(n)
    lane, last = i % 256, i >= 256 * ((n - 1) // 256)
    pats = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": i % 2 == 1, "random": rng.random(n) < 0.5, "last block": last,
            "wave 2": (lane >= 128) & (lane < 192)}
    for l in (0, 63, 64, 255):
        pats[f"lane {l}"] = lane == l
    return pats


def _codes(n, legal, full, rng):
    """(name, code[n]): every pattern with the legal codes dealt in turn, all rows with one code (`full`), and a random deal of
    every legal code and 0 (the columns' flags then differ from each other at every row)."""
    i = np.arange(n)
    legal = np.array(legal)
    for name, rows in _patterns(n, rng).items():
        yield name, np.where(rows, legal[i % len(legal)], 0).astype(np.int32)
    for code in full:
        yield f"all {code}", np.full(n, code, np.int32)
    yield "random deal", np.r_[0, legal][rng.integers(0, len(legal) + 1, n)].astype(np.int32)


@pytest.mark.parametrize("n", INDEX_N)
def test_densify_index_alone(n):
    """Hand-written codes; offsets and totals from numpy: neither decide nor scan takes part."""
    L, lib = _lib()
    rng = np.random.default_rng(n)
    for name, code in _codes(n, DENSIFY_LEGAL, (3, 4), rng):
        offsets, totals = R.exclusive_offsets(R.block_counts(code, 3))
        src, kind = R.index_densify(code)
        m = len(src)
        assert m == totals[0] + totals[1] + 2 * totals[2]
        b = Buffers()
        d_code, d_off, d_tot, d_src, d_kind = b.put(code), b.put(offsets), b.put(totals), b.out(m), b.out(m)
        assert lib.emd_densify_index(n, m, d_code.data_ptr(), d_off.data_ptr(), d_tot.data_ptr(), d_src.data_ptr(), d_kind.data_ptr(), L.stream()) == L.EMD_OK
        b.check()
        _expect(d_src, src, name)
        _expect(d_kind, kind, name)


@pytest.mark.parametrize("n", INDEX_N)
def test_refine_index_alone(n):
    L, lib = _lib()
    rng = np.random.default_rng(n + 7)
    for name, code in _codes(n, REFINE_LEGAL, (15, 12, 3), rng):
        offsets, totals = R.exclusive_offsets(R.block_counts(code, 4))
        b0 = Buffers()
        d_code, d_off, d_tot = b0.put(code), b0.put(offsets), b0.put(totals)
        for ns in (1, 2, 3, 13):
            src, kind, rank = R.index_refine(code, ns)
            m = len(src)
            assert m == totals[0] + ns * totals[2] + totals[1]
            for with_rank in (False, True):
                b = Buffers()
                d_src, d_kind, d_rank = b.out(m), b.out(m), b.out(m)
                rc = lib.emd_refine_index(n, m, ns, d_code.data_ptr(), d_off.data_ptr(), d_tot.data_ptr(), d_src.data_ptr(), d_kind.data_ptr(),
                                          d_rank.data_ptr() if with_rank else None, L.stream())
                assert rc == L.EMD_OK
                b.check()
                tag = f"{name}, {ns} samples"
                _expect(d_src, src, tag)
                _expect(d_kind, kind, tag)
                _expect(d_rank, rank if with_rank else np.full(m, SENTINEL, np.int32), tag)
        b0.check()


def test_refine_index_refuses_0_and_14_samples():
    L, lib = _lib()
    code = np.full(300, 13, np.int32)
    offsets, totals = R.exclusive_offsets(R.block_counts(code, 4))
    for ns in (0, 14):
        b = Buffers()
        d_code, d_off, d_tot = b.put(code), b.put(offsets), b.put(totals)
        m = 300 * 15
        d_src, d_kind, d_rank = b.out(m), b.out(m), b.out(m)
        rc = lib.emd_refine_index(300, 300 + 300 * ns, ns, d_code.data_ptr(), d_off.data_ptr(), d_tot.data_ptr(), d_src.data_ptr(), d_kind.data_ptr(),
                                  d_rank.data_ptr(), L.stream())
        assert rc == L.EMD_ERR_INVALID
        b.check()
        assert all((_read(t, m) == SENTINEL).all() for t in (d_src, d_kind, d_rank))


@pytest.mark.parametrize("n_keep,n_clone,n_split", [(0, 0, 1), (5, 3, 0), (0, 0, 300), (257, 100, 129), (1, 0, 1000)])
def test_densify_split_rank(n_keep, n_clone, n_split):
    L, lib = _lib()
    m = n_keep + n_clone + 2 * n_split
    b = Buffers()
    d_rank = b.out(m)
    assert lib.emd_densify_split_rank(m, n_keep, n_clone, n_split, d_rank.data_ptr(), L.stream()) == L.EMD_OK
    b.check()
    _expect(d_rank, R.split_rank_densify(m, n_keep, n_clone, n_split), "rank")


# ---- decide -> scan -> index chained ---------------------------------------------------------------------------------------------------------
def _chain(n, cols, decide, index, want_code, want_index):
    """Run decide -> scan -> index on the device, each link on the previous link's OUTPUT, and compare every intermediate with the reference."""
    L, lib = _lib()
    nb = (n + 255) // 256
    b = Buffers()
    d_code, d_col, d_tot = b.out(n), b.out(cols * nb), b.out(cols)
    assert decide(b, d_code, d_col) == L.EMD_OK
    b.check()
    _expect(d_code, want_code, "code")
    counts = R.block_counts(want_code, cols)
    _expect(d_col, counts, "block counts")
    assert lib.emd_densify_scan(n, cols, d_col.data_ptr(), d_tot.data_ptr(), L.stream()) == L.EMD_OK
    b.check()
    offsets, totals = R.exclusive_offsets(counts)
    _expect(d_col, offsets, "block offsets")
    _expect(d_tot, totals, "totals")
    m = len(want_index[0])
    outs = [b.out(m) for _ in want_index]
    assert index(m, d_code, d_col, d_tot, outs) == L.EMD_OK
    b.check()
    for name, got, want in zip(("src", "kind", "split_rank"), outs, want_index):
        _expect(got, want, name)
    return totals


def _densify_index_call(n):
    L, lib = _lib()
    return lambda m, code, off, tot, outs: lib.emd_densify_index(n, m, code.data_ptr(), off.data_ptr(), tot.data_ptr(), outs[0].data_ptr(),
                                                                 outs[1].data_ptr(), L.stream())


def _run_densify(n, inp):
    L, lib = _lib()

    def decide(b, d_code, d_col):
        a = L.EmdDensifyArgs()
        a.num_points, a.mode = n, L.DENSIFY_MODE_DENSIFY
        a.scaling, a.grad_accum, a.denom = (b.put(inp[k]).data_ptr() for k in ("scaling", "grad_accum", "denom"))
        a.grad_threshold, a.size_threshold = float(inp["grad_threshold"]), float(inp["size_threshold"])
        return lib.emd_densify_decide(C.byref(a), d_code.data_ptr(), d_col.data_ptr(), L.stream())
    code = R.decide_densify(inp["scaling"], inp["grad_accum"], inp["denom"], inp["grad_threshold"], inp["size_threshold"])
    _chain(n, 3, decide, _densify_index_call(n), code, R.index_densify(code))
    return code


def _run_prune(n, inp):
    L, lib = _lib()

    def decide(b, d_code, d_col):
        a = L.EmdDensifyArgs()
        a.num_points, a.mode = n, L.DENSIFY_MODE_PRUNE
        a.scaling, a.opacity, a.max_radii2D = (b.put(inp[k]).data_ptr() for k in ("scaling", "opacity", "max_radii2D"))
        if inp["extra_drop"] is not None:
            a.extra_drop = b.put(inp["extra_drop"]).data_ptr()
        a.min_opacity, a.max_screen_size, a.size_threshold = float(inp["min_opacity"]), float(inp["max_screen_size"]), float(inp["size_threshold"])
        return lib.emd_densify_decide(C.byref(a), d_code.data_ptr(), d_col.data_ptr(), L.stream())
    code = R.decide_prune(inp["scaling"], inp["opacity"], inp["max_radii2D"], inp["extra_drop"], inp["min_opacity"], inp["max_screen_size"],
                          inp["size_threshold"])
    _chain(n, 3, decide, _densify_index_call(n), code, R.index_densify(code))
    return code


def _run_refine(n, inp, flags, ns):
    L, lib = _lib()

    def decide(b, d_code, d_col):
        a = L.EmdRefineArgs()
        a.num_points = n
        a.do_densify, a.do_cull, a.use_split_screen, a.cull_big, a.use_cull_screen = flags
        a.scaling, a.opacity, a.grad_norm, a.vis_counts, a.max_2Dsize = (b.put(inp[k]).data_ptr()
                                                                         for k in ("scaling", "opacity", "grad_norm", "vis_counts", "max_2Dsize"))
        for k, v in inp["thr"].items():
            setattr(a, k, float(v))
        return lib.emd_refine_decide(C.byref(a), d_code.data_ptr(), d_col.data_ptr(), L.stream())

    def index(m, code, off, tot, outs):
        return lib.emd_refine_index(n, m, ns, code.data_ptr(), off.data_ptr(), tot.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                    L.stream())
    code = R.decide_refine(flags, inp["scaling"], inp["opacity"], inp["grad_norm"], inp["vis_counts"], inp["max_2Dsize"], inp["thr"])
    _chain(n, 4, decide, index, code, R.index_refine(code, ns))
    return code


CHAIN_N = [1, 255, 256, 257, 1000, 262401]          # the last: 1 026 blocks, the three-column scan makes its second trip


@pytest.mark.parametrize("n", CHAIN_N)
def test_chain_densify(n):
    """The hand rows (tests/density_ref.py:build_densify) hold the equalities: quotient == grad_threshold is hot (>=), the float below is not,
    0/0 counts as 0, x/0 as inf."""
    inp = R.build_densify(n, 10 + n)
    code = _run_densify(n, inp)
    assert code[inp["hand"]].tolist() == [3, 4, 1, 1, 4, 3, 1][:len(inp["hand"])]
    if n >= 1000:
        assert set(code.tolist()) == {1, 3, 4}


def test_chain_densify_with_a_zero_gradient_threshold():
    """grad_threshold == 0: every row is hot, the 0/0 rows (NaN -> 0 >= 0) included."""
    inp = R.build_densify(1000, 5, grad_threshold=0.0)
    code = _run_densify(1000, inp)
    assert code[inp["hand"]].tolist() == [3, 4, 4, 4, 4, 3, 3] and set(code.tolist()) == {3, 4}


@pytest.mark.parametrize("n", CHAIN_N)
@pytest.mark.parametrize("screen,extra,min_opacity", [(True, False, R.MIN_OPACITY), (False, False, R.MIN_OPACITY), (True, True, R.MIN_OPACITY),
                                                      (False, True, -1.0)], ids=["screen", "no-screen", "extra-drop", "prune-points"])
def test_chain_prune(n, screen, extra, min_opacity):
    """max_radii2D == max_screen_size stays; max_screen_size 0 turns the size tests off even for a huge, wide Gaussian; extra_drop bytes 1 and 255
    drop; min_opacity -1 with a mask is prune_points."""
    inp = R.build_prune(n, 20 + n, screen, extra, min_opacity)
    code = _run_prune(n, inp)
    want = [1, 0 if screen else 1, 0 if screen else 1, 0 if extra else 1, 0 if extra else 1, 1, 1 if min_opacity < 0 else 0]
    assert code[inp["hand"]].tolist() == want[:len(inp["hand"])]


@pytest.fixture(scope="module")
def refine_inputs():
    return R.build_refine(1000, 31), R.build_refine(1000, 32, cull_screen=-0.125)


@pytest.mark.parametrize("flags", R.ALL_REFINE_FLAGS, ids=lambda f: "".join(str(x) for x in f))
def test_chain_refine_in_every_flag_combination(refine_inputs, flags):
    """(do_densify, do_cull, use_split_screen, cull_big, use_cull_screen), with a positive and with a negative cull_screen (the latter culls every
    new row wherever the screen-size cull is on)."""
    for inp, ns in zip(refine_inputs, (2, 3)):
        code = _run_refine(1000, inp, flags, ns)
        assert set(code.tolist()) == R.refine_codes_possible(flags, inp["thr"])
    if flags == (1, 1, 1, 1, 1):
        inp = refine_inputs[0]
        code = R.decide_refine(flags, inp["scaling"], inp["opacity"], inp["grad_norm"], inp["vis_counts"], inp["max_2Dsize"], inp["thr"])
        assert code[inp["hand"]].tolist() == [1, 13, 1, 3, 15, 3, 13, 8, 1]


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_chain_refine_small(n):
    _run_refine(n, R.build_refine(n, 40 + n), (1, 1, 1, 1, 1), 2)


@pytest.mark.parametrize("flags", [(1, 1, 1, 1, 1), (1, 0, 0, 0, 0)], ids=lambda f: "".join(str(x) for x in f))
def test_chain_refine_at_1026_blocks(flags):
    _run_refine(262401, R.build_refine(262401, 50), flags, 2)


# ---- emd_after_train_stats -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("stride", [2, 3, 5])
def test_after_train_stats(n, stride):
    L, lib = _lib()
    rng = np.random.default_rng(100 * n + stride)
    radii = rng.integers(-3, 50, n).astype(np.int32)
    radii[rng.random(n) < 0.3] = 0
    if n == 1:
        radii[0] = 7
    else:
        radii[:3] = [0, -5, 12]
    grad = (rng.normal(size=(n, stride)) * 1e-3).astype(np.float32)
    norm0, vis0 = (rng.random(n) * 1e-3).astype(np.float32), rng.integers(0, 5, n).astype(np.float32)
    m2d0 = (rng.random(n) * 0.02).astype(np.float32)
    on = radii > 0
    for last_size in (1600.0, 37.0):
        want_norm = norm0.astype(np.float64) + np.hypot(grad[:, 0].astype(np.float64), grad[:, 1].astype(np.float64))
        want_vis = np.where(on, vis0 + np.float32(1), vis0)
        want_m2d = np.where(on, np.maximum(m2d0, radii.astype(np.float32) / np.float32(last_size)), m2d0)
        for absent in (None, 0, 1, 2):
            b = Buffers()
            d_radii, d_grad = b.put(radii), b.put(grad)
            outs = [None if absent == k else b.out(n) for k in range(3)]
            for t, init in zip(outs, (norm0, vis0, m2d0)):
                if t is not None:
                    t[:n] = torch.from_numpy(init.view(np.int32).copy()).to(DEV)
            ptr = [None if t is None else t.data_ptr() for t in outs]
            rc = lib.emd_after_train_stats(n, d_radii.data_ptr(), d_grad.data_ptr(), stride, ptr[0], ptr[1], ptr[2], last_size, L.stream())
            assert rc == L.EMD_OK
            b.check()
            if outs[0] is not None:
                got = _read(outs[0], n, np.float32)
                np.testing.assert_array_equal(got[~on].view(np.int32), norm0[~on].view(np.int32), err_msg="grad_norm of an invisible row")
                np.testing.assert_allclose(got[on].astype(np.float64), want_norm[on], rtol=1e-6, atol=0)
            if outs[1] is not None:
                np.testing.assert_array_equal(_read(outs[1], n, np.float32).view(np.int32), want_vis.view(np.int32), err_msg="vis_counts")
            if outs[2] is not None:
                np.testing.assert_array_equal(_read(outs[2], n, np.float32).view(np.int32), want_m2d.view(np.int32), err_msg="max_2Dsize")
    for bad_stride, bad_last in ((1, 1600.0), (2, 0.0)):
        b = Buffers()
        d_radii, d_grad = b.put(radii), b.put(grad)
        outs = [b.out(n) for _ in range(3)]
        rc = lib.emd_after_train_stats(n, d_radii.data_ptr(), d_grad.data_ptr(), bad_stride, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                       bad_last, L.stream())
        assert rc == L.EMD_ERR_INVALID
        b.check()
        assert all((_read(t, n) == SENTINEL).all() for t in outs)


# ---- threshold rounding ----------------------------------------------------------------------------------------------------------------------
def test_size_threshold_is_the_double_product_rounded_once():
    """percent_dense = 0.001, extent = 999.9999389648438: the reference's threshold percent_dense * extent, formed in double and rounded to float
    once, is 0.99999994; the product of the two floats is 1.0.  Hot Gaussians whose max exp(scale) is exactly 1.0 (expf(0) == 1) are split by the
    reference -- under the float product they would be cloned."""
    pd, extent = 0.001, 999.9999389648438
    scaling = np.array([[0, 0, 0], [0, -1, -2], [-3, 0, -1]], np.float32)
    ones = np.ones(3, np.float32)
    inp = dict(scaling=scaling, grad_accum=ones, denom=ones, grad_threshold=np.float32(R.GRAD_THRESHOLD), size_threshold=R.f32_product(pd, extent))
    assert float(inp["size_threshold"]) == float(np.float32(0.99999994)) < 1.0
    code = _run_densify(3, inp)
    assert code.tolist() == [R.SPLIT] * 3


def test_gaussian_model_hands_over_the_reference_thresholds():
    """The same case through GaussianModel.densify, whose host forms the product: (keep, clone, split) = (0, 0, 3).  And prune's 0.1 * extent with
    extent = 9.9999996: the double product rounds to 0.99999994, so a Gaussian of max exp(scale) 1.0 is dropped (rounded to float first, the
    extent is 10 and the threshold 1.0: it would stay); a small Gaussian beside them stays."""
    from emd_amd.gaussian_model import GaussianModel
    assert R.f32_product(0.1, 9.9999996) == np.float32(0.99999994) and np.float32(0.1) * np.float32(9.9999996) == np.float32(1.0)

    def model(scaling):
        n = len(scaling)
        m = GaussianModel(device=DEV)
        P = lambda t: torch.nn.Parameter(t.to(DEV).contiguous())
        m._xyz, m._scaling, m._opacity = P(torch.zeros(n, 3)), P(torch.tensor(scaling, dtype=torch.float32)), P(torch.zeros(n, 1))
        m._rotation = P(torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1))
        m._features_dc, m._features_rest, m._embedding = P(torch.zeros(n, 1, 3)), P(torch.zeros(n, 15, 3)), P(torch.zeros(n, 4))
        m._deformation_table = torch.ones(n, dtype=torch.bool, device=DEV)
        m.xyz_gradient_accum, m.denom, m.max_radii2D = torch.ones(n, 1, device=DEV), torch.ones(n, 1, device=DEV), torch.zeros(n, device=DEV)
        m.percent_dense = 0.001
        return m
    rows = [[0, 0, 0], [0, -1, -2], [-3, 0, -1]]
    with torch.no_grad():
        assert model(rows).densify(R.GRAD_THRESHOLD, 0.005, 999.9999389648438, None) == (0, 0, 3)
        m = model(rows + [[-3, -3, -3]])
        assert m.prune(R.GRAD_THRESHOLD, 0.005, 9.9999996, 20) == (1, 0, 0)
        assert m._scaling.shape[0] == 1 and m._scaling.detach().cpu().tolist() == [[-3.0, -3.0, -3.0]]
