"""-m "not gpu": the numpy reference of the binning stage (tests/binning_checks.py) against typed-out cases and against the C oracle's sorted list,
the text of its failure reports, and the argument validation of emd_raster_binning, which needs no GPU: every call below fails before anything is
launched."""
import ctypes as C

import numpy as np
import pytest

from emd_amd import _lib as L
from tests import binning_checks as bc

U = lambda *x: np.array(x, dtype=np.uint32)
F = lambda *x: np.array(x, dtype=np.float32).view(np.uint32)


def test_one_tile():
    ref = bc.binning_reference(F(1.0, 0.5, 2.0), bc.make_binrec(0, 0, 1, 1, n=3), H=16, W=16, capacity=8)
    assert (ref["V"], ref["D"], ref["overflow"], ref["T"]) == (3, 3, 0, 1) and ref["status"] == (3, 0, 3, 3)
    assert ref["perm"].tolist() == [1, 0, 2] and ref["ids"].tolist() == [1, 0, 2] and ref["tiles"].tolist() == [0, 0, 0]
    assert ref["masks"].tolist() == [15, 15, 15] and ref["ranges"].tolist() == [[0, 3]]
    assert ref["keys"].tolist() == [0x3F000000, 0x3F800000, 0x40000000]
    assert ref["bucket"].tolist() == [0] and not ref["identity_order"]


@pytest.mark.parametrize("skip, masks", [(0, [15, 15, 15, 15]), (1, [10, 15, 10, 15]), (2, [15, 5, 15, 5]), (4, [12, 12, 15, 15]), (8, [15, 15, 3, 3]),
                                         (15, [8, 4, 2, 1])])
def test_two_by_two_rectangle_with_each_skip_bit(skip, masks):
    """x0 = 1, y0 = 0 on a 3 x 3 grid: tiles 1, 2, 4, 5 in row-major order; bit qy * 2 + qx."""
    ref = bc.binning_reference(F(1.0), bc.make_binrec(1, 0, 2, 2, skip, upper=0xABCDE), H=48, W=48, capacity=4)
    assert ref["tiles"].tolist() == [1, 2, 4, 5] and ref["ids"].tolist() == [0, 0, 0, 0]
    assert ref["masks"].tolist() == masks
    assert ref["ranges"].tolist() == [[0, 0], [0, 1], [1, 2], [0, 0], [2, 3], [3, 4], [0, 0], [0, 0], [0, 0]]


def test_width_one_with_both_skip_bits_has_no_quadrant():
    ref = bc.binning_reference(F(1.0, 1.0, 1.0), bc.make_binrec(0, 0, [1, 1, 3], [1, 3, 1], [3, 12, 15]), H=48, W=48, capacity=16)
    assert ref["masks"].tolist() == [0, 12, 0, 0, 0, 15, 3] and ref["tiles"].tolist() == [0, 0, 0, 1, 2, 3, 6]
    assert ref["ids"].tolist() == [0, 1, 2, 2, 2, 1, 1]


def test_depth_tie_keeps_id_order_and_culled_ids_are_left_out():
    keys = F(3.0, 1.0, 3.0, 0.0, 1.0, 3.0)
    keys[3] = bc.CULLED
    ref = bc.binning_reference(keys, bc.make_binrec([0, 1, 0, 0, 0, 1], 0, [2, 1, 1, 2, 2, 1], 1), H=16, W=32, capacity=100)
    assert ref["perm"].tolist() == [1, 4, 0, 2, 5] and (ref["V"], ref["D"]) == (5, 7)
    assert ref["dup_id"].tolist() == [1, 4, 4, 0, 0, 2, 5] and ref["dup_tile"].tolist() == [1, 0, 1, 0, 1, 0, 1]
    assert ref["ids"].tolist() == [4, 0, 2, 1, 4, 0, 5] and ref["tiles"].tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert ref["ranges"].tolist() == [[0, 3], [3, 7]] and ref["status"] == (7, 0, 5, 5)
    assert ref["src"].tolist() == [1, 3, 5, 0, 2, 4, 6]


def test_empty_tile_between_two_full_ones_and_zero_pair_gaussians():
    # Gaussian 1 is visible with a rectangle of width 0: it counts towards V and emits nothing
    ref = bc.binning_reference(F(2.0, 1.5, 1.0), bc.make_binrec([0, 1, 2], 0, [1, 0, 1], [1, 1, 1]), H=16, W=48, capacity=2)
    assert (ref["V"], ref["D"], ref["overflow"]) == (3, 2, 0)
    assert ref["ids"].tolist() == [0, 2] and ref["tiles"].tolist() == [0, 2] and ref["ranges"].tolist() == [[0, 1], [0, 0], [1, 2]]
    assert ref["counts"].tolist() == [1, 0, 1] and ref["starts"].tolist() == [0, 1, 1]


def test_overflow_bits_and_capacity_zero():
    rec = bc.make_binrec(0, 0, 2, 1, n=2)
    ref = bc.binning_reference(F(1.0, 2.0), rec, H=16, W=32, capacity=3)
    assert ref["status"] == (4, 1, 2, 2) and ref["ids"] is None and ref["ranges"].tolist() == [[0, 0], [0, 0]] and not ref["identity_order"]
    ref = bc.binning_reference(F(1.0, 2.0), rec, H=16, W=32, capacity=0)
    assert ref["status"] == (4, 1, 2, 2) and ref["identity_order"]
    assert bc.binning_reference(F(1.0, 2.0), bc.make_binrec(0, 0, 0, 1, n=2), H=16, W=32, capacity=0)["status"] == (0, 0, 2, 2)
    # narrow: key - bits(0.2f) must fit 27 bits; 0.2 * 65536 is the first depth that does not
    far = F(0.2 * 65536.0)
    assert int(far[0]) - bc.near_bits(0.2) == 1 << 27
    assert bc.binning_reference(np.concatenate([F(1.0), far]), rec, H=16, W=32, capacity=4)["status"] == (4, 2, 2, 2)
    assert bc.binning_reference(np.concatenate([F(1.0), far - 1]), rec, H=16, W=32, capacity=4)["status"] == (4, 0, 2, 2)
    assert bc.binning_reference(np.concatenate([F(1.0), far]), rec, H=16, W=32, capacity=3)["status"] == (4, 3, 2, 2)
    assert bc.binning_reference(np.concatenate([F(1.0), far]), rec, H=16, W=32, capacity=4, wide=True)["status"] == (4, 0, 2, 2)
    assert bc.binning_reference(F(0.1), bc.make_binrec(0, 0, 1, 1), H=16, W=16, capacity=4)["overflow"] == 2         # in front of the near plane: it wraps
    assert bc.binning_reference(F(0.1), bc.make_binrec(0, 0, 1, 1), H=16, W=16, capacity=4, near_plane=0.1)["overflow"] == 0


def test_no_gaussians():
    ref = bc.binning_reference(U(), np.zeros((0, 2), np.uint32), H=20, W=40, capacity=7)
    assert ref["status"] == (0, 0, 0, 0) and ref["T"] == 6 and ref["identity_order"] and not ref["ranges"].any() and len(ref["ids"]) == 0


def test_tile_order_contract():
    # list lengths 40, 0, 16, 15, 17 -> buckets 2, 0, 1, 0, 1
    ref = bc.binning_reference(np.full(88, 0x3F800000, np.uint32), bc.make_binrec(np.repeat([0, 2, 3, 4], [40, 16, 15, 17]), 0, 1, 1), H=16, W=80, capacity=100)
    assert ref["bucket"].tolist() == [2, 0, 1, 0, 1]
    bc.assert_tile_order("order", U(0, 2, 4, 1, 3), ref)
    bc.assert_tile_order("order", U(0, 4, 2, 3, 1), ref)
    for bad, text in ((U(2, 0, 4, 1, 3), "increases at position 1"), (U(0, 2, 4, 1, 1), "not a permutation"), (U(0, 2, 4, 1, 5), "not a permutation"),
                      (U(0, 2, 4, 1), "entries")):
        with pytest.raises(AssertionError, match=text):
            bc.assert_tile_order("order", bad, ref)
    ref["identity_order"] = True
    bc.assert_tile_order("order", U(0, 1, 2, 3, 4), ref)
    with pytest.raises(AssertionError, match="identity"):
        bc.assert_tile_order("order", U(0, 2, 4, 1, 3), ref)
    assert bc.binning_reference(F(1.0), bc.make_binrec(0, 0, 1, 1), H=16 * 257, W=16 * 256, capacity=1)["identity_order"]          # T = 65 792
    assert not bc.binning_reference(F(1.0), bc.make_binrec(0, 0, 1, 1), H=16 * 256, W=16 * 256, capacity=1)["identity_order"]      # T = 65 536
    ref = bc.binning_reference(F(1.0), bc.make_binrec(0, 0, 1, 1023), H=16 * 1023, W=16, capacity=20000)
    assert ref["bucket"].tolist() == [0] * 1023
    ref = bc.binning_reference(np.full(20000, 0x3F800000, np.uint32), bc.make_binrec(0, 0, 1, 1, n=20000), H=16, W=16, capacity=20000)
    assert ref["bucket"].tolist() == [1023]                                                                                          # the cap


def test_failure_text_names_window_gaussian_block_and_offset():
    n = 300
    keys = F(*np.linspace(1.0, 2.0, n)[::-1])                  # id i has depth rank n - 1 - i
    ref = bc.binning_reference(keys, bc.make_binrec(0, 0, 4, 4, n=n), H=64, W=64, capacity=n * 16)
    want = ref["ids"].copy()
    p = 2 * n + 7                                              # tile 2's eighth entry: depth rank 7, the third pair of its run
    got = want.copy()
    got[p] ^= 1
    with pytest.raises(AssertionError) as e:
        bc.assert_list("ids", got, want, ref)
    msg = str(e.value)
    assert f"sorted position {p} (tile 2) <- emission slot {7 * 16 + 2} (window 0, slot 114 of it)" in msg, msg
    assert "owned by Gaussian 292 = depth rank 7 (block 0, lane 7), offset 2 of its run of 16 starting at slot 112" in msg, msg
    p = 15 * n + 299                                           # the last pair of all: rank 299 sits in block 1, its run in window 2
    assert "(window 2, slot 703 of it), owned by Gaussian 0 = depth rank 299 (block 1, lane 43), offset 15" in bc.describe(ref, p)
    with pytest.raises(AssertionError, match="tile 3: got \\(1, 2\\), expected \\(900, 1200\\)"):
        r = ref["ranges"].copy()
        r[3] = (1, 2)
        bc.assert_ranges("ranges", r, ref["ranges"])


def test_reference_equals_the_oracle_list():
    """The C oracle sorts (tile << 32 | depth bits, id) with qsort; the reference orders depth first and tiles second.  Same list, entry for entry."""
    from tests.helpers import make_case, run_oracle
    case = make_case(n=3000, H=70, W=90, seed=3)
    orc = run_oracle(case)
    pre, b = orc["pre"], orc["bin"]
    rect = pre["rect"].astype(np.int64)
    vis = pre["tiles_touched"] > 0
    assert 1000 < vis.sum() < 3000 and b["D"] > 3000
    depth_key = np.where(vis, pre["depths"].view(np.uint32), bc.CULLED).astype(np.uint32)
    rec = bc.make_binrec(rect[:, 0], rect[:, 1], rect[:, 2] - rect[:, 0], rect[:, 3] - rect[:, 1])
    rec[~vis] = 0xFFFFFFFF                                     # a culled Gaussian's record is never read
    ref = bc.binning_reference(depth_key, rec, H=70, W=90, capacity=b["D"], near_plane=case["near_plane"])
    assert ref["status"] == (b["D"], 0, int(vis.sum()), int(vis.sum()))
    np.testing.assert_array_equal(ref["keys"], b["keys"])
    np.testing.assert_array_equal(ref["ids"], b["ids"])
    np.testing.assert_array_equal(ref["ranges"], b["ranges"])
    assert (ref["masks"] == 15).all()
    wide = bc.binning_reference(depth_key, rec, H=70, W=90, capacity=b["D"], wide=True)
    np.testing.assert_array_equal(wide["keys"], b["keys"])
    np.testing.assert_array_equal(wide["ids"], b["ids"])


# ---- emd_raster_binning: what the host refuses before anything is launched ----------------------------------------------------------------------
def _args(**kw):
    one = 256                                                # a non-null pointer that is never dereferenced: validation fails first
    a = L.EmdBinningArgs()
    a.num_gaussians, a.image_height, a.image_width, a.flags, a.near_plane, a.bin_capacity = 1000, 64, 96, 0, 0.2, 5000
    a.depth_key = a.binrec = a.geom_ws = a.bin_ws = a.status = a.tile_order = one
    a.geom_bytes, a.bin_bytes, _, _ = L.workspace_sizes(1000, 64, 96, 5000)
    for name, v in kw.items():
        setattr(a, name, v(a.geom_bytes, a.bin_bytes) if callable(v) else v)
    return a


@pytest.mark.parametrize("kw, code, text", bc.BAD_ARGUMENTS)
def test_invalid_arguments(kw, code, text):
    lib = L.load()
    assert lib.emd_raster_binning(C.byref(_args(**kw)), None) == code, kw
    assert text in lib.emd_last_error(), (kw, lib.emd_last_error())


def test_null_args_and_symbol():
    lib = L.load()
    assert "emd_raster_binning" in L.EXPORTED_SYMBOLS
    assert lib.emd_raster_binning(None, None) == L.EMD_ERR_INVALID and b"null" in lib.emd_last_error()
