"""-m gpu: the segmented row sum behind the deterministic backward, called directly (emd_segmented_row_sum) and compared BIT FOR BIT with
the numpy restatement of the pinned association (tests/segsum_checks.py, written from csrc/segsum.h, pinned by tests/test_deterministic_cpu.py).

Every comparison is `assert_array_equal` on the uint32 bit patterns of the whole output buffer: the rows of destinations with a run, the sentinel
in every float nobody may write (destinations without a run, the pad floats behind `width`), and 4096-word guards behind the output and the
partials.  keys, slots and rows must come back unchanged.  Sizes are the smallest at which each mechanism exists: 16 / 32 elements per batch of a
lane group, EMD_SEG_CHUNK elements per chunk, two chunk-sum slots per window of EMD_SEG_CHUNK elements."""
import ctypes as C

import numpy as np
import pytest
import torch

from emd_amd import _lib as L
from tests import segsum_checks as sg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xDEADBEEF             # pre-fill of the output and the guards (as a float: -6.26e18, never a sum of the inputs below)
GUARD = 4096
CH = sg.SEG_CHUNK
SHAPES = ((16, 12), (16, 16), (32, 20), (L.ACTOR_STRIDE, L.ACTOR_STRIDE))        # (row pitch, payload); the last one is the pose shape
RUN_LENGTHS = (1, 2, 63, 64, 65, CH - 1, CH, CH + 1, 3 * CH + 7)


def _dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV)


def _values(pattern, shape, rng):
    if pattern == "cancel":          # +-1e8 beside 1e-3: 59 bits between the largest and the smallest bit in play, more than fp64 carries
        big = rng.choice(np.array([1e8, -1e8, 0.0], np.float32), size=shape, p=[0.25, 0.25, 0.5])
        return (big + rng.standard_normal(shape).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    if pattern == "wide":            # +3e19 / -3e19 in every fourth row beside O(1): whether a small term survives depends on when the large ones cancel
        big = np.zeros(shape, np.float32)
        big[0::4], big[2::4] = 3e19, -3e19
        return np.where(big != 0, big, rng.standard_normal(shape).astype(np.float32)).astype(np.float32)
    if pattern == "negzero":
        return np.full(shape, -0.0, np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def _sum_and_check(keys, slots, rows, width, n_dest, out_pitch, n_dev=None, label="", twice=False):
    """One emd_segmented_row_sum call, checked in full against the restatement.  keys / slots [n_cap]; n_dev: device-side count (None: n_cap)."""
    keys, slots = np.ascontiguousarray(keys, np.uint32), np.ascontiguousarray(slots, np.uint32)
    n_cap, pitch = len(keys), rows.shape[1]
    n = n_cap if n_dev is None else n_dev
    lib = L.load()
    pbytes = lib.emd_segmented_row_sum_workspace(n_cap, width)
    out0 = np.full(n_dest * out_pitch + GUARD, SENT, np.uint32)
    par0 = np.full(pbytes // 4 + GUARD, SENT, np.uint32)
    t_keys, t_slots, t_rows = _dev_u32(keys), _dev_u32(slots), torch.from_numpy(rows).to(DEV)
    t_cnt = _dev_u32(np.array([n, SENT], np.uint32))
    want = out0.copy()
    sg.segsum_reference(keys[:n], slots[:n], rows, width, want[:n_dest * out_pitch].view(np.float32).reshape(n_dest, out_pitch))
    results = []
    for _ in range(2 if twice else 1):
        t_out, t_par = _dev_u32(out0), _dev_u32(par0)
        a = L.EmdSegSumArgs()
        a.keys, a.slots, a.n_dev, a.n_cap = t_keys.data_ptr(), t_slots.data_ptr(), (None if n_dev is None else t_cnt.data_ptr()), n_cap
        a.rows, a.row_pitch, a.width = t_rows.data_ptr(), pitch, width
        a.out, a.out_pitch = t_out.data_ptr(), out_pitch
        a.partials, a.partial_bytes = t_par.data_ptr(), pbytes
        rc = lib.emd_segmented_row_sum(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, f"{label}: {lib.emd_last_error()}"
        got = t_out.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got, want, err_msg=f"{label}: output rows / sentinels / guard (P={pitch} w={width} n={n}/{n_cap})")
        np.testing.assert_array_equal(t_par.cpu().numpy().view(np.uint32)[-GUARD:], par0[-GUARD:], err_msg=f"{label}: guard behind the partials")
        results.append(got)
    np.testing.assert_array_equal(t_keys.cpu().numpy().view(np.uint32), keys, err_msg=f"{label}: keys were written to")
    np.testing.assert_array_equal(t_slots.cpu().numpy().view(np.uint32), slots, err_msg=f"{label}: slots were written to")
    np.testing.assert_array_equal(t_rows.cpu().numpy(), rows, err_msg=f"{label}: rows were written to")
    np.testing.assert_array_equal(t_cnt.cpu().numpy().view(np.uint32), np.array([n, SENT], np.uint32), err_msg=f"{label}: the count was written to")
    if twice:
        np.testing.assert_array_equal(results[0], results[1], err_msg=f"{label}: two calls differ")
    return results[0]


def _keys_of_runs(lengths, skip=1):
    """Runs of the given lengths with destinations 0, skip, 2 skip, ... -> (keys, number of destinations)."""
    return np.repeat(np.arange(len(lengths), dtype=np.uint32) * skip, lengths), (len(lengths) - 1) * skip + 1


@pytest.mark.parametrize("pitch,width", SHAPES)
@pytest.mark.parametrize("order", ("ascending", "descending", "rotated"))
def test_run_lengths_at_every_seam(pitch, width, order):
    """Runs of 1, 2, 63, 64, 65, C - 1, C, C + 1 and 3 C + 7 elements in one call; three orders of the runs move every chunk start against the
    windows of C elements the chunk sums are filed under.  Slots are a random permutation: element order and memory order are unrelated."""
    rng = np.random.default_rng(pitch * 100 + width)
    lengths = list(RUN_LENGTHS)
    if order == "descending":
        lengths = lengths[::-1]
    elif order == "rotated":
        lengths = lengths[5:] + lengths[:5] + [CH + 1, 2 * CH, 1, 2 * CH + 1]
    keys, n_dest = _keys_of_runs(lengths)
    n = len(keys)
    rows = _values("cancel", (n + 5, pitch), rng)
    _sum_and_check(keys, rng.permutation(n + 5)[:n], rows, width, n_dest, pitch if pitch >= 16 else L.ACTOR_STRIDE, label=f"run lengths {order}")


@pytest.mark.parametrize("pitch,width", SHAPES[:1] + SHAPES[2:])
@pytest.mark.parametrize("structure", ("one_run", "all_single", "skipping", "empty", "device_count"))
def test_run_structures(pitch, width, structure):
    rng = np.random.default_rng(7)
    n_dev = None
    if structure == "one_run":
        keys, n_dest = np.full(4 * CH + 3, 5, np.uint32), 8
    elif structure == "all_single":
        keys, n_dest = np.arange(1500, dtype=np.uint32), 1500
    elif structure == "skipping":                  # destinations 0, 3, 6, ...: the rows between keep the sentinel
        keys, n_dest = _keys_of_runs([3, 1, CH + 2, 70, 2], skip=3)
    elif structure == "empty":
        keys, n_dest, n_dev = np.zeros(300, np.uint32), 4, 0
    else:                                          # the count on the device cuts a long run short; what lies behind it is not sorted and ignored
        keys, n_dest = _keys_of_runs([10, 2 * CH + 9, 40])
        n_dev = 10 + CH + 100
        keys = keys.copy()
        keys[n_dev:] = rng.integers(0, n_dest, len(keys) - n_dev)
    n = len(keys)
    rows = _values("cancel", (n, pitch), rng)
    _sum_and_check(keys, rng.permutation(n), rows, width, n_dest, 16 if width <= 16 else 32, n_dev=n_dev, label=structure)


@pytest.mark.parametrize("pitch,width", ((16, 12), (32, 20)))
def test_more_elements_than_one_sweep_of_the_grid(pitch, width):
    """Launch 1 is at most 16 384 workgroups of 16 (8) lane groups whose groups stride over the elements: 300 000 elements take a second sweep
    (a third for 32-lane groups), with a run of 2 C + 1 across the seam of the first sweep and the device-side count below the buffer."""
    rng = np.random.default_rng(5)
    sweep = 16384 * (256 // (16 if width <= 16 else 32))
    lengths = list(rng.integers(1, 9, 70000))
    cut = int(np.searchsorted(np.cumsum(lengths), sweep - CH))
    lengths[cut:cut] = [2 * CH + 1]                          # starts shortly before the seam, ends behind it
    keys, n_dest = _keys_of_runs(lengths, skip=2)
    n_dev = 300000
    assert len(keys) > n_dev + 1000 and np.cumsum(lengths)[cut - 1] < sweep < np.cumsum(lengths)[cut] and n_dev > sweep + 4 * CH
    n = len(keys)
    rows = _values("cancel", (n, pitch), rng)
    _sum_and_check(keys, rng.permutation(n), rows, width, n_dest, pitch, n_dev=n_dev, label="two sweeps")


@pytest.mark.parametrize("pattern", ("cancel", "wide", "negzero", "descending_slots"))
def test_value_patterns_pin_the_order(pattern):
    """Inputs on which another association gives other bits: heavy cancellation, a range beyond fp64's 53 bits, -0.0 (0.0 + -0.0 = +0.0: a run of
    -0.0 sums to +0.0), and slots in DESCENDING memory order (ascending element order is not ascending address order)."""
    rng = np.random.default_rng(11)
    keys, n_dest = _keys_of_runs([CH + 5, 3, 64, 2 * CH, 17, 1])
    n = len(keys)
    slots = np.arange(n)[::-1] if pattern == "descending_slots" else rng.permutation(n)
    rows = np.empty((n, 16), np.float32)
    rows[slots] = _values("wide" if pattern == "descending_slots" else pattern, (n, 16), rng)       # (the pattern follows the ELEMENT order)
    got = _sum_and_check(keys, slots, rows, 12, n_dest, 16, label=pattern, twice=True)
    if pattern == "negzero":
        assert (got[:n_dest * 16].reshape(n_dest, 16)[:, :12] == 0).all(), "a run of -0.0 must give +0.0 (bit pattern 0)"
    if pattern in ("wide", "descending_slots"):
        # the inputs do tell orders apart: the same elements summed in ascending ADDRESS order give other bits in the restatement itself
        a = np.zeros((n_dest, 16), np.float32)
        b = np.zeros((n_dest, 16), np.float32)
        sg.segsum_reference(keys, slots, rows, 12, a)
        sg.segsum_reference(keys, np.concatenate([np.sort(slots[keys == k]) for k in range(n_dest)]), rows, 12, b)
        assert not np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_bad_arguments_are_refused_before_any_launch():
    lib = L.load()
    a = L.EmdSegSumArgs()
    a.n_cap, a.width, a.row_pitch, a.out_pitch = 10, 33, 40, 40
    assert lib.emd_segmented_row_sum(C.byref(a), None) == L.EMD_ERR_INVALID and b"width" in lib.emd_last_error()
    a.width = 12
    assert lib.emd_segmented_row_sum(C.byref(a), None) == L.EMD_ERR_INVALID and b"null" in lib.emd_last_error()
    t = torch.zeros(64, device=DEV, dtype=torch.float64)
    a.keys = a.slots = a.rows = a.out = a.partials = t.data_ptr()
    a.partial_bytes = 8
    assert lib.emd_segmented_row_sum(C.byref(a), None) == L.EMD_ERR_WORKSPACE and b"partials" in lib.emd_last_error()
