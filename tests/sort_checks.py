"""Reference of the device radix sort (emd_radix_sort, include/emd_raster.h) in numpy on the CPU, written from the contract in
emd_amd/csrc/radix_sort.h and never from the kernels.  tests/test_sort_cpu.py pins it against typed-out cases; tests/test_sort_gpu.py compares
the HIP sort with it, exactly and at every position."""
import numpy as np

DROPPED = 0xFFFFFFFF          # a compacting sort leaves elements with this key out
SORT_TILE, WAVE_SLICE, ROUND = 2048, 512, 64          # keys per sort block, per wave of a block, per ballot round: where the failure report points


def result_index(compacting, passes):
    """Which of the two buffer pairs holds the result (emd_radix_result_buf of csrc/common.h, restated)."""
    return 0 if passes < 1 else (passes - (1 if compacting else 0)) & 1


def sort_reference(keys, vals=None, *, passes, bits, offset=0, range_bits=32, n_dev=None, n_dev_overflow=0):
    """keys [n_cap] uint32; vals [n_cap] uint32, or None for a compacting sort (values = element indices, keys == DROPPED left out).
    -> (sorted keys, sorted values, count, overflow word, result index)"""
    compacting = vals is None
    n = len(keys) if n_dev is None else int(n_dev)
    if n_dev is not None and n_dev_overflow:
        n = 0
    k = np.asarray(keys, dtype=np.uint32)[:n]
    v = np.arange(n, dtype=np.uint32) if compacting else np.asarray(vals, dtype=np.uint32)[:n]
    if compacting:
        keep = k != DROPPED
        k, v = k[keep], v[keep]
    rel = (k.astype(np.int64) - int(offset)) & 0xFFFFFFFF
    width = passes * bits                                      # (16-bit sort keys take numpy's fast stable path: the multi-million-element cases)
    order = np.argsort((rel & ((1 << width) - 1)).astype(np.uint16 if width <= 16 else np.uint32), kind="stable")
    overflow = 2 if compacting and range_bits < 32 and bool((rel >> range_bits).any()) else 0
    return k[order], v[order], len(k), overflow, result_index(compacting, passes)


def describe(pos, key, *, passes, bits, offset=0):
    """Where output position `pos` lies in the sort's geometry, and the digit of `key` in every pass: the text of a failure."""
    rel = (int(key) - int(offset)) & 0xFFFFFFFF
    digits = ", ".join(f"pass {p}: {(rel >> (p * bits)) & ((1 << bits) - 1)}" for p in range(passes))
    return (f"position {pos} (sort block {pos // SORT_TILE}, wave slice {pos % SORT_TILE // WAVE_SLICE}, round {pos % WAVE_SLICE // ROUND}, "
            f"lane {pos % ROUND}), key 0x{int(key):08X}, digits of key - offset [{digits}]")


def assert_same(what, got, want, report_keys=None, **geometry):
    """got == want at every position, or an AssertionError that names the first differing position (`describe`, with the key that belongs
    there: report_keys[p], or want[p] when the arrays are the keys themselves)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: {got.shape[0]} elements, expected {want.shape[0]}"
    bad = np.flatnonzero(got != want)
    if len(bad):
        p = int(bad[0])
        where = describe(p, (want if report_keys is None else report_keys)[p], **geometry) if geometry else f"position {p}"
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} positions differ, the first at {where}: got 0x{int(got[p]):08X}, expected 0x{int(want[p]):08X}")
