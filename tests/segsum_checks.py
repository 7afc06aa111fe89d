"""The segmented row sum (emd_segmented_row_sum, include/emd_raster.h) restated in numpy on the CPU, written from the association pinned in
emd_amd/csrc/segsum.h and never from the kernels: a run of equal keys is cut into consecutive chunks of SEG_CHUNK elements, a chunk is summed in
ascending element order in fp64 from 0.0, the chunk sums are added in ascending chunk order in fp64 from 0.0, the result is rounded to fp32 once.
tests/test_deterministic_cpu.py pins it against typed-out cases; tests/test_segsum_gpu.py and tests/test_deterministic_gpu.py compare the HIP
kernels with it bit for bit."""
import numpy as np

SEG_CHUNK = 512           # EMD_SEG_CHUNK of include/emd_raster.h (tests/test_deterministic_cpu.py checks the three copies against each other)


def run_structure(keys):
    """keys [n] non-decreasing -> (start [R], length [R]) of the maximal runs of equal keys."""
    keys = np.asarray(keys)
    n = len(keys)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    assert (keys[1:] >= keys[:-1]).all(), "keys must be non-decreasing"
    start = np.flatnonzero(np.concatenate(([True], keys[1:] != keys[:-1])))
    return start, np.diff(np.concatenate((start, [n])))


def segsum_reference(keys, slots, rows, width, out, chunk=SEG_CHUNK):
    """keys / slots [n] (already cut to the element count), rows [.., pitch] float32, out [.., out_pitch] float32: written in place for the
    destinations that have a run (columns < width), left alone everywhere else.  -> out"""
    keys = np.asarray(keys).astype(np.int64)
    slots = np.asarray(slots).astype(np.int64)
    n = len(keys)
    if n == 0:
        return out
    start, length = run_structure(keys)
    run = np.repeat(np.arange(len(start)), length)             # run of every element
    pos = np.arange(n) - start[run]                              # its position in the run
    nchunk = (length + chunk - 1) // chunk
    first_chunk = np.concatenate(([0], np.cumsum(nchunk)[:-1]))  # number of a run's first chunk
    seg = first_chunk[run] + pos // chunk                        # chunk of every element
    within = pos % chunk
    vals = rows[slots, :width].astype(np.float64)                # (fp32 -> fp64 is exact)
    acc = np.zeros((int(nchunk.sum()), width), np.float64)       # every chunk starts from +0.0
    order = np.argsort(within, kind="stable")
    bounds = np.searchsorted(within[order], np.arange(int(within.max()) + 2))
    for q in range(len(bounds) - 1):                             # step q adds element q of every chunk: ascending element order inside a chunk
        idx = order[bounds[q]:bounds[q + 1]]
        acc[seg[idx]] = acc[seg[idx]] + vals[idx]                # (one element per chunk and step: no index repeats)
    total = np.zeros((len(start), width), np.float64)            # ... and the chunk sums in ascending chunk order, from +0.0
    for c in range(int(nchunk.max())):
        has = np.flatnonzero(nchunk > c)
        total[has] = total[has] + acc[first_chunk[has] + c]
    out[keys[start], :width] = total.astype(np.float32)          # one rounding (nearest even)
    return out


def segsum_scalar(values, chunk=SEG_CHUNK):
    """The association once more for ONE run of scalars, as the plainest loop: the typed-out cases pin segsum_reference against this and against
    hand-computed numbers."""
    total = np.float64(0.0)
    for c0 in range(0, len(values), chunk):
        acc = np.float64(0.0)
        for v in values[c0:c0 + chunk]:
            acc = acc + np.float64(np.float32(v))
        total = total + acc
    return np.float32(total)
