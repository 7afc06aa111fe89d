"""-m "not gpu": the slice arithmetic of the render backward's dL/dshs fill (csrc/common.h, emd_fill_per / emd_fill_slice), through its thin C entry
point emd_backward_fill_slice -- the very functions the launcher and the kernel call.  Workgroup b of `grid` zeroes [lo_b, hi_b) of `count` 16-byte
elements; for every (count, grid) below the slices, taken in workgroup order, are disjoint, ascending and cover [0, count) exactly, every slice
but the last non-empty one is a whole number of 64-lane store instructions, and no slice is longer than ceil(count / grid) rounded up to 64."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from emd_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = (24_000_000, 26_816)          # 2 M Gaussians x 12 float4; 4 x the padded tile grid of a 1066 x 1600 image


def slices(count, grid):
    lib, out = L.load(), (C.c_uint64 * 2)()
    got = np.empty((grid, 2), dtype=np.uint64)
    for b in range(grid):
        assert lib.emd_backward_fill_slice(count, grid, b, out) == L.EMD_OK
        got[b] = out[0], out[1]
    return got


def pairs():
    out = [HEADLINE, (HEADLINE[0] + 1, HEADLINE[1]), (444, 128), (12, 128), ((1 << 32) + 77, 4096), (12 * 358_000_000, 26_816)]
    for grid in (1, 3, 128, 26_816):
        for count in (0, 1, 63, 64, 65, grid - 1, grid, grid + 1, 64 * grid - 1, 64 * grid, 64 * grid + 1):
            out.append((count, grid))
    return sorted(set(out))


def test_the_entry_point_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "emd_raster.h")).read()
    assert "emd_backward_fill_slice" in L.EXPORTED_SYMBOLS and hasattr(L.load(), "emd_backward_fill_slice")
    assert re.search(r"\bint emd_backward_fill_slice\(", header)


@pytest.mark.parametrize("count, grid", pairs(), ids=lambda v: str(v))
def test_slices_are_disjoint_ordered_and_cover_the_range(count, grid):
    s = slices(count, grid).astype(object)          # (Python integers: counts beyond 2^63 never occur, sums beyond 2^64 must not wrap silently)
    lo, hi = s[:, 0], s[:, 1]
    assert lo[0] == 0 and hi[-1] == count
    assert all(a <= b for a, b in zip(lo, hi)), "a slice ends in front of its start"
    assert all(hi[b] == lo[b + 1] for b in range(grid - 1)), "two neighbouring slices overlap or leave a gap"
    length = hi - lo
    per = -(-count // grid)
    per = (per + 63) // 64 * 64
    assert all(n <= per for n in length)
    filled = [n for n in length if n]
    assert sum(filled) == count
    assert all(n % 64 == 0 for n in filled[:-1]), "a slice in front of the last one is not a whole number of 1 KB store instructions"
    # the workgroups past the end hold the empty slice [count, count): nothing to store, no address formed
    first_empty = len(filled)
    assert all(lo[b] == hi[b] == count for b in range(first_empty, grid))


def test_the_headline_shape():
    s = slices(*HEADLINE)
    n = (s[:, 1] - s[:, 0]).astype(np.int64)
    assert n.max() == 896 and (n == 896).sum() == HEADLINE[0] // 896          # 14 store instructions per wave; the last workgroups idle
    assert int(n.sum()) == HEADLINE[0]


def test_invalid_arguments():
    lib, out = L.load(), (C.c_uint64 * 2)()
    assert lib.emd_backward_fill_slice(10, 0, 0, out) == L.EMD_ERR_INVALID
    assert lib.emd_backward_fill_slice(10, 4, 4, out) == L.EMD_ERR_INVALID and b"backward_fill_slice" in lib.emd_last_error()
    assert lib.emd_backward_fill_slice(10, 4, 0, None) == L.EMD_ERR_INVALID
