"""-m "not gpu": the host side of the deterministic backward -- struct layout, exported symbols, the option's default, the chunk constant in
its three places, workspace sizing, and the numpy restatement of the pinned association (tests/segsum_checks.py) on typed-out cases."""
import ctypes as C
import os
import re

import numpy as np

from emd_amd import _lib as L
from emd_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, RasterCall, RasterConfig, RasterOptions
from tests import segsum_checks as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "emd_raster.h")


def test_struct_sizes_match_the_c_compiler():
    """What the compiler cannot say (sizes, offsets and the header's constants: tests/test_abi.py): the flag's bit, the checker's chunk, the tail."""
    assert L.FLAG_DETERMINISTIC == 1 << 12
    assert L.SEG_CHUNK == sg.SEG_CHUNK
    # det_ws / det_bytes are the LAST two fields of EmdBwdArgs
    assert [f[0] for f in L.EmdBwdArgs._fields_[-2:]] == ["det_ws", "det_bytes"]
    assert L.EmdBwdArgs.det_bytes.offset + C.sizeof(C.c_size_t) == C.sizeof(L.EmdBwdArgs)


def test_chunk_constant_in_the_header_and_the_kernel_header():
    v = int(re.search(r"#define EMD_SEG_CHUNK (\d+)", open(HEADER).read()).group(1))
    assert v == L.SEG_CHUNK
    pinned = open(os.path.join(ROOT, "emd_amd", "csrc", "segsum.h")).read()
    assert f"static_assert(EMD_SEG_CHUNK == {v}" in pinned


def test_new_symbols_declared_listed_and_exported():
    lib = L.load()
    assert lib.emd_abi_version() == L.ABI_VERSION
    for name in ("emd_raster_det_workspace_size", "emd_raster_det_layout", "emd_segmented_row_sum", "emd_segmented_row_sum_workspace"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_option_defaults_off_and_reaches_every_surface():
    assert RasterOptions().deterministic is False and RasterConfig.deterministic is False
    assert RasterConfig.replace(deterministic=True).deterministic is True
    import torch
    rs = GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)
    assert GaussianRasterizer(rs).options.deterministic is False
    assert GaussianRasterizer(rs, deterministic=True).options.deterministic is True
    assert "det_state" in RasterCall.__slots__ and RasterCall().det_state is None


def test_workspace_size_formula():
    """The formula of include/emd_raster.h, restated: every array rounded up to 256 bytes."""
    up = lambda x: (x + 255) // 256 * 256

    def sort_bytes(n, group):
        return up(4 * n) * 5 + up(4 * 512 * ((n + 2047) // 2048)) + up(8 * group * 2 * ((n + L.SEG_CHUNK - 1) // L.SEG_CHUNK))

    for N, cap, nx in ((1, 1, 0), (3000, 65536, 0), (100000, 123457, 1), (2_000_000, 8_000_000, 2), (0, 0, 0)):
        n, R, p = max(N, 1), 4 * max(cap, 1), L.bwd_stride(nx)
        want = up(4 * R * p) + sort_bytes(R, 16 if 12 + 4 * nx <= 16 else 32) + up(64) + up(48 * n) + sort_bytes(n, 16) + 256
        assert L.det_workspace_size(N, cap, nx) == want
        lay = L.det_layout(N, cap, nx, 3)
        offs = [lay["rows"], *lay["keys"], *lay["slots"], lay["counts"], lay["pose_rows"], *lay["pose_keys"], *lay["pose_points"]]
        assert lay["rows"] == 0 and all(o % 256 == 0 for o in offs) and sorted(set(offs)) == sorted(offs) and max(offs) < want
    d = L.EmdDims(-1, 1, 1, 0, 0, 0)
    out = C.c_size_t()
    assert L.load().emd_raster_det_workspace_size(C.byref(d), C.byref(out)) == L.EMD_ERR_INVALID


def test_flag_without_workspace_is_refused_on_the_host():
    """Argument checking happens before any HIP call: no GPU needed."""
    lib = L.load()
    b = L.EmdBwdArgs()
    b.num_gaussians, b.flags, b.bin_capacity = 0, L.FLAG_DETERMINISTIC, 100
    b.s.image_height = b.s.image_width = 32
    b.s.tanfovx = b.s.tanfovy = 1.0
    fake = 1 << 20             # never dereferenced: the call is refused first
    b.radii = b.geom_ws = b.bin_ws = b.img_ws = b.bwd_ws = b.status = b.out_color = b.out_depth = fake
    b.geom_bytes = b.bin_bytes = b.img_bytes = b.bwd_bytes = 1 << 40
    assert lib.emd_raster_backward(C.byref(b), None) == L.EMD_ERR_WORKSPACE
    assert b"det_ws" in lib.emd_last_error()
    b.det_ws, b.det_bytes = fake, 16
    assert lib.emd_raster_backward(C.byref(b), None) == L.EMD_ERR_WORKSPACE
    b.det_bytes, b.pair_stats = 1 << 40, fake
    assert lib.emd_raster_backward(C.byref(b), None) == L.EMD_ERR_INVALID
    assert b"pair_stats" in lib.emd_last_error()


def _fake_det_backward(capacity):
    b = L.EmdBwdArgs()
    b.num_gaussians, b.flags, b.bin_capacity = 0, L.FLAG_DETERMINISTIC, capacity
    b.s.image_height = b.s.image_width = 32
    b.s.tanfovx = b.s.tanfovy = 1.0
    fake = 1 << 20             # never dereferenced: the call is refused first
    b.radii = b.geom_ws = b.bin_ws = b.img_ws = b.bwd_ws = b.status = b.out_color = b.out_depth = fake
    b.geom_bytes = b.bin_bytes = b.img_bytes = b.bwd_bytes = 1 << 62
    return b


def test_misaligned_workspace_is_refused_on_the_host():
    """det_ws is 64-byte aligned: a large enough workspace at another address is an invalid argument, not a short workspace."""
    lib = L.load()
    b = _fake_det_backward(100)
    b.det_ws, b.det_bytes = (1 << 20) + 32, 1 << 40
    assert lib.emd_raster_backward(C.byref(b), None) == L.EMD_ERR_INVALID
    assert b"det_ws" in lib.emd_last_error() and b"aligned" in lib.emd_last_error()


def test_slot_numbers_past_32_bits_are_refused_on_the_host():
    """4 x bin_capacity contribution slots are numbered in 32 bits, less one sort tile (2048 keys) that the sort rounds its launch up by."""
    lib = L.load()
    last = (2 ** 32 - 1 - 2048) // 4                         # the largest capacity the mode serves
    b = _fake_det_backward(last + 1)
    b.det_ws, b.det_bytes = 1 << 20, 1 << 62
    assert lib.emd_raster_backward(C.byref(b), None) == L.EMD_ERR_INVALID
    assert b"bin_capacity" in lib.emd_last_error()
    # the capacity below gets past that check: it is refused for its workspace (none given) instead
    b = _fake_det_backward(last)
    assert lib.emd_raster_backward(C.byref(b), None) == L.EMD_ERR_WORKSPACE
    assert b"det_ws" in lib.emd_last_error() and b"bin_capacity" not in lib.emd_last_error()


# ---- the restatement itself, on cases typed out by hand -------------------------------------------------------------------------------------
def _one_run(values, chunk):
    v = np.asarray(values, np.float32).reshape(-1, 1)
    out = np.full((1, 1), 99.0, np.float32)
    sg.segsum_reference(np.zeros(len(v), np.uint32), np.arange(len(v)), v, 1, out, chunk=chunk)
    return out[0, 0]


def test_restatement_typed_out_cases():
    big = 2.0 ** 60
    # one chunk, ascending: ((0 + big) + 1) - big = 0 in fp64 (1 is below half an ulp of 2^60), then + 1 = 1
    assert _one_run([big, 1.0, -big, 1.0], chunk=4) == 1.0
    # chunks of two: (big + 1) = big, (-big + 1) = -big, big + -big = 0
    assert _one_run([big, 1.0, -big, 1.0], chunk=2) == 0.0
    # chunks of three: (big - big) + 1 = 1, then the second chunk = 1: 0 + 1 + 1 = 2 (nothing is lost once the large terms have cancelled)
    assert _one_run([big, -big, 1.0, 1.0], chunk=3) == 2.0
    # one rounding at the end: 1 + 2^-24 + 2^-24 = 1 + 2^-23 exactly in fp64, an fp32 number; a running fp32 sum rounds each tie back to 1.0
    assert _one_run([1.0, 2.0 ** -24, 2.0 ** -24], chunk=512) == np.float32(1.0 + 2.0 ** -23) != np.float32(1.0)
    assert np.float32(np.float32(np.float32(1.0) + np.float32(2.0 ** -24)) + np.float32(2.0 ** -24)) == np.float32(1.0)
    # -0.0: every chunk and the total start from +0.0, and +0.0 + -0.0 = +0.0
    r = _one_run([-0.0, -0.0, -0.0], chunk=2)
    assert r == 0.0 and not np.signbit(r)
    # against the plain loop
    rng = np.random.default_rng(3)
    v = (rng.standard_normal(1300) * 10.0 ** rng.integers(-6, 12, 1300)).astype(np.float32)
    for chunk in (1, 7, 512, 2000):
        assert _one_run(v, chunk) == sg.segsum_scalar(v, chunk)


def test_restatement_runs_slots_and_untouched_rows():
    rows = np.array([[1, 10, 7], [2, 20, 7], [4, 40, 7], [8, 80, 7], [16, 160, 7]], np.float32)
    keys = np.array([1, 1, 4, 4, 4], np.uint32)           # destinations 0, 2, 3 have no run
    slots = np.array([4, 0, 3, 1, 2], np.uint32)
    out = np.full((5, 4), -1.0, np.float32)
    sg.segsum_reference(keys, slots, rows, 2, out)
    want = np.full((5, 4), -1.0, np.float32)
    want[1, :2], want[4, :2] = (17, 170), (14, 140)
    np.testing.assert_array_equal(out, want)
    start, length = sg.run_structure(keys)
    assert start.tolist() == [0, 2] and length.tolist() == [2, 3]
    empty = np.full((2, 2), 5.0, np.float32)
    sg.segsum_reference(np.zeros(0, np.uint32), np.zeros(0, np.uint32), rows, 2, empty)
    assert (empty == 5.0).all()
