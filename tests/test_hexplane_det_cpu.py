"""-m "not gpu": the host side of the deterministic HexPlane backward (EMD_HEX_FLAG_DETERMINISTIC) -- the struct extension,
the exported symbols, workspace sizing against the header's formula, the refusals decided before any launch, the Python switches."""
import ctypes as C
import os

from emd_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "emd_raster.h")
NEW_SYMBOLS = ("emd_hexplane_det_workspace_size", "emd_hexplane_det_workspace_offsets")


def _args(N, Cc, res=((16, 12, 10, 6),)):
    a = L.EmdHexArgs()
    a.num_points, a.channels, a.num_scales = N, Cc, len(res)
    for s, r in enumerate(res):
        for k in range(4):
            a.res[s][k] = r[k]
    return a


def test_new_symbols_declared_listed_and_exported():
    lib, header = L.load(), open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name) and f"int {name}(" in header
    assert "#define EMD_HEX_FLAG_DETERMINISTIC 1u" in header
    assert lib.emd_abi_version() == 31                  # a compatible extension: it kept the version (31 since EmdDensifyArgs.size_threshold)


def test_grads_struct_matches_the_c_compiler():
    """(Size, offsets and the flag's value against the compiler: tests/test_abi.py.)"""
    G = L.EmdHexGrads
    assert L.HEX_FLAG_DETERMINISTIC == 1
    # `flags` took the place of `reserved`; the three new fields are appended behind the last field of the earlier layout
    names = [f[0] for f in G._fields_]
    assert names[-5:] == ["flags", "dL_dtime_sum", "det_ws", "det_bytes", "det_keep_plane"] and "reserved" not in names
    assert G().flags == 0 and G().det_keep_plane == 0


def test_workspace_size_is_host_only_monotone_and_the_headers_formula():
    """The formula of include/emd_raster.h, restated: every array rounded up to 256 bytes.  Runs without a GPU, so the entry is host-only."""
    up = lambda x: (x + 255) // 256 * 256
    chunks = lambda n: (n + L.SEG_CHUNK - 1) // L.SEG_CHUNK

    def sort_bytes(m, group):
        return up(4 * m) * 5 + up(4 * 512 * ((m + 2047) // 2048)) + up(8 * group * 2 * chunks(m))

    def want(N, Cc):
        n = max(N, 1)
        return up(16 * n * Cc) + sort_bytes(4 * n, 16 if Cc <= 16 else 32) + up(64) + 3 * up(4 * n) + up(8 * 16 * 2 * chunks(n)) + 256

    for N in (0, 1, 255, 513, 30011, 2_000_000):
        for Cc in (1, 4, 16, 32):
            assert L.hex_det_workspace_size(_args(N, Cc)) == want(N, Cc)
    sizes = [L.hex_det_workspace_size(_args(N, 32)) for N in (1, 2, 100, 30011, 30012, 10 ** 6, 2 * 10 ** 6)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[2] < sizes[3] < sizes[5] < sizes[6]
    # the largest plane of the call: never a smaller workspace for a larger plane (in this layout it sets the number of sort passes only)
    by_plane = [L.hex_det_workspace_size(_args(30011, 32, ((r, r, r, 6), (2 * r, r, r, 6)))) for r in (2, 16, 100, 512, 4096)]
    assert by_plane == sorted(by_plane)
    # the offsets name distinct aligned arrays inside the reported size, and the pass count is ceil(log2(W H)) bits in passes of at most nine
    a = _args(30011, 32, ((16, 12, 10, 6), (512, 512, 512, 25)))
    for plane, passes in ((1, 1), (3, 1), (7, 2), (9, 2), (12, 2)):           # 16 x 12 = 192 texels: 8 bits; 512 x 512: 18 bits; 512 x 25: 14 bits
        lay = L.hex_det_layout(a, plane)
        offs = [lay[k] for k in ("rows", "keys", "slots", "time_column", "raw_keys", "counts")]
        assert lay["rows"] == 0 and all(o % 256 == 0 for o in offs) and len(set(offs)) == len(offs) and max(offs) < lay["bytes"]
        assert lay["passes"] == passes and lay["bytes"] == L.hex_det_workspace_size(a)
    out = C.c_size_t()
    assert L.load().emd_hexplane_det_workspace_size(C.byref(_args(10, 64)), C.byref(out)) == L.EMD_ERR_INVALID
    assert L.load().emd_hexplane_det_workspace_offsets(C.byref(a), 13, (C.c_size_t * 8)()) == L.EMD_ERR_INVALID


def _fake_call(Cc):
    fake = 1 << 20             # never dereferenced: the call is refused first
    a = _args(1000, Cc)
    for p in range(6):
        a.planes[0][p] = fake
    a.pts = a.times = fake
    g = L.EmdHexGrads()
    g.dL_dout, g.flags = fake, L.HEX_FLAG_DETERMINISTIC
    for p in range(6):
        g.dL_dplanes[0][p] = fake
    return a, g


def test_flag_without_workspace_is_refused_on_the_host():
    """Argument checking happens before any HIP call: no GPU needed."""
    lib = L.load()
    a, g = _fake_call(32)
    assert lib.emd_hexplane_backward(C.byref(a), C.byref(g), None) == L.EMD_ERR_WORKSPACE
    assert b"det_ws" in lib.emd_last_error()
    g.det_ws, g.det_bytes = 1 << 20, L.hex_det_workspace_size(a) - 1
    assert lib.emd_hexplane_backward(C.byref(a), C.byref(g), None) == L.EMD_ERR_WORKSPACE
    g.det_ws, g.det_bytes = (1 << 20) + 64, 1 << 40
    assert lib.emd_hexplane_backward(C.byref(a), C.byref(g), None) == L.EMD_ERR_INVALID and b"aligned" in lib.emd_last_error()
    g.det_ws, g.det_keep_plane = 1 << 20, 7                    # one scale: planes 1 .. 6
    assert lib.emd_hexplane_backward(C.byref(a), C.byref(g), None) == L.EMD_ERR_INVALID and b"det_keep_plane" in lib.emd_last_error()


def test_flag_with_64_channels_is_refused_on_the_host():
    lib = L.load()
    a, g = _fake_call(64)
    g.det_ws, g.det_bytes = 1 << 20, 1 << 40
    assert lib.emd_hexplane_backward(C.byref(a), C.byref(g), None) == L.EMD_ERR_INVALID
    assert b"32 channels" in lib.emd_last_error()


def test_slot_numbers_past_32_bits_are_refused_on_the_host():
    """4 N slots are numbered in 32 bits, less one sort tile (2048 keys) per tap: num_points < 2^30 - 2048."""
    lib = L.load()
    a, g = _fake_call(32)
    a.num_points = 2 ** 30 - 2048
    assert lib.emd_hexplane_backward(C.byref(a), C.byref(g), None) == L.EMD_ERR_INVALID
    assert b"32 bits" in lib.emd_last_error()
    # one point less gets past that check: the call is refused for its workspace (none given) instead
    a.num_points -= 1
    assert lib.emd_hexplane_backward(C.byref(a), C.byref(g), None) == L.EMD_ERR_WORKSPACE
    assert b"det_ws" in lib.emd_last_error()


def test_python_switches_default_off():
    from emd_amd.deformation import DeformOptions
    from emd_amd.hexplane import DeterministicSum, HexPlaneField
    assert HexPlaneField.deterministic is False and DeformOptions().deterministic is False and DeformOptions(deterministic=True).deterministic is True
    cfg = {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 4, "resolution": [4, 4, 4, 2]}
    field = HexPlaneField(1.6, cfg, [1])
    assert field.deterministic is False and field.det_state is None
    rec = DeterministicSum()
    assert rec.keep_plane is None and rec.order is None and rec.det_state is None
