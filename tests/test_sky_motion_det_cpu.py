"""-m "not gpu": the host side of the deterministic sky and motion backward (emd_sky_backward_det, emd_motion_backward_det; DESIGN.md section
8.10) -- the exported symbols, workspace sizing against the formulas of include/emd_raster.h, the offsets, the refusals decided before any
launch, the Python switches."""
import ctypes as C
import inspect
import os
import re
import types

from emd_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "emd_raster.h")
NEW_SYMBOLS = {"emd_sky_det_workspace_size": "size_t", "emd_sky_det_workspace_offsets": "int", "emd_sky_backward_det": "int",
               "emd_motion_det_workspace_size": "size_t", "emd_motion_det_workspace_offsets": "int", "emd_motion_backward_det": "int"}
SLOT_LIMIT = 2 ** 32 - 1 - 2048         # 4 P (sky) and 4 n (motion) at most

up = lambda x: (x + 255) // 256 * 256
chunks = lambda n: (n + L.SEG_CHUNK - 1) // L.SEG_CHUNK


def sort_bytes(m, group):
    """sort(m, g) of the header: raw keys and two ping-pong pairs, the histograms, the fp64 chunk sums."""
    return 5 * up(4 * m) + up(4 * 512 * ((m + 2047) // 2048)) + up(8 * group * 2 * chunks(m))


def sky_bytes(P):
    m = 4 * max(P, 1)
    return up(16 * m) + sort_bytes(m, 16) + up(64) + 256


def motion_bytes(n):
    m = max(n, 1)
    return up(48 * m) + sort_bytes(m, 16) + up(64) + 256


def sort_passes(n_ids):
    bits = max(int(n_ids) - 1, 1).bit_length()            # ceil(log2 n_ids), at least one bit
    return (bits + 8) // 9


def test_new_symbols_declared_listed_and_exported():
    lib, header = L.load(), open(HEADER).read()
    for name, ret in NEW_SYMBOLS.items():
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert re.search(rf"^{ret}\s+{name}\(", header, re.M), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.emd_abi_version() == 31 and "#define EMD_ABI_VERSION 31" in header          # a compatible extension: it kept the version (31 since EmdDensifyArgs.size_threshold)
    # the header states both formulas in terms of sort(m, g)
    assert "bytes = up(16 m) + sort(m, 16) + up(64) + 256" in header and "bytes = up(48 m) + sort(m, 16) + up(64) + 256" in header
    # no struct grew and no flag bit was added: the modes are entry points of their own
    assert C.sizeof(L.EmdSkyBwdArgs) == C.sizeof(L.EmdSkyArgs) + 5 * C.sizeof(C.c_void_p)


def test_workspace_sizes_are_host_only_monotone_and_the_headers_formula():
    """Runs without a GPU, so the entries are host-only."""
    lib = L.load()
    for P in (0, 1, 255, 512, 513, 2000, 64 * 96, 37 * 53, 1066 * 1600):
        assert lib.emd_sky_det_workspace_size(P) == sky_bytes(P) == L.sky_det_workspace_size(P), P
    for n in (0, 1, 255, 513, 4000, 30011, 2_000_000):
        assert lib.emd_motion_det_workspace_size(n) == motion_bytes(n) == L.motion_det_workspace_size(n), n
    for f in (lib.emd_sky_det_workspace_size, lib.emd_motion_det_workspace_size):
        sizes = [f(n) for n in (1, 2, 100, 30011, 30012, 10 ** 6, 2 * 10 ** 6)]
        assert sizes == sorted(sizes) and sizes[0] < sizes[2] < sizes[3] < sizes[5] < sizes[6]
    # the limits: 4 P, 4 n <= 2^32 - 1 - 2048; beyond them no size is reported
    assert lib.emd_sky_det_workspace_size(SLOT_LIMIT // 4) == sky_bytes(SLOT_LIMIT // 4)
    assert lib.emd_sky_det_workspace_size(SLOT_LIMIT // 4 + 1) == 0 and lib.emd_sky_det_workspace_size(-1) == 0
    assert lib.emd_motion_det_workspace_size(SLOT_LIMIT // 4) == motion_bytes(SLOT_LIMIT // 4)
    assert lib.emd_motion_det_workspace_size(SLOT_LIMIT // 4 + 1) == 0 and lib.emd_motion_det_workspace_size(-1) == 0


def test_offsets_name_the_arrays_and_the_result_pair():
    """rows first, then the raw keys, then keys[0], keys[1], slots[0], slots[1] (the sort's ping-pong), ..., the count words last: the
    offsets report the pair the sorted lists end up in, which alternates with the number of passes (ceil(log2 ids) bits, at most nine a pass)."""
    lib = L.load()
    for P, res in ((64 * 96, 4), (2000, 8), (2000, 64), (1066 * 1600, 1024), (1, 1)):
        m = 4 * P
        lay = L.sky_det_layout(P, res)
        pair = (sort_passes(6 * res * res) - 1) & 1
        assert lay["rows"] == 0 and lay["raw_keys"] == up(16 * m) and lay["bytes"] == sky_bytes(P)
        assert lay["keys"] == lay["raw_keys"] + (1 + pair) * up(4 * m) and lay["slots"] == lay["raw_keys"] + (3 + pair) * up(4 * m)
        assert lay["counts"] == lay["bytes"] - 256 - up(64)
    assert [sort_passes(6 * r * r) for r in (1, 4, 8, 64, 1024)] == [1, 1, 1, 2, 3]
    for n, A in ((4000, 5), (4000, 1), (30011, 600), (1, 1)):
        lay = L.motion_det_layout(n, A)
        pair = (sort_passes(A) - 1) & 1
        assert lay["rows"] == 0 and lay["raw_keys"] == up(48 * n) and lay["bytes"] == motion_bytes(n)
        assert lay["keys"] == lay["raw_keys"] + (1 + pair) * up(4 * n) and lay["slots"] == lay["raw_keys"] + (3 + pair) * up(4 * n)
        assert lay["counts"] == lay["bytes"] - 256 - up(64)
    out = (C.c_size_t * 6)()
    assert lib.emd_sky_det_workspace_offsets(100, 0, out) == L.EMD_ERR_INVALID
    assert lib.emd_sky_det_workspace_offsets(SLOT_LIMIT // 4 + 1, 8, out) == L.EMD_ERR_INVALID
    assert lib.emd_motion_det_workspace_offsets(100, 0, out) == L.EMD_ERR_INVALID


FAKE = 1 << 20             # never dereferenced: the calls are refused first


def _sky_call(H=64, W=96, res=4):
    b = L.EmdSkyBwdArgs()
    b.f.height, b.f.width, b.f.resolution, b.f.flags = H, W, res, L.SKY_CLAMP01
    b.f.cube = b.dL_dsky = b.dL_dcube = FAKE
    b.f.mask_threshold = -1.0
    return b


def test_sky_entry_refuses_a_missing_short_or_misaligned_workspace_on_the_host():
    """Argument checking happens before any HIP call: no GPU needed."""
    lib = L.load()
    b = _sky_call()
    need = L.sky_det_workspace_size(64 * 96)
    assert lib.emd_sky_backward_det(C.byref(b), None, 0, None) == L.EMD_ERR_WORKSPACE and b"det_ws" in lib.emd_last_error()
    assert lib.emd_sky_backward_det(C.byref(b), None, need, None) == L.EMD_ERR_WORKSPACE
    assert lib.emd_sky_backward_det(C.byref(b), FAKE, need - 1, None) == L.EMD_ERR_WORKSPACE
    assert lib.emd_sky_backward_det(C.byref(b), FAKE + 64, 1 << 40, None) == L.EMD_ERR_WORKSPACE and b"aligned" in lib.emd_last_error()
    # the default entry's own checks apply unchanged, and come first
    assert lib.emd_sky_backward_det(None, FAKE, need, None) == L.EMD_ERR_INVALID
    b.dL_dsky = None
    assert lib.emd_sky_backward_det(C.byref(b), FAKE, need, None) == L.EMD_ERR_INVALID and b"no incoming gradient" in lib.emd_last_error()
    b = _sky_call()
    b.f.cube = None
    assert lib.emd_sky_backward_det(C.byref(b), FAKE, need, None) == L.EMD_ERR_INVALID and b"cube" in lib.emd_last_error()
    # the size limit of the mode
    b = _sky_call(H=1 << 15, W=1 << 15)
    assert lib.emd_sky_backward_det(C.byref(b), FAKE, 1 << 50, None) == L.EMD_ERR_INVALID and b"32 bits" in lib.emd_last_error()


def test_motion_entry_refuses_a_missing_short_or_misaligned_workspace_on_the_host():
    lib = L.load()
    n = 4000
    m = L.EmdMotion(FAKE, FAKE, 5, None, None)
    need = L.motion_det_workspace_size(n)
    call = lambda ws, nbytes, motion=m, means=FAKE: lib.emd_motion_backward_det(n, means, None, None, C.byref(motion) if motion else None, FAKE, None,
                                                                                None, FAKE, None, None, FAKE, None, None, ws, nbytes, None)
    assert call(None, 0) == L.EMD_ERR_WORKSPACE and b"det_ws" in lib.emd_last_error()
    assert call(None, need) == L.EMD_ERR_WORKSPACE
    assert call(FAKE, need - 1) == L.EMD_ERR_WORKSPACE
    assert call(FAKE + 64, 1 << 40) == L.EMD_ERR_WORKSPACE and b"aligned" in lib.emd_last_error()
    # the default entry's own checks apply unchanged, and come first
    assert call(FAKE, need, means=None) == L.EMD_ERR_INVALID
    assert call(FAKE, need, motion=None) == L.EMD_ERR_INVALID
    assert call(FAKE, need, motion=L.EmdMotion(FAKE, None, 5, None, None)) == L.EMD_ERR_INVALID and b"actor_pose" in lib.emd_last_error()


def test_python_switches_default_off():
    from emd_amd import motion, nodes
    from emd_amd.sky import EnvLight, SkyCubeMap, _SkyOp
    assert SkyCubeMap.deterministic is False and EnvLight.deterministic is False
    cfg = types.SimpleNamespace(sky_resolution=2, sky_white_background=False, white_background=False)
    assert SkyCubeMap(cfg, device="cpu").deterministic is False and SkyCubeMap(cfg, device="cpu", deterministic=True).deterministic is True
    assert EnvLight(resolution=2, device="cpu").deterministic is False and EnvLight(resolution=2, device="cpu", deterministic=True).deterministic is True
    assert SkyCubeMap.deterministic is False and EnvLight.deterministic is False            # an instance's switch is its own
    for f in (motion.transform_gaussians, nodes.rigid_gaussians, nodes.deformable_gaussians, _SkyOp.forward, motion._MotionTransform.forward):
        assert inspect.signature(f).parameters["deterministic"].default is False, f
