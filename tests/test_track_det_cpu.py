"""No device needed: the interface of the deterministic actor chain (csrc/track_det.hip) -- exported symbols, the
workspace layout, every refusal that is decided before a launch, and the Python switches.  The entry points are a compatible extension: no struct
changed, so the ABI version is the header's and the binding's (the tests that pin its value stay as they are)."""
import ctypes as C
import inspect
import os
import re

import pytest

from emd_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("emd_track_det_workspace_size", "emd_track_det_workspace_offsets", "emd_actor_row_sum_det", "emd_track_heads_forward_det",
       "emd_track_heads_backward_det", "emd_tracked_pose_backward_det")
# a non-null, 256-aligned address that is never dereferenced: every call below is refused, or returns, before anything is launched
FAKE = 0x10000


def test_symbols_and_abi():
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "emd_raster.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS and re.search(r"\b%s\(" % name, header), name
    v = int(re.search(r"#define EMD_ABI_VERSION (\d+)", header).group(1))
    assert lib.emd_abi_version() == v == L.ABI_VERSION


def test_the_unit_is_built_by_the_makefile():
    mk = open(os.path.join(ROOT, "emd_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS = .*\btrack_det\.o\b", mk, re.M)
    for header in ("temporal_sample.h", "quat_math.h", "det_reduce.h"):
        assert re.search(r"^[^#\n]*\btrack_det\.o\b[^\n]*: [^\n]*%s" % re.escape(header), mk, re.M), header
    csrc = os.path.join(ROOT, "emd_amd", "csrc")
    code = lambda name: re.sub(r"//[^\n]*", "", open(os.path.join(csrc, name)).read())
    assert "atomic" not in code("track_det.hip")                 # no atomics anywhere in the unit's code
    # ... nor in the source text the units without atomics share with the default kernels: every project file they include, directly or through
    # another, that holds such shared text is read the same way
    shared = {"track_det.hip": ("track_heads.h", "temporal_sample.h", "te_gather_body.inc"), "sky_det.hip": ("sky_pixel_bwd_body.inc",),
              "embed_det.hip": ("temporal_sample.h", "te_gather_body.inc")}

    def included(name, seen):
        for inc in re.findall(r'^\s*#include "([^"]+)"', open(os.path.join(csrc, name)).read(), re.M):
            if inc not in seen and os.path.exists(os.path.join(csrc, inc)):
                seen.add(inc)
                included(inc, seen)
        return seen

    for unit, files in shared.items():
        incs = included(unit, set())
        for f in files:
            assert f in incs, (unit, f)
            assert "atomic" not in code(f), f
    # a file named *_body.inc or track_heads.h that one of these units includes is in the list above: a new one is not missed
    for unit in shared:
        for f in included(unit, set()):
            if f.endswith(".inc") or f == "track_heads.h":
                assert f in shared[unit], (unit, f)
    # the objects are rebuilt when the shared text changes
    for objs, dep in ((("embed.o", "track_det.o"), "track_heads.h"), (("sky.o", "sky_det.o"), "sky_pixel_bwd_body.inc"),
                      (("standalone_ops.o",), "motion_point_bwd_body.inc"), (("embed_det.o", "track_det.o"), "te_gather_body.inc"),
                      (("plane_reg.o", "vanilla.o", "trainer_loss.o"), "fixed_sum.h")):
        for obj in objs:
            assert re.search(r"^[^#\n]*\b%s\b[^\n]*: [^\n]*\b%s\b" % (re.escape(obj), re.escape(dep)), mk, re.M), (obj, dep)
        users = [u for u in os.listdir(csrc) if u.endswith(".hip") and re.search(r'#include "%s"' % re.escape(dep), open(os.path.join(csrc, u)).read())]
        assert sorted(u[:-4] + ".o" for u in users) == sorted(objs), (dep, users)


@pytest.mark.parametrize("A,w,n,g", [(1, 0, 1, 1), (32, 36, 0, 0), (32, 0, 160000, 10), (4, 64, 9221, 8), (5, 0, 4000, 64), (33, 3, 99, 40)])
def test_workspace_offsets_are_monotone_and_aligned(A, w, n, g):
    total = L.track_det_workspace_size(A, w, n, g)
    lay = L.track_det_layout(A, w, n, g)
    assert lay["bytes"] == total and total % 256 == 0
    offs = [lay["slab"], lay["dh"]] + ([lay["raw_keys"]] if g and n else []) + [lay["counts"], total]
    assert all(o % 256 == 0 for o in offs) and all(b >= a for a, b in zip(offs, offs[1:]))
    if w:
        assert lay["pitch"] >= 8 * w + 8 and lay["pitch"] % 16 == 0
        assert lay["dh"] - lay["slab"] >= 4 * A * lay["pitch"]
        assert (lay["raw_keys"] if g and n else lay["counts"]) - lay["dh"] >= 4 * A * 2 * 64
    if g and n:
        assert lay["raw_keys"] < min(lay["keys"], lay["slots"]) and max(lay["keys"], lay["slots"]) + 4 * n <= lay["counts"]
        assert lay["keys"] % 256 == 0 and lay["slots"] % 256 == 0
    # more of anything never needs less
    assert L.track_det_workspace_size(A + 1, w, n, g) >= total and L.track_det_workspace_size(A, w, n + 1000, g) >= total


def test_workspace_size_refuses_sizes_outside_the_limits():
    lib = L.load()
    assert lib.emd_track_det_workspace_size(4, 65, 0, 0) == 0
    assert lib.emd_track_det_workspace_size(4, 0, 10, 65) == 0
    assert lib.emd_track_det_workspace_size(-1, 0, 10, 4) == 0
    assert lib.emd_track_det_workspace_size(4, 0, 2 ** 31, 4) == 0
    # the points are numbered in an int, less one sort tile (2048 keys) that the sort rounds its launch up by
    last = 0x7FFFFFFF - 2048
    assert lib.emd_track_det_workspace_size(4, 0, last, 4) > 0 and lib.emd_track_det_workspace_size(4, 0, last + 1, 4) == 0
    out = (C.c_size_t * 8)()
    assert lib.emd_track_det_workspace_offsets(4, 65, 0, 0, out) == -1       # EMD_ERR_INVALID


def _row_sum(n, width, pitch, A, ws, ws_bytes, out_pitch=None, rows=FAKE, ids=FAKE, out=FAKE):
    return L.load().emd_actor_row_sum_det(n, width, rows, pitch, ids, A, None, out, width if out_pitch is None else out_pitch, ws, ws_bytes, None)


def test_row_sum_refusals_come_before_any_launch():
    need = L.track_det_workspace_size(3, 0, 100, 10)
    assert _row_sum(100, 10, 12, 3, None, 0) == -4                         # EMD_ERR_WORKSPACE: null
    assert _row_sum(100, 10, 12, 3, FAKE, need - 1) == -4                  # short
    assert _row_sum(100, 10, 12, 3, FAKE + 128, need + 256) == -4          # misaligned
    assert b"emd_track_det_workspace_size" in L.load().emd_last_error()
    assert _row_sum(100, 65, 70, 3, FAKE, 1 << 30) == -1                   # EMD_ERR_INVALID: width > 64
    assert _row_sum(100, 10, 9, 3, FAKE, 1 << 30) == -1                    # row_pitch < width
    assert _row_sum(100, 0, 4, 3, FAKE, 1 << 30) == -1
    assert _row_sum(100, 10, 12, 3, FAKE, 1 << 30, rows=None) == -1        # null rows
    assert _row_sum(0, 10, 12, 3, None, 0) == 0                            # no points: nothing launched, no workspace
    assert _row_sum(100, 10, 12, 0, None, 0) == 0                          # no actors


def _track_args(A=2, rows=40, dim=32, E=4, n=10, seg=True):
    a = L.EmdTrackArgs()
    a.num_actors, a.rows, a.dim, a.embed_dim, a.k_coarse, a.k_fine, a.num_points = A, rows, dim, E, 30, 30, n
    a.weight = a.embeddings = a.point_ids = a.count = a.emb_sum = FAKE
    a.segment_start = FAKE if seg else None
    for h in range(4):
        a.head_w[h] = a.head_b[h] = FAKE
    return a


def _track_grads(cls):
    g = cls()
    for name, _ in cls._fields_:
        if name in ("d_head_w", "d_head_b"):
            for h in range(4):
                getattr(g, name)[h] = FAKE
        else:
            setattr(g, name, FAKE)
    return g


def test_chain_backward_refusals_come_before_any_launch():
    lib = L.load()
    a, g = _track_args(), _track_grads(L.EmdTrackGrads)
    need = L.track_det_workspace_size(2, 36)
    for ws, nbytes in ((None, 0), (FAKE, need - 1), (FAKE + 64, need + 256)):
        assert lib.emd_track_heads_backward_det(C.byref(a), C.byref(g), ws, nbytes, None) == -4
    p = L.EmdTrackedPoseArgs()
    p.track, p.q_all, p.t_all, p.num_frames, p.frame = a, FAKE, FAKE, 3, 1
    gp = _track_grads(L.EmdTrackedPoseGrads)
    for ws, nbytes in ((None, 0), (FAKE, need - 1), (FAKE + 64, need + 256)):
        assert lib.emd_tracked_pose_backward_det(C.byref(p), C.byref(gp), ws, nbytes, None) == -4
    # the default entries' refusals apply
    p.frame = 3
    assert lib.emd_tracked_pose_backward_det(C.byref(p), C.byref(gp), FAKE, need, None) == -1
    p.frame, p.track.segment_start = 1, None
    assert lib.emd_tracked_pose_backward_det(C.byref(p), C.byref(gp), FAKE, need, None) == -1
    wide = _track_args(dim=60, E=5)
    assert lib.emd_track_heads_backward_det(C.byref(wide), C.byref(g), FAKE, 1 << 30, None) == -1
    g.d_mean = None
    assert lib.emd_track_heads_backward_det(C.byref(a), C.byref(g), FAKE, need, None) == -1
    # no actors: nothing launched, no workspace
    none = _track_args(A=0)
    assert lib.emd_track_heads_backward_det(C.byref(none), C.byref(g), None, 0, None) == 0
    p.track = none
    assert lib.emd_tracked_pose_backward_det(C.byref(p), C.byref(gp), None, 0, None) == 0
    assert lib.emd_track_heads_forward_det(C.byref(none), None, 0, None) == 0


def test_forward_of_unsorted_ids_needs_the_workspace():
    lib = L.load()
    a = _track_args(seg=False)
    a.trans = a.rot = FAKE
    need = L.track_det_workspace_size(2, 0, 10, 4)
    assert lib.emd_track_heads_forward_det(C.byref(a), None, 0, None) == -4
    assert lib.emd_track_heads_forward_det(C.byref(a), FAKE, need - 1, None) == -4
    a.trans = None
    assert lib.emd_track_heads_forward_det(C.byref(a), FAKE, need, None) == -1


def test_python_switches():
    from emd_amd import deformation, motion, nodes
    assert motion.TrackOffsetHeads.deterministic is False
    assert motion.TrackOffsetHeads(3).deterministic is False
    heads = motion.TrackOffsetHeads(3, deterministic=True)
    assert heads.deterministic is True and motion.TrackOffsetHeads.deterministic is False
    heads.deterministic = False
    assert heads.deterministic is False
    assert inspect.signature(deformation.nonrigid_deformation).parameters["deterministic"].default is False
    assert inspect.signature(deformation._DeformInput.forward).parameters["deterministic"].default is False
    assert inspect.signature(motion._TrackHeads.forward).parameters["deterministic"].default is False
    assert inspect.signature(motion._TrackedPose.forward).parameters["deterministic"].default is False
    assert list(inspect.signature(motion._TrackedPose.forward).parameters)[-1] == "deterministic"      # a trailing non-tensor argument
    assert re.search(r"= nonrigid_deformation\([^\n]*deterministic=deterministic\)", inspect.getsource(nodes.deformable_gaussians))
