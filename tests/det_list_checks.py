"""What a deterministic entry point leaves in its caller-owned workspace, read back and checked (emd_sky_backward_det, emd_motion_backward_det;
DESIGN.md section 8.10): the structure of the sorted lists and the output against the pinned sum of tests/segsum_checks.py, bit for bit.
Not a test: tests/test_sky_det_gpu.py and tests/test_motion_det_gpu.py call it."""
import numpy as np

from tests import segsum_checks as sg

DROPPED = 0xFFFFFFFF


def read_workspace(ws, lay, n_slots, row_pitch):
    """ws: the uint8 workspace tensor after the call, lay: the dict of _lib.sky_det_layout / motion_det_layout
    -> (rows [n_slots, row_pitch] float32, raw_keys [n_slots] uint32, keys [count], slots [count], count)."""
    raw = ws.cpu().numpy()
    view = lambda off, n, dt: raw[off:off + 4 * n].view(dt)
    count = int(view(lay["counts"], 1, np.uint32)[0])
    assert 0 <= count <= n_slots
    rows = view(lay["rows"], n_slots * row_pitch, np.float32).reshape(n_slots, row_pitch)
    return rows, view(lay["raw_keys"], n_slots, np.uint32), view(lay["keys"], n_slots, np.uint32)[:count], view(lay["slots"], n_slots, np.uint32)[:count], count


def check_lists(ws, lay, n_slots, row_pitch, width, out, n_ids):
    """out: [n_ids, >= width] float32 array the call wrote (zeroed by the call, then the sums).  -> (run lengths, raw_keys, keys, slots)"""
    rows, raw_keys, keys, slots, count = read_workspace(ws, lay, n_slots, row_pitch)
    keys64, slots64 = keys.astype(np.int64), slots.astype(np.int64)
    assert (np.diff(keys64) >= 0).all()                                          # the sorted keys are non-decreasing
    assert (np.diff(slots64)[np.diff(keys64) == 0] > 0).all()                    # slots ascending inside a run
    kept = np.flatnonzero(raw_keys != DROPPED)
    assert np.array_equal(np.sort(slots64), kept)                                # the kept slots are exactly those with a destination
    assert np.array_equal(raw_keys[slots64], keys) and (keys64 < n_ids).all()
    want = np.zeros((n_ids, out.shape[1]), np.float32)                           # destinations without a run: +0.0
    sg.segsum_reference(keys64, slots64, rows, width, want)
    assert np.array_equal(np.ascontiguousarray(out).view(np.uint32), want.view(np.uint32))
    untouched = np.ones(n_ids, bool)
    untouched[keys64] = False
    assert (np.ascontiguousarray(out[untouched]).view(np.uint32) == 0).all()     # +0.0, not -0.0
    return sg.run_structure(keys64)[1], raw_keys, keys64, slots64
