"""-m "not gpu": the pitch of the render backward's accumulator rows.  A row is its 12 payload floats + 4 per extra colour set, rounded up to
whole 64-byte lines (16, 16, 32 floats for 0, 1, 2 extra sets); the workspace is N x pitch floats and starts on a 64-byte line.  The size and
alignment checks of emd_raster_backward / emd_raster_backward_camera sit ahead of every device call, so they are exercised here with
pointers that are never dereferenced."""
import ctypes as C

import pytest

from emd_amd import _lib as L

H = W = 32
CAP = 100
FAKE = 0x7F0000000000        # 64-byte aligned, never dereferenced: every call below is refused by the host-side validation


@pytest.mark.parametrize("num_extra, pitch", [(0, 16), (1, 16), (2, 32)])
def test_pitch_is_the_payload_rounded_up_to_whole_lines(num_extra, pitch):
    assert L.BWD_PAYLOAD == 12
    assert L.bwd_stride(num_extra) == pitch
    assert pitch >= L.BWD_PAYLOAD + 4 * num_extra and pitch % 16 == 0
    assert L.BWD_STRIDE == L.bwd_stride(0)


@pytest.mark.parametrize("num_extra", [0, 1, 2])
@pytest.mark.parametrize("N", [0, 1, 5, 2_000_000])
def test_workspace_size_is_rows_times_pitch(N, num_extra):
    w = L.workspace_sizes(N, 1066, 1600, 8_000_000, num_extra=num_extra)[3]
    assert w == max(N, 1) * L.bwd_stride(num_extra) * 4       # (N = 0: one row, as the other workspaces keep one element)
    assert w % 64 == 0


def _bwd_args(N, num_extra, bwd_ws, bwd_bytes):
    gb, bb, ib, _ = L.workspace_sizes(N, H, W, CAP, num_extra=num_extra)
    b = L.EmdBwdArgs()
    b.s.image_height, b.s.image_width, b.s.tanfovx, b.s.tanfovy = H, W, 1.0, 1.0
    b.num_gaussians, b.bin_capacity, b.num_extra = N, CAP, num_extra
    b.means3D = b.opacities = b.colors_precomp = b.scales = b.rotations = FAKE
    b.radii = b.geom_ws = b.bin_ws = b.img_ws = b.status = b.out_color = b.out_depth = FAKE
    b.geom_bytes, b.bin_bytes, b.img_bytes = gb, bb, ib
    b.bwd_ws, b.bwd_bytes = bwd_ws, bwd_bytes
    return b


def _calls(b):
    lib = L.load()
    yield "backward", lambda: lib.emd_raster_backward(C.byref(b), None)
    yield "backward_camera", lambda: lib.emd_raster_backward_camera(C.byref(b), FAKE, FAKE, L.camera_grad_workspace_size(b.num_gaussians), None)


@pytest.mark.parametrize("num_extra", [0, 2])
def test_short_workspace_is_refused_before_any_launch(num_extra):
    N = 5
    need = N * L.bwd_stride(num_extra) * 4
    # one byte short, and the size the 48-byte pitch would have asked for
    for have in (need - 1, N * (L.BWD_PAYLOAD + 4 * num_extra) * 4):
        b = _bwd_args(N, num_extra, FAKE, have)
        for what, call in _calls(b):
            assert call() == L.EMD_ERR_WORKSPACE, (what, have)
            assert b"workspace too small" in L.load().emd_last_error(), what


@pytest.mark.parametrize("offset", [4, 16, 32, 48])
def test_misaligned_workspace_is_refused_before_any_launch(offset):
    N = 5
    b = _bwd_args(N, 0, FAKE + offset, N * L.bwd_stride(0) * 4)
    for what, call in _calls(b):
        assert call() == L.EMD_ERR_INVALID, what
        assert b"bwd_ws must be 64-byte aligned" in L.load().emd_last_error(), what
