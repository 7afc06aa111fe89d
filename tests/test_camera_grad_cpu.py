"""-m "not gpu": the camera-gradient entry points exist and agree on the ABI; the adapter's camera (gsplat_api._device_camera) is the same
fp32 camera with and without autograd and differentiates as its fp64 restatement does."""
import ctypes as C
import os
import re

import numpy as np
import torch

from emd_amd import _lib as L
from emd_amd import gsplat_api
from tests import camera_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("emd_camera_grad_workspace_size", "emd_raster_backward_camera")


def test_entry_points_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "emd_raster.h")).read(), flags=re.S)
    lib = L.load()
    for n in NEW:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n)


def test_abi_31_in_header_binding_and_library():
    v = int(re.search(r"#define EMD_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "emd_raster.h")).read()).group(1))
    assert v == L.ABI_VERSION == L.load().emd_abi_version() == 31


def test_workspace_size_is_monotone_and_never_empty():
    sizes = [L.camera_grad_workspace_size(n) for n in (1, 255, 256, 257, 600, 100_000, 2_000_000)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[2] < sizes[3] and sizes[-1] == ((2_000_000 + 255) // 256) * 36 * 4        # one 36-float row per 256 Gaussians
    assert L.camera_grad_workspace_size(0) > 0
    out = C.c_size_t()
    assert L.load().emd_camera_grad_workspace_size(-1, C.byref(out)) == L.EMD_ERR_INVALID
    assert L.load().emd_camera_grad_workspace_size(5, None) == L.EMD_ERR_INVALID


def test_null_arguments_are_reported_before_any_launch():
    lib = L.load()
    assert lib.emd_raster_backward_camera(None, None, None, 0, None) == L.EMD_ERR_INVALID
    b = L.EmdBwdArgs()
    b.s.image_height = b.s.image_width = 16
    b.s.tanfovx = b.s.tanfovy = 1.0
    assert lib.emd_raster_backward_camera(C.byref(b), None, None, 0, None) == L.EMD_ERR_INVALID
    assert b"null" in lib.emd_last_error()


def _camera(seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(4, generator=g), dim=0)
    w, x, y, z = q.tolist()
    Rm = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                       [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    vm = torch.eye(4)
    vm[:3, :3], vm[:3, 3] = Rm, torch.randn(3, generator=g) * 3
    K = torch.tensor([[118.0, 0, 48 / 2 + 3.5], [0, 112.0, 32 / 2 - 2.25], [0, 0, 1]])
    return vm, K


def test_device_camera_forward_values_do_not_depend_on_autograd():
    vm, K = _camera()
    plain = gsplat_api._device_camera(vm.clone(), K, 48, 32)
    attached = gsplat_api._device_camera(vm.clone().requires_grad_(True), K, 48, 32)
    assert all(a.requires_grad for a in attached[:3]) and not attached[3].requires_grad
    for a, b in zip(plain, attached):
        assert torch.equal(a, b.detach())
    # and a second attached call is not disturbed by the first (the cached constants are never written)
    again = gsplat_api._device_camera(vm.clone().requires_grad_(True), K, 48, 32)
    for a, b in zip(plain, again):
        assert torch.equal(a, b.detach())


def test_device_camera_jacobian_matches_the_fp64_restatement():
    vm, K = _camera(1)
    f32 = lambda v: torch.cat([x.reshape(-1) for x in gsplat_api._device_camera(v, K, 48, 32)[:3]])
    f64 = lambda v: torch.cat([x.reshape(-1) for x in R.device_camera_ref(v, K, 48, 32)])
    got = torch.autograd.functional.jacobian(f32, vm).reshape(35, 16).double().numpy()
    want = torch.autograd.functional.jacobian(f64, vm.double()).reshape(35, 16).numpy()
    assert np.abs(f32(vm).detach().double().numpy() - f64(vm.double()).numpy()).max() <= 1e-5
    # every entry is a sum of at most three products of two fp32 numbers: a few ulps of the largest entry
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    assert (want != 0).sum() >= 16 + 24 + 18
