"""-m gpu: the HIP sky cube-map path (through the C ABI, emd_amd/sky.py) against the CPU oracle and the golden vectors
captured from the reference's SkyCubeMap / EnvLight.  Floating point: colours within 2e-5 of the oracle (fp32: the bilinear
weights are fractions of u * res, so their rounding error grows with res -- ~res * 2^-23; the face / tap decisions are
identical), texture gradients within 1e-4 of the largest entry (float atomics reorder the sums).  The camera-ray path (rays built in the
kernel, 2-D backward tiles) is compared element by element with the float64 oracle further down, on the cases and bars of tests/sky_cases.py."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import sky_oracle as so

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
TOL = 2e-5


def _cam(g, dev):
    return types.SimpleNamespace(image_height=int(g["H"]), image_width=int(g["W"]), intrinsic=torch.from_numpy(g["K"]).to(dev),
                                 world_view_transform=torch.from_numpy(g["world_view_transform"]).to(dev))


def test_skycubemap_matches_reference_golden():
    from emd_amd.sky import SkyCubeMap, composite_s3g
    dev = torch.device("cuda", 0)
    g = np.load(os.path.join(G, "s3g_sky.npz"))
    cam = _cam(g, dev)
    for tag, white in (("white", True), ("black", False)):
        cfg = types.SimpleNamespace(sky_resolution=16, sky_white_background=white, white_background=False)
        m = SkyCubeMap(cfg, device=dev)
        m.sky_cube_map.data = torch.from_numpy(g[f"{tag}_cube"]).to(dev)
        acc = torch.from_numpy(g[f"{tag}_acc"]).to(dev)
        np.testing.assert_allclose(m(cam).detach().cpu().numpy(), g[f"{tag}_sky_all"], atol=1e-5)
        np.testing.assert_allclose(m(cam, acc=acc).detach().cpu().numpy(), g[f"{tag}_sky_masked"], atol=1e-5)
        out, sky = composite_s3g(m, cam, torch.from_numpy(g[f"{tag}_render"]).to(dev), acc)
        np.testing.assert_allclose(out.detach().cpu().numpy(), g[f"{tag}_blended"], atol=1e-5)
        np.testing.assert_allclose(sky.detach().cpu().numpy(), g[f"{tag}_sky_masked"], atol=1e-5)


def test_envlight_matches_reference_golden():
    from emd_amd.sky import EnvLight, composite_add
    dev = torch.device("cuda", 0)
    g = np.load(os.path.join(G, "or_envlight.npz"))
    env = EnvLight(resolution=8, device=dev)
    env.base.data = torch.from_numpy(g["base"]).to(dev)
    infos = {"viewdirs": torch.from_numpy(g["viewdirs"]).to(dev)}
    np.testing.assert_allclose(env(infos).detach().cpu().numpy(), g["light"], atol=1e-6)
    rgb, sky = composite_add(env, infos, torch.from_numpy(g["rgb"]).to(dev), torch.from_numpy(g["opacity"]).to(dev))
    np.testing.assert_allclose(rgb.detach().cpu().numpy(), g["blended"], atol=1e-6)


@pytest.mark.parametrize("res,P,seed", [(8, 20000, 0), (64, 200000, 1), (33, 50000, 2)])
def test_lookup_forward_backward_vs_oracle(res, P, seed):
    from emd_amd.sky import EnvLight, composite_add
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand(6, res, res, 3, generator=gen)
    dirs = torch.randn(P, 3, generator=gen)
    dirs[:64] = torch.tensor([1.0, 1.0, 1.0]) * torch.sign(torch.randn(64, 3, generator=gen))        # cube corners
    dirs[64:256, 0] = dirs[64:256, 1].abs()                                                           # on an edge
    rgb, op = torch.rand(P, 3, generator=gen), torch.rand(P, 1, generator=gen)
    g_out, g_sky = torch.randn(P, 3, generator=gen), torch.randn(P, 3, generator=gen)
    # oracle (torch autograd on CPU); EnvLight rotates to OpenGL axes first, undo that so both see `dirs`
    b0 = base.clone().requires_grad_(True); r0 = rgb.clone().requires_grad_(True); o0 = op.clone().requires_grad_(True)
    sky0 = so.cube_lookup(b0, dirs)
    out0 = so.blend_add(r0, o0, sky0)
    ((out0 * g_out).sum() + (sky0 * g_sky).sum()).backward()
    env = EnvLight(resolution=res, device=dev)
    env.base.data = base.to(dev)
    r1 = rgb.to(dev).requires_grad_(True); o1 = op.to(dev).requires_grad_(True)
    infos = {"viewdirs": (dirs @ env.to_opengl.cpu()).to(dev)}          # (d M) M^T = d for the orthonormal axis swap
    out1, sky1 = composite_add(env, infos, r1, o1)
    ((out1 * g_out.to(dev)).sum() + (sky1 * g_sky.to(dev)).sum()).backward()
    np.testing.assert_allclose(sky1.detach().cpu().numpy(), sky0.detach().numpy(), atol=TOL)
    np.testing.assert_allclose(out1.detach().cpu().numpy(), out0.detach().numpy(), atol=2 * TOL)
    gb0, gb1 = b0.grad.numpy(), env.base.grad.cpu().numpy()
    assert np.abs(gb1 - gb0).max() <= 1e-4 * np.abs(gb0).max(), np.abs(gb1 - gb0).max()
    np.testing.assert_allclose(r1.grad.cpu().numpy(), r0.grad.numpy(), atol=1e-6)
    np.testing.assert_allclose(o1.grad.cpu().numpy(), o0.grad.numpy(), atol=1e-4)   # -sum_c g_c sky_c with |g| up to ~4


def test_full_size_properties():
    """1066 x 1600 view, 1024^2 faces (the reference's sizes): colours stay inside the texture's range, a constant map
    gives a constant image, and the texture gradient conserves mass (bilinear weights sum to one)."""
    from emd_amd.sky import SkyCubeMap, composite_s3g
    dev = torch.device("cuda", 0)
    H, W = 1066, 1600
    K = torch.tensor([[1700.0, 0, 800.0], [0, 1700.0, 533.0], [0, 0, 1]], device=dev)
    yaw = 0.3
    R = torch.tensor([[np.sin(yaw), -np.cos(yaw), 0], [0, 0, -1], [np.cos(yaw), np.sin(yaw), 0]], dtype=torch.float32)
    wvt = torch.eye(4); wvt[:3, :3] = R.T; wvt[3, :3] = torch.tensor([0.3, -1.5, 0.2])
    cam = types.SimpleNamespace(image_height=H, image_width=W, intrinsic=K, world_view_transform=wvt.to(dev))
    cfg = types.SimpleNamespace(sky_resolution=1024, sky_white_background=False, white_background=False)
    m = SkyCubeMap(cfg, device=dev)
    m.sky_cube_map.data.fill_(0.25)
    assert torch.all((m(cam) - 0.25).abs() < 1e-6)
    gen = torch.Generator().manual_seed(5)
    m.sky_cube_map.data = (torch.rand(6, 1024, 1024, 3, generator=gen) * 0.8 + 0.1).to(dev)
    acc = torch.rand(1, H, W, generator=gen).to(dev).requires_grad_(True)
    render = torch.rand(3, H, W, generator=gen).to(dev).requires_grad_(True)
    out, sky = composite_s3g(m, cam, render, acc)
    sampled = (1 - acc.detach()[0]) > 1e-3                      # fully covered pixels are not looked up (fill colour)
    assert sky[:, sampled].min() >= 0.1 - 1e-6 and sky[:, sampled].max() <= 0.9 + 1e-6 and torch.all(sky[:, ~sampled] == 0)
    torch.testing.assert_close(out, render * acc + sky.detach() * (1 - acc), atol=1e-6, rtol=0)
    out.sum().backward()
    # d(sum out)/d texel summed over texels = sum over pixels of (1 - acc) * 3 channels... per channel: sum (1 - acc)
    expect = ((1 - acc.detach()[0]) * sampled).sum().item()
    got = m.sky_cube_map.grad.sum(dim=(0, 1, 2)).cpu().numpy()
    np.testing.assert_allclose(got, expect, rtol=2e-4)
    torch.testing.assert_close(render.grad, acc.detach().expand(3, H, W), atol=1e-6, rtol=0)


# ---- the camera-ray path (SkyCubeMap / composite_s3g: rays built in the kernel, 16 x 16 backward tiles with the LDS window) element by element
# ---- against the float64 oracle.  Cases, reference and bars: tests/sky_cases.py; the bars are 4 x what float32 costs the oracle itself, measured
# ---- by tests/test_sky_cpu.py, never taken from the kernel.
from tests import sky_cases as sc  # noqa: E402


def _camera(c, dev, **extra):
    return types.SimpleNamespace(image_height=c.H, image_width=c.W, intrinsic=c.K.to(dev), world_view_transform=c.w2c.T.contiguous().to(dev), **extra)


def _run(c, cam, through_forward=False):
    """One forward + backward of case `c` on the HIP path -> dict of sky_cases.QUANTITIES on the CPU.  through_forward: SkyCubeMap.forward and the
    blend in torch instead of composite_s3g (what composite_s3g itself does for a camera with a sky_mask)."""
    from emd_amd.sky import SkyCubeMap, composite_s3g
    dev = torch.device("cuda", 0)
    cfg = types.SimpleNamespace(sky_resolution=c.res, sky_white_background=c.white, white_background=False)
    m = SkyCubeMap(cfg, device=dev)
    m.sky_cube_map.data = c.cube.to(dev)
    render, weight = c.render.to(dev).requires_grad_(True), c.acc.to(dev).requires_grad_(True)
    train = c.jitter is not None
    jitter = c.jitter.to(dev) if train else None
    if not c.blend:
        out, sky = None, m(cam, acc=weight)
    elif through_forward:
        sky = m(cam, acc=weight, is_train=train, jitter=jitter)
        out = render * weight + sky * (1 - weight)
    else:
        out, sky = composite_s3g(m, cam, render, weight, is_train=train, jitter=jitter)
    sc.loss(out, sky, c.g_out.to(dev), c.g_sky.to(dev)).backward()
    r = {"sky": sky.detach().cpu(), "d_cube": m.sky_cube_map.grad.cpu()}
    if c.blend:
        r.update(out=out.detach().cpu(), d_render=render.grad.cpu(), d_weight=weight.grad.cpu())
    return r


def _check(got, c, only=None):
    ref = sc.reference(c.id, c.white)
    assert set(got) == set(ref)
    assert torch.equal(got["sky"][:, ~c.sampled], torch.full_like(got["sky"][:, ~c.sampled], c.fill))     # not looked up: the fill, exactly
    assert torch.isfinite(got["d_cube"]).all()
    bad = []
    for q in only or ref:
        assert got[q].shape == ref[q].shape
        diff, limit = sc.max_diff(got[q], ref[q], c, q), sc.bar(c.id, q)
        print(f"{c.id} white={c.white} {q}: max |hip - float64| {diff:.3e}  bar {limit:.3e}  largest reference entry {float(ref[q].abs().max()):.3e}")
        if not diff <= limit:
            bad.append((q, diff, limit))
    assert not bad, bad


@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("case_id", list(sc.CASES))
def test_camera_rays_forward_backward_vs_oracle(case_id, white):
    """composite_s3g on every case of sky_cases.CASES: sky, out, dL/dcube at every texel, dL/drender, dL/dweight."""
    c = sc.build(case_id, white)
    _check(_run(c, _camera(c, torch.device("cuda", 0))), c)


@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("through_forward", [False, True])
def test_jitter_vs_oracle(through_forward, white):
    """A given sub-pixel draw under is_train, through composite_s3g and through SkyCubeMap.forward, against the reference with the same draw."""
    c = sc.build("jitter", white)
    _check(_run(c, _camera(c, torch.device("cuda", 0)), through_forward), c)


@pytest.mark.parametrize("white", [True, False])
def test_sky_mask_route_vs_oracle(white):
    """is_train with camera.sky_mask: rows < 50 forced on, threshold 0.5, the fill elsewhere, two launches and the blend in torch."""
    c = sc.build("sky-mask", white)
    dev = torch.device("cuda", 0)
    _check(_run(c, _camera(c, dev, sky_mask=c.sky_mask.to(dev))), c)


@pytest.mark.parametrize("white", [True, False])
def test_forward_without_blend_vs_oracle(white):
    """SkyCubeMap.forward(cam, acc=acc): dL/dcube from the sky colour's gradient alone."""
    c = sc.build("no-blend", white)
    _check(_run(c, _camera(c, torch.device("cuda", 0))), c)


@pytest.mark.parametrize("white", [True, False])
def test_device_camera_matches_host_camera(white):
    """camera.sky_rays (the 21 floats on the device) against the host-camera call: the same arithmetic, so everything but dL/dcube is
    bit-identical; dL/dcube (float atomics reorder) is held to the oracle's bar."""
    from emd_amd.sky import sky_ray_constants
    c = sc.build("corner-64", white)
    dev = torch.device("cuda", 0)
    host_cam = _camera(c, dev)
    host = _run(c, host_cam)
    rays = sky_ray_constants(host_cam.intrinsic, host_cam.world_view_transform).to(dev)
    assert rays.shape == (21,)
    got = _run(c, types.SimpleNamespace(image_height=c.H, image_width=c.W, sky_rays=rays))
    for q in ("sky", "out", "d_render", "d_weight"):
        assert torch.equal(got[q], host[q]), q
    _check(got, c, only=["d_cube"])
