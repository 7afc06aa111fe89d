"""-m gpu: one S3Gaussian-style step with every deterministic switch it has -- the rasterizer's (RasterOptions.deterministic)
and the sky cube map's (SkyCubeMap.deterministic, section 8.10) -- at the small size of tests/test_full_step_gpu.py: rasterizer with fused actor motion
-> sky composite -> image-loss tail -> backward.  Every gradient of the step has identical bits from run to run and in a hipGraph replay.  With the
sky switch off the step still composes as tests/test_full_step_gpu.py checks it; nothing here asserts that the default mode DIFFERS between runs (a
test must not depend on a race showing up)."""
import types

import numpy as np
import pytest
import torch

from oracle import loss_oracle as lo
from oracle import sky_oracle as so

pytestmark = pytest.mark.gpu
NAMES = ("_xyz", "_scaling", "_rotation", "_opacity", "_features", "instances_quats", "instances_trans")


def _setup(dev, sky_deterministic):
    from emd_amd import RasterOptions, scenes
    from emd_amd.loss import image_loss
    from emd_amd.model import StreetGaussians, render
    from emd_amd.sky import SkyCubeMap, composite_s3g
    N, H, W = 30000, 96, 160
    scene = scenes.add_actors(scenes.make_static_scene(N, seed=0), num_actors=3, pts_per_actor=2000, num_frames=5, seed=1)
    model = StreetGaussians(scene, dev)
    cam = scenes.rig_camera(2, 0, H, W)
    K = torch.tensor([[W / (2 * cam.tanfovx), 0, W / 2], [0, H / (2 * cam.tanfovy), H / 2], [0, 0, 1]], dtype=torch.float32)
    skycam = types.SimpleNamespace(image_height=H, image_width=W, intrinsic=K.to(dev), world_view_transform=cam.world_view_transform.to(dev))
    sky = SkyCubeMap(types.SimpleNamespace(sky_resolution=16, sky_white_background=False, white_background=False), device=dev,
                     deterministic=sky_deterministic)
    g = torch.Generator().manual_seed(9)
    sky.sky_cube_map.data = torch.rand(6, 16, 16, 3, generator=g).to(dev)
    gt = torch.rand(3, H, W, generator=g).to(dev)
    gt_depth = (torch.rand(1, H, W, generator=g) * 60).to(dev)
    sky_mask = (torch.rand(1, H, W, generator=g) < 0.3).to(dev)
    not_sky = ~sky_mask
    opts = RasterOptions(deterministic=True, no_sync=True, capacity_hint=1 << 20)
    leaves = [getattr(model, n) for n in NAMES] + [sky.sky_cube_map]
    bg = torch.zeros(3)

    def step():
        out = render(model, cam, bg, frame=2, options=opts)
        image, sky_color = composite_s3g(sky, skycam, out["render"], out["weight"])
        loss, _ = image_loss(image, gt, out["depth"], gt_depth, not_sky, out["weight"], sky_mask)
        return list(torch.autograd.grad(loss, leaves)), dict(out=out, sky_color=sky_color, loss=loss)
    return types.SimpleNamespace(step=step, cam=cam, K=K, sky=sky, gt=gt, gt_depth=gt_depth, sky_mask=sky_mask, H=H, W=W)


def test_deterministic_step_has_identical_bits_across_runs_and_in_a_graph_replay():
    dev = torch.device("cuda", 0)
    s = _setup(dev, sky_deterministic=True)
    runs = [[g.clone() for g in s.step()[0]] for _ in range(2)]
    for name, g in zip(NAMES + ("sky_cube_map",), runs[0]):
        assert torch.isfinite(g).all() and g.abs().sum() > 0, name
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.step()                                                 # (warm-up on the capture stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = s.step()[0]
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    runs.append([g.clone() for g in captured])
    for name, a, b, c in zip(NAMES + ("sky_cube_map",), *runs):
        assert torch.equal(a, b), f"two eager runs differ in {name}"
        assert torch.equal(a, c), f"the graph replay differs from the eager step in {name}"


def test_step_with_the_sky_switch_off_still_composes_and_agrees():
    """The same step with SkyCubeMap.deterministic off: the composition checks of test_s3g_style_step_composes hold, every gradient but the cube map's
    has the bits of the deterministic step (the sky kernel's per-pixel outputs are the same either way), and the cube map's agrees within the bar of
    test_lookup_forward_backward_vs_oracle, 1e-4 of the largest entry (float atomics add the same contributions in another order)."""
    dev = torch.device("cuda", 0)
    s = _setup(dev, sky_deterministic=False)
    assert s.sky.deterministic is False
    grads, got = s.step()
    out = got["out"]
    r, w, d = out["render"].detach().cpu(), out["weight"].detach().cpu(), out["depth"].detach().cpu()
    w2c = s.cam.world_view_transform.T
    sky_o = so.sky_s3g(s.sky.sky_cube_map.detach().cpu(), so.rays(s.H, s.W, s.K, w2c[:3, :3], w2c[:3, 3]), w)
    np.testing.assert_allclose(got["sky_color"].detach().cpu().numpy(), sky_o.numpy(), atol=2e-5)
    tot_o, _ = lo.loss_tail(so.blend_s3g(r, w, sky_o), s.gt.cpu(), d, s.gt_depth.cpu(), (~s.sky_mask).float().cpu(), w, s.sky_mask.cpu())
    np.testing.assert_allclose(got["loss"].item(), tot_o.item(), rtol=2e-5)
    for name, g in zip(NAMES + ("sky_cube_map",), grads):
        assert torch.isfinite(g).all() and g.abs().sum() > 0, name
    det = _setup(dev, sky_deterministic=True).step()[0]
    for name, a, b in zip(NAMES, grads, det):
        assert torch.equal(a, b), name
    assert float((grads[-1] - det[-1]).abs().max()) <= 1e-4 * float(det[-1].abs().max())
