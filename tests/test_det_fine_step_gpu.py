"""-m gpu: S3Gaussian's fine-stage step with every deterministic switch it has -- DeformOptions.deterministic (the HexPlane backward, DESIGN.md section
8.9; the MLP kernels and the temporal table, section 8.14) and RasterOptions.deterministic (section 8.8) -- at the small size of
tests/test_det_step_gpu.py: deformation network (both levels, every head, the regularisers folded into the head kernels) -> rasterizer with the
feature passes -> image-loss tail -> backward.  Every gradient of the step -- the Gaussians' parameters, the embeddings, and every parameter of the
network: planes, temporal table, time_offset, all MLP weights -- is finite, non-zero and has identical bits in two eager runs, on a side stream and
in a hipGraph replay.  Nothing here asserts that the default mode DIFFERS between runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu
GAUSSIAN = ("_xyz", "_scaling", "_rotation", "_opacity", "_features")


def _setup(dev):
    from emd_amd import RasterOptions, scenes
    from emd_amd.deformation import DeformOptions, deform_network
    from emd_amd.loss import image_loss
    from emd_amd.model import StreetGaussians, render, residual_abs_mean
    N, H, W = 6000, 96, 160
    model = StreetGaussians(scenes.make_static_scene(N, seed=0), dev)
    torch.manual_seed(3)
    # every head of both levels takes part (the run script switches the scale and rotation heads off: their weights would have no gradient)
    net = deform_network(DeformOptions(deterministic=True, multires=[1, 2], no_ds=False, no_dr=False,
                                       kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32,
                                                       "resolution": [16, 16, 16, 8]})).to(dev)
    net.deformation_net.set_aabb([120.0, 30.0, 10.0], [0.0, -30.0, -2.0])
    for n_, p_ in net.named_parameters():
        if p_.dim() > 1 and "grid" not in n_:
            p_.data.mul_(0.05)
    emb = torch.nn.Parameter(0.1 * torch.randn(N, 4, device=dev))
    cam = scenes.rig_camera(2, 0, H, W)
    g = torch.Generator().manual_seed(9)
    gt = torch.rand(3, H, W, generator=g).to(dev)
    gt_depth = (torch.rand(1, H, W, generator=g) * 60).to(dev)
    sky_mask = (torch.rand(1, H, W, generator=g) < 0.3).to(dev)
    not_sky = ~sky_mask
    feat_gt = torch.rand(3, H, W, generator=g).to(dev)
    opts = RasterOptions(deterministic=True, no_sync=True, capacity_hint=1 << 20)
    trained = [(n, p) for n, p in net.named_parameters() if p.requires_grad]          # (all but the HexPlane's bounding box, a constant kept as a parameter)
    assert len(trained) >= len(list(net.named_parameters())) - 1
    names = list(GAUSSIAN) + ["embeddings"] + [n for n, _ in trained]
    leaves = [getattr(model, n) for n in GAUSSIAN] + [emb] + [p for _, p in trained]
    bg = torch.zeros(3)

    def step():
        out = render(model, cam, bg, frame=2, deformation=net, embeddings=emb, iteration=12000, time=0.4, fused_l1=("dx", "dshs"), options=opts,
                     render_feat=True)
        loss, _ = image_loss(out["render"], gt, out["depth"], gt_depth, not_sky, out["weight"], sky_mask)
        for lvl in ("coarse", "fine"):
            d = out["ddict"][lvl]
            loss = loss + 0.02 * residual_abs_mean(d, "dx") + 0.01 * residual_abs_mean(d, "dshs")
        loss = loss + 0.1 * ((out["feat_c"] - feat_gt).abs().mean() + (out["feat_f"] - feat_gt).abs().mean())          # (the feature head of both levels)
        return list(torch.autograd.grad(loss, leaves))
    return step, names


def test_fine_stage_step_has_identical_bits_across_runs_streams_and_in_a_graph_replay():
    dev = torch.device("cuda", 0)
    step, names = _setup(dev)
    assert any("grid" in n for n in names) and any(n.endswith("deformation_net.weight") for n in names) and any("time_offset" in n for n in names)
    runs = [[g.clone() for g in step()] for _ in range(2)]
    for name, g in zip(names, runs[0]):
        assert torch.isfinite(g).all() and g.abs().sum() > 0, name
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append([g.clone() for g in step()])                 # (also the warm-up on the capture stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = step()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    runs.append([g.clone() for g in captured])
    for name, a, b, c, d in zip(names, *runs):
        assert torch.equal(a, b), f"two eager runs differ in {name}"
        assert torch.equal(a, c), f"the run on a side stream differs from the eager step in {name}"
        assert torch.equal(a, d), f"the graph replay differs from the eager step in {name}"
