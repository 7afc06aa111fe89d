"""-m gpu: the deterministic sky cube-map backward (SkyCubeMap.deterministic / EnvLight.deterministic, emd_sky_backward_det; DESIGN.md section
8.10).  dL/dcube is the pinned sum (tests/segsum_checks.py) of the call's own contribution lists, bit for bit; all gradients have identical bits
from run to run, on another stream with other work in flight and in a hipGraph replay; and the values stay inside the existing bars of
tests/test_sky_gpu.py / tests/sky_cases.py against the float64 reference."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from emd_amd import _lib as L
from tests import det_list_checks as dl
from tests import segsum_checks as sg
from tests import sky_cases as sc
from tests import test_sky_gpu as base

pytestmark = pytest.mark.gpu
ROW_PITCH = 4


def _dev():
    return torch.device("cuda", 0)


def _refuse(name):
    def f(*a, **k):
        raise AssertionError(f"{name} must not be called here")
    return f


def _backward(inp, det, want_cube=True, ws=None):
    """One call of emd_sky_backward_det (det) or emd_sky_backward through ctypes on the inputs `inp` (CPU tensors and scalars, see the builders below).
    -> dict(d_cube [6 res^2, 3] | None, d_fg, d_acc, ws, lay) as numpy arrays; the workspace is the test's own."""
    dev, lib = _dev(), L.load()
    H, W, res = inp["H"], inp["W"], inp["res"]
    P = H * W
    t = {k: v.to(dev).contiguous() for k, v in inp.items() if isinstance(v, torch.Tensor)}
    b = L.EmdSkyBwdArgs()
    b.f.height, b.f.width, b.f.resolution, b.f.flags = H, W, res, inp["flags"]
    b.f.cube = t["cube"].data_ptr()
    if "dirs" in t:
        b.f.dirs = t["dirs"].data_ptr()
    elif "camera_dev" in t:
        b.f.camera_dev = t["camera_dev"].data_ptr()
    else:
        cam = inp["cam21"]
        for i in range(9):
            b.f.Kinv[i], b.f.R[i] = cam[i], cam[9 + i]
        for i in range(3):
            b.f.T[i] = cam[18 + i]
    if "jitter" in t:
        b.f.jitter = t["jitter"].data_ptr()
    b.f.acc, b.f.fg = L.ptr(t.get("acc")), L.ptr(t.get("fg"))
    b.f.mask_threshold, b.f.fill = inp["threshold"], inp.get("fill", 0.0)
    b.dL_dout, b.dL_dsky = L.ptr(t.get("g_out")), L.ptr(t.get("g_sky"))
    d_cube = torch.full((6 * res * res, 3), float("nan"), device=dev) if want_cube else None          # the call zeroes it
    d_fg = torch.full_like(t["fg"], float("nan")) if "fg" in t else None
    d_acc = torch.full_like(t["acc"], float("nan")) if "fg" in t else None
    b.dL_dcube, b.dL_dfg, b.dL_dacc = L.ptr(d_cube), L.ptr(d_fg), L.ptr(d_acc)
    lay = None
    if det:
        if want_cube and ws is None:
            ws = torch.empty(L.sky_det_workspace_size(P), dtype=torch.uint8, device=dev)
            ws.fill_(0xA5)                                                                             # never cleared by the call, and need not be
        lay = L.sky_det_layout(P, res)
        L.check(lib.emd_sky_backward_det(C.byref(b), L.ptr(ws), 0 if ws is None else ws.numel(), L.stream()), "emd_sky_backward_det")
    else:
        L.check(lib.emd_sky_backward(C.byref(b), L.stream()), "emd_sky_backward")
    torch.cuda.synchronize()
    n = lambda x: None if x is None else x.cpu().numpy()
    return dict(d_cube=n(d_cube), d_fg=n(d_fg), d_acc=n(d_acc), ws=ws, lay=lay)


def _full_size_camera(H, W, focal):
    """The camera of test_sky_gpu.test_full_size_properties (yaw 0.3) at another size -> its 21 ray constants."""
    from emd_amd.sky import sky_ray_constants
    K = torch.tensor([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]])
    yaw = 0.3
    R = torch.tensor([[np.sin(yaw), -np.cos(yaw), 0], [0, 0, -1], [np.cos(yaw), np.sin(yaw), 0]], dtype=torch.float32)
    wvt = torch.eye(4)
    wvt[:3, :3] = R.T
    wvt[3, :3] = torch.tensor([0.3, -1.5, 0.2])
    return sky_ray_constants(K, wvt)


@functools.lru_cache(maxsize=None)
def _pinhole(H, W, res, focal, seed, covered=0.05):
    """Planar S3G call: clamp + blend, random acc of which a share `covered` lies above the sampling threshold (those pixels are not sampled)."""
    gen = torch.Generator().manual_seed(seed)
    acc = torch.rand(H, W, generator=gen) * 0.99
    acc[torch.rand(H, W, generator=gen) < covered] = 1.0
    return dict(H=H, W=W, res=res, flags=L.SKY_CLAMP01 | L.SKY_BLEND_S3G, threshold=1e-3, cam21=tuple(_full_size_camera(H, W, focal).tolist()),
                cube=torch.rand(6, res, res, 3, generator=gen) * 1.6 - 0.3, acc=acc, fg=torch.rand(3, H, W, generator=gen),
                g_out=torch.randn(3, H, W, generator=gen), g_sky=torch.randn(3, H, W, generator=gen))


@functools.lru_cache(maxsize=None)
def _dir_list(res, P, seed):
    """Interleaved OmniRe call on a direction list built as test_lookup_forward_backward_vs_oracle builds it: 64 cube-corner directions first, then
    192 on an edge (as far as P reaches)."""
    gen = torch.Generator().manual_seed(seed)
    base_map = torch.rand(6, res, res, 3, generator=gen)
    dirs = torch.randn(max(P, 256), 3, generator=gen)
    dirs[:64] = torch.tensor([1.0, 1.0, 1.0]) * torch.sign(torch.randn(64, 3, generator=gen))
    dirs[64:256, 0] = dirs[64:256, 1].abs()
    dirs = dirs[:P].contiguous()
    return dict(H=1, W=P, res=res, flags=L.SKY_INTERLEAVED | L.SKY_BLEND_ADD, threshold=-1.0, cube=base_map, dirs=dirs,
                acc=torch.rand(P, generator=gen), fg=torch.rand(P, 3, generator=gen), g_out=torch.randn(P, 3, generator=gen),
                g_sky=torch.randn(P, 3, generator=gen))


def _check_call(inp, got):
    """The lists and sums of a deterministic call (-> run lengths, raw keys, sorted slots) and its per-pixel outputs against the default entry's."""
    P = inp["H"] * inp["W"]
    lengths, raw, keys, slots = dl.check_lists(got["ws"], got["lay"], 4 * P, ROW_PITCH, 3, got["d_cube"], 6 * inp["res"] ** 2)
    default = _backward(inp, det=False)
    for q in ("d_fg", "d_acc"):                                  # per pixel, nothing shared: the same bits as the default kernel
        assert np.array_equal(got[q].view(np.uint32), default[q].view(np.uint32)), q
    # the default mode adds the same contributions with float atomics in another order
    assert np.abs(got["d_cube"] - default["d_cube"]).max() <= 1e-4 * max(np.abs(default["d_cube"]).max(), 1e-30)
    return lengths, raw, slots


def test_pinhole_gradient_is_the_pinned_sum_of_the_calls_own_lists():
    """64 x 96 pixels on 4^2 faces: every texel in view collects hundreds to thousands of taps, so all three run classes of the segmented sum occur
    (one chunk, two chunks, more than two)."""
    inp = _pinhole(64, 96, 4, 60.0, seed=11)
    got = _backward(inp, det=True)
    P = 64 * 96
    rows, raw, keys, slots, count = dl.read_workspace(got["ws"], got["lay"], 4 * P, ROW_PITCH)
    lengths = sg.run_structure(keys.astype(np.int64))[1]
    print(f"pinhole: {count} of {4 * P} slots kept, {len(lengths)} texels touched, runs > 1024 / 513..1024 / <= 512: "
          f"{(lengths > 1024).sum()} / {((lengths > 512) & (lengths <= 1024)).sum()} / {(lengths <= 512).sum()}, longest {lengths.max()}")
    assert (lengths > 2 * sg.SEG_CHUNK).any() and ((lengths > sg.SEG_CHUNK) & (lengths <= 2 * sg.SEG_CHUNK)).any() and (lengths <= sg.SEG_CHUNK).any()
    # not sampled (acc above the threshold): all four slots of the pixel are dropped
    masked = np.flatnonzero(~((1 - inp["acc"].reshape(-1).numpy()) > np.float32(1e-3)))
    assert len(masked) > 0 and all((raw[k * P + masked] == dl.DROPPED).all() for k in range(4))
    _check_call(inp, got)


def test_direction_list_gradient_is_the_pinned_sum_and_corner_taps_are_dropped():
    inp = _dir_list(8, 2000, seed=0)
    got = _backward(inp, det=True)
    P = 2000
    lengths, raw, slots = _check_call(inp, got)
    dropped = np.flatnonzero(raw == dl.DROPPED)
    print(f"direction list: {len(dropped)} of {4 * P} slots dropped (weight zero), {len(lengths)} texels touched, longest run {lengths.max()}")
    assert len(dropped) > 0
    assert (dropped % P < 64).any()                              # among them taps of the cube-corner directions: the missing fourth tap


@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("case_id", list(sc.CASES) + list(sc.VARIANTS))
def test_parity_with_the_float64_reference(case_id, white, monkeypatch):
    """Every case of tests/sky_cases.py through composite_s3g / SkyCubeMap.forward with the switch on, held to sc.bar(...) as the default mode is."""
    from emd_amd.sky import SkyCubeMap
    monkeypatch.setattr(SkyCubeMap, "deterministic", True)
    monkeypatch.setattr(L.load(), "emd_sky_backward", _refuse("emd_sky_backward"))
    c = sc.build(case_id, white)
    extra = dict(sky_mask=c.sky_mask.to(_dev())) if c.sky_mask is not None else {}
    base._check(base._run(c, base._camera(c, _dev(), **extra)), c)


@pytest.mark.parametrize("res,P,seed", [(8, 20000, 0), (33, 50000, 2)])
def test_parity_with_cube_lookup_autograd(res, P, seed, monkeypatch):
    """test_lookup_forward_backward_vs_oracle as it stands (EnvLight / composite_add against so.cube_lookup autograd, dL/dcube within 1e-4 of the
    largest entry), with the switch on."""
    from emd_amd.sky import EnvLight
    monkeypatch.setattr(EnvLight, "deterministic", True)
    monkeypatch.setattr(L.load(), "emd_sky_backward", _refuse("emd_sky_backward"))
    base.test_lookup_forward_backward_vs_oracle(res, P, seed)


def _python_step(c, model, cam, static):
    """composite_s3g + backward on static device inputs -> (dL/dcube, dL/drender, dL/dweight)."""
    from emd_amd.sky import composite_s3g
    out, sky = composite_s3g(model, cam, static["render"], static["weight"])
    return torch.autograd.grad(sc.loss(out, sky, static["g_out"], static["g_sky"]), [model.sky_cube_map, static["render"], static["weight"]])


def test_identical_bits_across_runs_streams_and_graph_replay(monkeypatch):
    from emd_amd.sky import SkyCubeMap
    monkeypatch.setattr(L.load(), "emd_sky_backward", _refuse("emd_sky_backward"))
    dev = _dev()
    c = sc.build("corner-mag", False)                            # 37 x 53 pixels on 64^2 faces: many pixels per texel, three faces in view
    cfg = types.SimpleNamespace(sky_resolution=c.res, sky_white_background=c.white, white_background=False)
    model = SkyCubeMap(cfg, device=dev, deterministic=True)
    model.sky_cube_map.data = c.cube.to(dev)
    cam = base._camera(c, dev)
    static = dict(render=c.render.to(dev).requires_grad_(True), weight=c.acc.to(dev).requires_grad_(True), g_out=c.g_out.to(dev), g_sky=c.g_sky.to(dev))
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    first = [g.clone() for g in _python_step(c, model, cam, static)]
    assert float(first[0].abs().max()) > 0
    assert same(first, _python_step(c, model, cam, static))                         # twice on the default stream
    # on a side stream, with other kernels in flight on the default stream
    busy = torch.randn(2048, 2048, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(8):
        busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        on_side = [g.clone() for g in _python_step(c, model, cam, static)]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert same(first, on_side)
    # forward + backward captured on one stream and replayed
    with torch.cuda.stream(side):
        _python_step(c, model, cam, static)                                         # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _python_step(c, model, cam, static)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same(first, captured)


@pytest.mark.parametrize("P", [1, 255, 512, 513])
def test_edges_of_the_chunk_and_the_block_on_the_list_path(P):
    inp = _dir_list(8, P, seed=3)
    _check_call(inp, _backward(inp, det=True))


def test_image_that_is_no_multiple_of_the_tile_or_the_block():
    inp = _pinhole(37, 53, 4, 35.0, seed=12)
    _check_call(inp, _backward(inp, det=True))


def test_device_camera_and_jitter_give_the_pinned_sum_too():
    """camera_dev (the 21 floats on the device) and a jitter draw: the other two ways a pinhole call is made."""
    inp = dict(_pinhole(37, 53, 4, 35.0, seed=12))
    host = _backward(inp, det=True)
    inp["camera_dev"] = torch.tensor(inp["cam21"], dtype=torch.float32)
    got = _backward(inp, det=True)
    for q in ("d_cube", "d_fg", "d_acc"):
        assert np.array_equal(got[q].view(np.uint32), host[q].view(np.uint32)), q                 # the same arithmetic on the same numbers
    inp["jitter"] = torch.rand(37, 53, 2, generator=torch.Generator().manual_seed(4))
    _check_call(inp, _backward(inp, det=True))


def test_every_pixel_masked_out():
    inp = dict(_pinhole(37, 53, 4, 35.0, seed=12))
    inp["acc"] = torch.ones(37, 53)
    got = _backward(inp, det=True)
    rows, raw, keys, slots, count = dl.read_workspace(got["ws"], got["lay"], 4 * 37 * 53, ROW_PITCH)
    assert count == 0 and (raw == dl.DROPPED).all()
    assert (got["d_cube"].view(np.uint32) == 0).all()                                               # +0.0 everywhere
    _check_call(inp, got)


def test_without_a_cube_gradient_no_workspace_is_needed():
    inp = _pinhole(37, 53, 4, 35.0, seed=12)
    got, default = _backward(inp, det=True, want_cube=False), _backward(inp, det=False, want_cube=False)
    assert got["ws"] is None and got["d_cube"] is None
    for q in ("d_fg", "d_acc"):
        assert np.isfinite(got[q]).all() and np.array_equal(got[q].view(np.uint32), default[q].view(np.uint32)), q


def test_default_mode_is_untouched_in_behaviour(monkeypatch):
    """With the switch off composite_s3g and composite_add go through emd_sky_backward and nothing of the mode: the same results as a direct call of
    that entry, inside the existing bars of their tests."""
    from emd_amd.sky import EnvLight, SkyCubeMap, composite_add
    assert SkyCubeMap.deterministic is False and EnvLight.deterministic is False
    monkeypatch.setattr(L.load(), "emd_sky_backward_det", _refuse("emd_sky_backward_det"))
    monkeypatch.setattr(L, "sky_det_workspace_size", _refuse("sky_det_workspace_size"))
    dev = _dev()
    # composite_s3g
    c = sc.build("corner-64", False)
    cam = base._camera(c, dev)
    got = base._run(c, cam)
    base._check(got, c)
    from emd_amd.sky import sky_ray_constants
    direct = _backward(dict(H=c.H, W=c.W, res=c.res, flags=L.SKY_CLAMP01 | L.SKY_BLEND_S3G, threshold=1e-3, fill=c.fill,
                            cam21=tuple(sky_ray_constants(cam.intrinsic, cam.world_view_transform).tolist()), cube=c.cube, acc=c.acc[0], fg=c.render,
                            g_out=2.0 * c.g_out, g_sky=2.0 * c.g_sky), det=False)                    # (sc.loss carries a factor 2)
    assert np.array_equal(got["d_render"].numpy().view(np.uint32), direct["d_fg"].view(np.uint32))
    assert np.array_equal(got["d_weight"].numpy().reshape(c.H, c.W).view(np.uint32), direct["d_acc"].view(np.uint32))
    assert np.abs(got["d_cube"].numpy().reshape(-1, 3) - direct["d_cube"]).max() <= 2 * sc.bar(c.id, "d_cube")     # each within the bar of the reference
    # composite_add
    inp = _dir_list(8, 20000, seed=0)
    env = EnvLight(resolution=8, device=dev)
    env.base.data = inp["cube"].to(dev)
    r1, o1 = inp["fg"].to(dev).requires_grad_(True), inp["acc"].reshape(-1, 1).to(dev).requires_grad_(True)
    out1, sky1 = composite_add(env, {"viewdirs": (inp["dirs"] @ env.to_opengl.cpu()).to(dev)}, r1, o1)
    ((out1 * inp["g_out"].to(dev)).sum() + (sky1 * inp["g_sky"].to(dev)).sum()).backward()
    direct = _backward(inp, det=False)
    assert np.array_equal(r1.grad.cpu().numpy().view(np.uint32), direct["d_fg"].view(np.uint32))
    assert np.array_equal(o1.grad.cpu().numpy().reshape(-1).view(np.uint32), direct["d_acc"].view(np.uint32))
    gb = env.base.grad.cpu().numpy().reshape(-1, 3)
    assert np.abs(gb - direct["d_cube"]).max() <= 1e-4 * np.abs(direct["d_cube"]).max()
