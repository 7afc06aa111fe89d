"""Cost of the deterministic sky and motion backward (SkyCubeMap.deterministic, transform_gaussians(deterministic=True)).
  sky:    composite_s3g at 1066 x 1600 with 1024^2 faces, the scene of tests/test_sky_gpu.py::test_full_size_properties;
  motion: transform_gaussians at 2 M points of which 160 k sit on 32 actors (5 000 each, interleaved with the static ones), residuals on.
In ONE run per op: the backward with and without the mode (median of 30 between HIP events, min - max beside it, the two modes interleaved in two
halves); the added launches on their own (row kernel, sort, sum: device time per kernel family from the profiler); the workspace bytes; the
run-length statistics of the lists (sky: from the sorted keys a direct call of emd_sky_backward_det leaves in its workspace).
    python profiles/sky_motion_deterministic_microbench.py [OUT.json]      -> profiles/sky_motion_deterministic_microbench.json"""
import ctypes as C
import json
import os
import statistics
import sys
import types

import numpy as np
import torch

sys.path.insert(0, ".")
from emd_amd import _lib as L  # noqa: E402
from emd_amd import motion  # noqa: E402
from emd_amd.sky import SkyCubeMap, composite_s3g, sky_ray_constants  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

REPS, PASSES = 30, 3
dev = torch.device("cuda", 0)


def timed(step, reps):
    """step() -> a scalar whose backward is the op under test; only the backward is between the events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        loss = step()
        e0.record()
        loss.backward()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "reps": len(ms)}


def both_modes(step, set_mode):
    samples = {"default": [], "deterministic": []}
    for mode in (False, True, False, True):                 # both modes in two halves, interleaved: two warm-up passes, then the timed repetitions
        set_mode(mode)
        timed(step, 2)
        samples["deterministic" if mode else "default"] += timed(step, REPS // 2)
    return {k: summary(v) for k, v in samples.items()}


def added_launches(step, fams):
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        timed(step, PASSES)
    launches = {k: {"ms": 0.0, "launches": 0} for k in fams}
    for ev in prof.key_averages():
        for fam, names in fams.items():
            if any(nm in ev.key for nm in names):
                dt = getattr(ev, "device_time_total", None)
                launches[fam]["ms"] += (ev.cuda_time_total if dt is None else dt) / 1e3 / PASSES
                launches[fam]["launches"] += ev.count // PASSES
    return {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in launches.items()}


def run_stats(cnt):
    cnt = cnt.double()
    return {"runs": int(cnt.numel()), "median": float(cnt.median()), "mean": round(float(cnt.mean()), 2), "max": int(cnt.max()),
            "longer_than_a_chunk": int((cnt > L.SEG_CHUNK).sum()), "chunk": L.SEG_CHUNK}


# ---- sky ----------------------------------------------------------------------------------------------------------------------------------
H, W, RES = 1066, 1600, 1024
K = torch.tensor([[1700.0, 0, 800.0], [0, 1700.0, 533.0], [0, 0, 1]], device=dev)
yaw = 0.3
R = torch.tensor([[np.sin(yaw), -np.cos(yaw), 0], [0, 0, -1], [np.cos(yaw), np.sin(yaw), 0]], dtype=torch.float32)
wvt = torch.eye(4)
wvt[:3, :3] = R.T
wvt[3, :3] = torch.tensor([0.3, -1.5, 0.2])
cam = types.SimpleNamespace(image_height=H, image_width=W, intrinsic=K, world_view_transform=wvt.to(dev))
sky = SkyCubeMap(types.SimpleNamespace(sky_resolution=RES, sky_white_background=False, white_background=False), device=dev)
gen = torch.Generator().manual_seed(5)
sky.sky_cube_map.data = (torch.rand(6, RES, RES, 3, generator=gen) * 0.8 + 0.1).to(dev)
acc = torch.rand(1, H, W, generator=gen).to(dev).requires_grad_(True)
render = torch.rand(3, H, W, generator=gen).to(dev).requires_grad_(True)
g_out = torch.randn(3, H, W, generator=gen).to(dev)


def sky_step():
    sky.sky_cube_map.grad = acc.grad = render.grad = None
    out, _ = composite_s3g(sky, cam, render, acc)
    return (out * g_out).sum()


res = {"sky": {"op": f"composite_s3g backward, {H} x {W} pixels, {RES}^2 faces (cube map, render and weight gradients), default against deterministic"}}
res["sky"].update(both_modes(sky_step, lambda m: setattr(sky, "deterministic", m)))
sky.deterministic = True
res["sky"]["added_launches_per_backward"] = added_launches(sky_step, {"row kernel": ("k_sky_det_rows",), "sort": ("k_radix_",), "sum": ("k_segsum_",)})
P = H * W
res["sky"]["workspace_bytes"] = L.sky_det_workspace_size(P)
res["sky"]["rows_bytes"] = 16 * 4 * P
# the lists of one call, from its own workspace
b = L.EmdSkyBwdArgs()
b.f.height, b.f.width, b.f.resolution, b.f.flags = H, W, RES, L.SKY_CLAMP01 | L.SKY_BLEND_S3G
vals = sky_ray_constants(K, cam.world_view_transform).tolist()
for i in range(9):
    b.f.Kinv[i], b.f.R[i] = vals[i], vals[9 + i]
for i in range(3):
    b.f.T[i] = vals[18 + i]
cube, a0, fg = sky.sky_cube_map.detach().contiguous(), acc.detach().reshape(H, W).contiguous(), render.detach().contiguous()
b.f.cube, b.f.acc, b.f.fg, b.f.mask_threshold = cube.data_ptr(), a0.data_ptr(), fg.data_ptr(), 1e-3
d_cube = torch.empty_like(cube)
b.dL_dout, b.dL_dcube = g_out.data_ptr(), d_cube.data_ptr()
ws = torch.empty(res["sky"]["workspace_bytes"], dtype=torch.uint8, device=dev)
L.check(L.load().emd_sky_backward_det(C.byref(b), ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "emd_sky_backward_det")
torch.cuda.synchronize()
lay = L.sky_det_layout(P, RES)
count = int(ws[lay["counts"]:lay["counts"] + 4].view(torch.int32)[0])
keys = ws[lay["keys"]:lay["keys"] + 4 * count].view(torch.int32)
res["sky"]["slots"] = {"total": 4 * P, "kept": count}
res["sky"]["run_lengths"] = run_stats(torch.unique_consecutive(keys, return_counts=True)[1])
del ws, d_cube

# ---- motion -------------------------------------------------------------------------------------------------------------------------------
N, A, PER = 2_000_000, 32, 5000
rng = np.random.default_rng(0)
ids = np.full(N, -1, np.int32)
ids[:A * PER] = np.repeat(np.arange(A, dtype=np.int32), PER)
ids = torch.from_numpy(ids[rng.permutation(N)]).to(dev)
pose = torch.randn(A, 12, generator=gen)
pose[:, 0:4] /= pose[:, 0:4].norm(dim=1, keepdim=True)
pose[:, 8:12] /= pose[:, 8:12].norm(dim=1, keepdim=True)
pose[:, 7] = 1.0
t = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=gen)).to(dev).requires_grad_(True)
means, quats, opac, rdx, rdq, pose = t(N, 3), t(N, 4), torch.rand(N, generator=gen).to(dev).requires_grad_(True), t(N, 3, s=0.05), t(N, 4, s=0.05), pose.to(dev).requires_grad_(True)
leaves = (means, quats, opac, rdx, rdq, pose)
g_wm, g_wq, g_wo = torch.randn(N, 3, generator=gen).to(dev), torch.randn(N, 4, generator=gen).to(dev), torch.randn(N, generator=gen).to(dev)
mode = {"det": False}


def motion_step():
    for x in leaves:
        x.grad = None
    wm, wq, wo = motion.transform_gaussians(means, quats, opac, ids, pose, rdx, rdq, deterministic=mode["det"])
    return (wm * g_wm).sum() + (wq * g_wq).sum() + (wo * g_wo).sum()


res["motion"] = {"op": f"transform_gaussians backward, {N} points of which {A * PER} on {A} actors, residuals on, default against deterministic"}
res["motion"].update(both_modes(motion_step, lambda m: mode.update(det=m)))
mode["det"] = True
res["motion"]["added_launches_per_backward"] = added_launches(motion_step, {"motion kernel (rows in place of atomics)": ("k_motion_backward_det",),
                                                                           "sort": ("k_radix_",), "sum": ("k_segsum_",)})
mode["det"] = False
res["motion"]["default_motion_kernel"] = added_launches(motion_step, {"motion kernel": ("k_motion_backward",)})
res["motion"]["workspace_bytes"] = L.motion_det_workspace_size(N)
res["motion"]["rows_bytes"] = 48 * N
res["motion"]["run_lengths"] = run_stats(torch.bincount(ids[ids >= 0].long(), minlength=A))

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "sky_motion_deterministic_microbench.json")
open(out, "w").write(json.dumps(res, indent=1) + "\n")
print(json.dumps(res))
