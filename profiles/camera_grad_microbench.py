"""The two launches of the camera gradient (csrc/camera_grad.hip) beside the projection backward (K8) at the headline shape: 2 M Gaussians of
which 32 x 5000 ride on actors, 1066 x 1600, raw parameters.  One forward + render backward, then each of the two is timed on the SAME
accumulator rows (they stay in place without EMD_FLAG_BWD_WS_CLEAN): median of `--reps` launches between HIP events.
    python profiles/camera_grad_microbench.py [--n 2000000] [--reps 30] [--out profiles/camera_grad_microbench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emd_amd import GaussianRasterizationSettings, GaussianRasterizer, scenes  # noqa: E402
from emd_amd import _lib as L  # noqa: E402
from emd_amd.motion import build_actor_pose  # noqa: E402
from emd_amd.rasterizer import make_c_settings  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "camera_grad_microbench.json"))
    a = ap.parse_args()
    dev, H, W, N = "cuda:0", 1066, 1600, a.n
    sc = scenes.add_actors(scenes.make_static_scene(N, seed=0), num_actors=32, pts_per_actor=5000, num_frames=50, seed=1)
    pose = build_actor_pose(sc.actor_quats, sc.actor_trans, sc.actor_valid, 0)
    cam = scenes.rig_camera(0, 0, H, W)
    leaf = lambda t: t.to(dev).clone().requires_grad_(True)
    V, P, c = leaf(cam.world_view_transform), leaf(cam.full_proj_transform), leaf(cam.camera_center)
    rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0, V, P, 3, c, False, False)
    T = dict(means3D=leaf(sc.means), shs=leaf(sc.shs), opacities=leaf(sc.opacity_logits), scales=leaf(sc.log_scales), rotations=leaf(sc.quats),
             actor_pose=leaf(pose))
    ids = sc.actor_id.to(dev)
    rast = GaussianRasterizer(rs, compute_normal=False, keep_render_grads=True)
    m2 = torch.zeros(N, 3, device=dev, requires_grad=True)
    color, depth, normal, alpha, radii, _ = rast(means2D=m2, raw_params=True, actor_ids=ids, **T)
    (color.sum() + 0.01 * depth.sum() + alpha.sum()).backward()
    torch.cuda.synchronize()
    call = rast.last_call
    b = L.EmdBwdArgs()
    b.s, _ = make_c_settings(GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0, cam.world_view_transform,
                                                           cam.full_proj_transform, 3, cam.camera_center, False, False))
    b.settings_dev = L.ptr(call.settings_dev)
    b.num_gaussians, b.sh_coeffs, b.flags, b.bin_capacity, b.num_rendered = N, T["shs"].shape[1], call.flags, call.capacity, call.num_rendered
    b.means3D, b.shs, b.opacities, b.scales, b.rotations = (T[k].data_ptr() for k in ("means3D", "shs", "opacities", "scales", "rotations"))
    b.motion.actor_id, b.motion.actor_pose, b.motion.num_actors = ids.data_ptr(), T["actor_pose"].data_ptr(), pose.shape[0]
    b.radii = call.radii.data_ptr()
    b.geom_ws, b.geom_bytes, b.bin_ws, b.bin_bytes, b.img_ws, b.img_bytes = (call.geom_ws.data_ptr(), call.sizes[0], call.bin_ws.data_ptr(),
                                                                              call.sizes[1], call.img_ws.data_ptr(), call.sizes[2])
    b.status, b.out_color, b.out_depth = call.status.data_ptr(), color.data_ptr(), depth.data_ptr()
    b.bwd_ws, b.bwd_bytes = call.render_grads.data_ptr(), call.render_grads.numel() * 4
    z = lambda *s: torch.empty(*s, device=dev)
    outs = [z(N, 3), z(N, 3), z(N, 16, 3), z(N), z(N, 3), z(N, 4), torch.zeros(pose.shape, device=dev)]
    b.dL_dmeans3D, b.dL_dmeans2D, b.dL_dshs, b.dL_dopacities, b.dL_dscales, b.dL_drotations, b.dL_dactor_pose = (o.data_ptr() for o in outs)
    lib, st = L.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws_bytes = L.camera_grad_workspace_size(N)
    ws, g35 = torch.empty(ws_bytes // 4, device=dev), torch.empty(35, device=dev)

    def camera():
        b.flags = call.flags
        L.check(lib.emd_raster_backward_camera(C.byref(b), g35.data_ptr(), ws.data_ptr(), ws_bytes, st), "camera")

    def project():
        b.flags = call.flags | L.FLAG_BWD_PROJECT_ONLY
        L.check(lib.emd_raster_backward(C.byref(b), st), "projection half")

    def timed(fn):
        ts = []
        for _ in range(a.reps + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = sorted(ts[5:])
        return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4))
    res = dict(num_gaussians=N, height=H, width=W, visible=int((radii > 0).sum()), reps=a.reps,
               camera_backward_two_launches=timed(camera), preprocess_backward_K8=timed(project),
               matches_autograd=bool(torch.equal(g35, call.camera_grad)))
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
