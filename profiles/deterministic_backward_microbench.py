"""What the deterministic backward (EMD_FLAG_DETERMINISTIC) costs at the headline shape: 2 M Gaussians of which 32 x 5000 ride on
actors, 1066 x 1600, raw parameters.  One forward; then, on that forward's state and in the SAME run, the backward through the C ABI with and without
the flag (whole, and its two halves), median of `--reps` between HIP events.  The added launches are timed on their own through the exported entry
points on the call's own lists: the two sorts (emd_radix_sort on the raw keys the backward left in its workspace) and the two segmented sums
(emd_segmented_row_sum on the sorted lists).  The two key builds have no entry point of their own: they are reported by difference, together with
whatever the storing K7 / K8 variants cost or save against the atomic ones.  Rows per destination: median / maximum of the run lengths.
    python profiles/deterministic_backward_microbench.py [--n 2000000] [--reps 30] [--out profiles/deterministic_backward_microbench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emd_amd import GaussianRasterizationSettings, GaussianRasterizer, scenes  # noqa: E402
from emd_amd import _lib as L  # noqa: E402
from emd_amd.motion import build_actor_pose  # noqa: E402
from emd_amd.rasterizer import _det_views, make_c_settings  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "deterministic_backward_microbench.json"))
    a = ap.parse_args()
    dev, H, W, N = "cuda:0", 1066, 1600, a.n
    sc = scenes.add_actors(scenes.make_static_scene(N, seed=0), num_actors=32, pts_per_actor=5000, num_frames=50, seed=1)
    pose = build_actor_pose(sc.actor_quats, sc.actor_trans, sc.actor_valid, 0)
    cam = scenes.rig_camera(0, 0, H, W)
    d = lambda t: t.to(dev).clone()
    rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0, d(cam.world_view_transform),
                                       d(cam.full_proj_transform), 3, d(cam.camera_center), False, False)
    T = dict(means3D=d(sc.means), shs=d(sc.shs), opacities=d(sc.opacity_logits), scales=d(sc.log_scales), rotations=d(sc.quats), actor_pose=d(pose))
    ids = sc.actor_id.to(dev)
    A = pose.shape[0]
    rast = GaussianRasterizer(rs, compute_normal=False)
    with torch.no_grad():
        color, depth, normal, alpha, radii, _ = rast(means2D=torch.zeros(N, 3, device=dev), raw_params=True, actor_ids=ids, **T)
    torch.cuda.synchronize()
    call = rast.last_call
    g = torch.Generator(device=dev).manual_seed(17)
    gC, gD, gA = torch.randn(3, H, W, device=dev, generator=g), 0.01 * torch.randn(1, H, W, device=dev, generator=g), torch.randn(1, H, W, device=dev, generator=g)
    b = L.EmdBwdArgs()
    b.s, _ = make_c_settings(GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0, cam.world_view_transform,
                                                           cam.full_proj_transform, 3, cam.camera_center, False, False))
    b.settings_dev = L.ptr(call.settings_dev)
    b.num_gaussians, b.sh_coeffs, b.bin_capacity, b.num_rendered = N, T["shs"].shape[1], call.capacity, call.num_rendered
    b.means3D, b.shs, b.opacities, b.scales, b.rotations = (T[k].data_ptr() for k in ("means3D", "shs", "opacities", "scales", "rotations"))
    b.motion.actor_id, b.motion.actor_pose, b.motion.num_actors = ids.data_ptr(), T["actor_pose"].data_ptr(), A
    b.radii = call.radii.data_ptr()
    b.geom_ws, b.geom_bytes, b.bin_ws, b.bin_bytes, b.img_ws, b.img_bytes = (call.geom_ws.data_ptr(), call.sizes[0], call.bin_ws.data_ptr(),
                                                                              call.sizes[1], call.img_ws.data_ptr(), call.sizes[2])
    b.status, b.out_color, b.out_depth = call.status.data_ptr(), color.data_ptr(), depth.data_ptr()
    b.dL_dcolor, b.dL_ddepth, b.dL_dalpha = gC.data_ptr(), gD.data_ptr(), gA.data_ptr()
    bwd_ws = torch.empty(N * L.BWD_STRIDE, device=dev)
    b.bwd_ws, b.bwd_bytes = bwd_ws.data_ptr(), bwd_ws.numel() * 4
    z = lambda *s: torch.empty(*s, device=dev)
    outs = [z(N, 3), z(N, 3), z(N, 16, 3), z(N), z(N, 3), z(N, 4), z(A, 12)]
    b.dL_dmeans3D, b.dL_dmeans2D, b.dL_dshs, b.dL_dopacities, b.dL_dscales, b.dL_drotations, b.dL_dactor_pose = (o.data_ptr() for o in outs)
    det_bytes = L.det_workspace_size(N, call.capacity, 0)
    det_ws = torch.empty(det_bytes, device=dev, dtype=torch.uint8)
    b.det_ws, b.det_bytes = det_ws.data_ptr(), det_bytes
    lib, st = L.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def backward(extra):
        def fn():
            b.flags = call.flags | extra
            L.check(lib.emd_raster_backward(C.byref(b), st), "backward")
        return fn

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

    DET, RO, PO = L.FLAG_DETERMINISTIC, L.FLAG_BWD_RENDER_ONLY, L.FLAG_BWD_PROJECT_ONLY
    res = dict(num_gaussians=N, height=H, width=W, visible=int((radii > 0).sum()), capacity=int(call.capacity), reps=a.reps,
               det_workspace_bytes=det_bytes)
    # (the projection half consumes nothing: without EMD_FLAG_BWD_WS_CLEAN the accumulator rows stay in place, so each half can be repeated)
    res["backward_default"] = timed(backward(0))
    res["backward_deterministic"] = timed(backward(DET))
    res["render_half_default"] = timed(backward(RO))
    res["render_half_deterministic"] = timed(backward(RO | DET))
    res["projection_half_default"] = timed(backward(PO))
    res["projection_half_deterministic"] = timed(backward(PO | DET))
    backward(DET)()
    torch.cuda.synchronize()
    # two deterministic passes give the same bits (the premise of the exercise)
    first = [o.clone() for o in outs]
    backward(DET)()
    torch.cuda.synchronize()
    res["two_passes_bit_identical"] = all(torch.equal(x, y) for x, y in zip(first, outs))

    # ---- the added launches on their own, on this call's lists --------------------------------------------------------------------------------
    lay = L.det_layout(N, call.capacity, 0, A)
    views = _det_views(det_ws, N, call.capacity, 0, A)
    counts = views["counts"].cpu().numpy().view(np.uint32)
    R = views["rows"].shape[0]
    bits = lambda n: max(int(n - 1).bit_length(), 1)
    passes = lambda n: (bits(n) + 8) // 9
    u32 = lambda n: torch.empty(n, device=dev, dtype=torch.int32)

    def sort_call(raw_off, n_cap, n_ids, n_dev_ptr):
        k, v, hist, cnt = [u32(n_cap), u32(n_cap)], [u32(n_cap), u32(n_cap)], u32(512 * ((n_cap + 2047) // 2048)), u32(4)
        s = L.EmdRadixSortArgs()
        s.keys_in = det_ws.data_ptr() + raw_off
        s.keys[0], s.keys[1], s.vals[0], s.vals[1], s.hist = k[0].data_ptr(), k[1].data_ptr(), v[0].data_ptr(), v[1].data_ptr(), hist.data_ptr()
        s.n_cap, s.n_dev, s.passes, s.range_bits, s.count_out = n_cap, n_dev_ptr, passes(n_ids), 32, cnt.data_ptr()
        s.bits = (bits(n_ids) + s.passes - 1) // s.passes
        keep = (k, v, hist, cnt)

        def fn(_keep=keep):
            assert lib.emd_radix_sort(C.byref(s), st) >= 0, lib.emd_last_error()
        return fn

    def sum_call(keys, slots, n_cap, n_dev_ptr, rows, pitch, width, out, out_pitch):
        pb = lib.emd_segmented_row_sum_workspace(n_cap, width)
        par = torch.empty(pb // 8 + 1, device=dev, dtype=torch.float64)
        s = L.EmdSegSumArgs()
        s.keys, s.slots, s.n_dev, s.n_cap = keys.data_ptr(), slots.data_ptr(), n_dev_ptr, n_cap
        s.rows, s.row_pitch, s.width, s.out, s.out_pitch, s.partials, s.partial_bytes = rows.data_ptr(), pitch, width, out.data_ptr(), out_pitch, par.data_ptr(), pb

        def fn(_keep=par):
            L.check(lib.emd_segmented_row_sum(C.byref(s), st), "segmented_row_sum")
        return fn

    cptr = views["counts"].data_ptr()
    scratch_rows, scratch_pose = torch.zeros(N * L.BWD_STRIDE, device=dev), torch.zeros(A * 12, device=dev)
    res["launches"] = dict(
        render_sort=dict(timed(sort_call(lay["raw_keys"], R, N, cptr)), passes=passes(N), kernels=3 * passes(N)),
        render_sum=dict(timed(sum_call(views["keys"], views["slots"], R, cptr + 4, views["rows"], L.BWD_STRIDE, 12, scratch_rows, L.BWD_STRIDE)), kernels=2),
        pose_sort=dict(timed(sort_call(lay["pose_raw_keys"], N, A, None)), passes=passes(A), kernels=3 * passes(A)),
        pose_sum=dict(timed(sum_call(views["pose_keys"], views["pose_points"], N, cptr + 8, views["pose_rows"], 12, 12, scratch_pose, 12)), kernels=2))
    torch.cuda.synchronize()
    res["sum_on_its_own_equals_the_backward"] = bool(torch.equal(scratch_rows, bwd_ws)) and bool(torch.equal(scratch_pose.view(A, 12), outs[6]))
    m = lambda k: res[k]["median_ms"]
    ln = res["launches"]
    res["key_builds_and_kernel_variants_by_difference_ms"] = dict(
        render_half=round(m("render_half_deterministic") - m("render_half_default") - ln["render_sort"]["median_ms"] - ln["render_sum"]["median_ms"], 4),
        projection_half=round(m("projection_half_deterministic") - m("projection_half_default") - ln["pose_sort"]["median_ms"] - ln["pose_sum"]["median_ms"], 4))
    kept = int(counts[1])
    keys = views["keys"][:kept].cpu().numpy()
    runs = np.diff(np.flatnonzero(np.concatenate(([True], keys[1:] != keys[:-1], [True]))))
    pk = views["pose_keys"][:int(counts[2])].cpu().numpy()
    pruns = np.diff(np.flatnonzero(np.concatenate(([True], pk[1:] != pk[:-1], [True])))) if len(pk) else np.zeros(1, np.int64)
    res["rows_per_destination"] = dict(contribution_slots_in_use=int(counts[0]), contributions=kept, gaussians_with_rows=int(len(runs)),
                                       median=float(np.median(runs)), maximum=int(runs.max()), mean=round(float(runs.mean()), 3),
                                       runs_longer_than_a_chunk=int((runs > L.SEG_CHUNK).sum()))
    res["pose_rows_per_actor"] = dict(points=int(counts[2]), actors_with_rows=int(len(pruns)), median=float(np.median(pruns)), maximum=int(pruns.max()))
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
