"""The image tail of an OmniRe step (csrc/trainer_loss.hip: apply_affine -> trainer_losses, every term on) at 1066 x 1600, forward + backward
through autograd, beside the yardstick: the same formulas (tests/trainer_loss_ref.py, the test reference moved to the device) in fp32 torch
through autograd on the same GPU.

Clocks.  Whole calls: HIP events on the launch stream around ONE forward + backward; `--warmup` untimed calls, then the median of `--reps`, taken
`warm` (calls back to back) and `cold` (a device-to-device copy of 2 x 256 MiB on the same stream before each timed call, outside the event pair, as
inside a training step that moves gigabytes between two calls).  The entry points on their own (emd_trainer_loss, emd_affine_forward,
emd_affine_backward): the same clock.  Single kernels: the device-side records of torch.profiler over `--reps` warm calls, median per kernel name
(events cannot be placed between the launches of one entry point), in a pass of its own after the timed ones.  Bytes: what each kernel has to move,
from the shapes (below); the copy peak is the same `copy_` timed with the events.  The outputs of the timed code are compared with the yardstick's
before anything is timed.
    python profiles/trainer_loss_microbench.py [--reps 30] [--out profiles/trainer_loss_microbench.json]"""
import argparse
import collections
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emd_amd import _lib as L  # noqa: E402
from emd_amd import trainer_loss as TL  # noqa: E402
from tests import trainer_loss_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1066)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "trainer_loss_microbench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trainer_loss_microbench needs a GPU: a CPU run gives no time")
    dev, H, W = "cuda:0", a.height, a.width
    P, PM = H * W, (H - 10) * (W - 10)
    c = {k: v.to(dev) for k, v in R.make_inputs(H, W, seed=0).items()}
    A = (torch.eye(3, 4) + 0.05 * torch.randn(3, 4, generator=torch.Generator().manual_seed(1))).to(dev).requires_grad_(True)
    x, o, d = (c[k].clone().requires_grad_(True) for k in ("x", "o", "d"))
    leaves = [x, o, d, A]
    cfg = R.config(mask_type="safe_bce")
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def timed(fn, cold):
        ts = []
        for _ in range(a.warmup + a.reps):
            if cold:
                dst.copy_(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = sorted(ts[a.warmup:])
        return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4))

    both = lambda fn: dict(warm=timed(fn, False), cold=timed(fn, True))

    def device_records(fn, reps):
        """{kernel name: [device durations in us]} of `reps` calls, from the profiler's device-side records; None where the profiler gives none."""
        try:
            from torch.profiler import ProfilerActivity, profile
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
            rec = collections.defaultdict(list)
            for e in prof.events():
                if str(e.device_type).endswith("CUDA"):
                    rec[e.name].append(e.device_time)
            return dict(rec) or None
        except Exception:
            return None

    def hip_step():
        loss, _ = TL.trainer_losses(TL.apply_affine(x, A), c["y"], o, c["s"], d, c["l"], **cfg)
        return loss, torch.autograd.grad(loss, leaves)

    def torch_step():
        loss, _ = R.losses(x @ A[:, :3].T + A[:, 3], c["y"], o, c["s"], d, c["l"], cfg)
        return loss, torch.autograd.grad(loss, leaves)

    l_hip, g_hip = hip_step()
    l_ref, g_ref = torch_step()
    worst = lambda p, q: float((p.double() - q.double()).abs().max() / q.double().abs().max())
    res = dict(height=H, width=W, reps=a.reps, warmup=a.warmup, chunk_pixels=L.TRAINER_LOSS_CHUNK, ssim_tile=L.TRAINER_SSIM_TILE, terms="all six, safe_bce",
               clock="HIP events on the launch stream around one forward + backward; median of reps after warmup; cold = a 2 x 256 MiB copy before each "
                     "timed call; single kernels from torch.profiler's device-side records of warm calls")
    res["difference_vs_torch_fp32"] = dict(loss=abs(float(l_hip) - float(l_ref)),
                                           worst_gradient_error_over_largest_entry={k: worst(p, q) for k, p, q in zip(("rgb", "opacity", "depth", "affine"), g_hip, g_ref)})
    assert res["difference_vs_torch_fp32"]["loss"] < 1e-5 and max(res["difference_vs_torch_fp32"]["worst_gradient_error_over_largest_entry"].values()) < 1e-3
    res["hip_forward_plus_backward"] = both(hip_step)
    res["torch_fp32_same_formulas_forward_plus_backward"] = both(torch_step)

    # the entry points on their own
    lib, st = L.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    t = L.EmdTrainerLossArgs()
    t.height, t.width, t.mask_type = H, W, L.TL_MASK_SAFE_BCE
    xc = TL.apply_affine(x, A).detach()
    t.rgb, t.gt_rgb, t.opacity, t.sky_mask, t.depth, t.lidar_depth = xc.data_ptr(), c["y"].data_ptr(), o.data_ptr(), c["s"].data_ptr(), d.data_ptr(), c["l"].data_ptr()
    for k in ("w_rgb", "w_ssim", "w_mask", "safe_limit", "w_depth", "upper_bound", "w_entropy", "w_smooth"):
        setattr(t, k, cfg[k])
    out7, g3, g1a, g1b = torch.empty(7, device=dev), torch.empty(P * 3, device=dev), torch.empty(P, device=dev), torch.empty(P, device=dev)
    t.losses, t.dL_drgb, t.dL_dopacity, t.dL_ddepth = out7.data_ptr(), g3.data_ptr(), g1a.data_ptr(), g1b.data_ptr()
    ws = torch.empty(lib.emd_trainer_loss_workspace_size(C.byref(t)), dtype=torch.uint8, device=dev)
    aws = torch.empty(lib.emd_affine_workspace_size(P), dtype=torch.uint8, device=dev)
    dA, Ad, xd = torch.empty(12, device=dev), A.detach(), x.detach()
    entries = dict(
        emd_trainer_loss=lambda: L.check(lib.emd_trainer_loss(C.byref(t), ws.data_ptr(), ws.numel(), st), "loss"),
        emd_affine_forward=lambda: L.check(lib.emd_affine_forward(P, xd.data_ptr(), Ad.data_ptr(), g3.data_ptr(), st), "affine forward"),
        emd_affine_backward=lambda: L.check(lib.emd_affine_backward(P, xd.data_ptr(), Ad.data_ptr(), xc.data_ptr(), g3.data_ptr(), dA.data_ptr(),
                                                                     aws.data_ptr(), aws.numel(), st), "affine backward"))
    res["entry_points"] = {k: both(fn) for k, fn in entries.items()}
    res["workspace_bytes"] = dict(trainer_loss=ws.numel(), affine_backward=aws.numel())

    cp = timed(lambda: dst.copy_(src), False)
    peak = 2 * src.numel() / (cp["median_ms"] * 1e-3)
    res["copy_peak"] = dict(bytes=2 * src.numel(), **cp, bytes_per_s=round(peak))

    # what each kernel has to move (a neighbour's value read again by the next pixel is served on-die and not counted)
    need = dict(k_tl_pointwise=(24 + 16 + 4) * P,                  # x, y; o, s, d, l; dL/dopacity
                k_tl_ssim_forward=24 * P + 36 * PM,               # x, y; three derivative maps of 3 (H-10) (W-10) floats
                k_tl_ssim_backward=36 * PM + 24 * P + 12 * P,     # the maps; x, y; dL/drgb
                k_tl_finalize=ws.numel() - 36 * PM,               # the partials
                k_tl_depth_grad=(4 + 4 + 4 + 12 + 4) * P,         # d, l, s, y; dL/ddepth
                k_affine_forward=24 * P,
                k_affine_backward=(12 + 12 + 12) * P,             # g, x; dL/drgb
                k_affine_finalize=aws.numel())
    rec = device_records(lambda: hip_step(), a.reps)
    kernels, hip_launches = {}, None
    if rec:
        hip_launches = sum(len(v) for v in rec.values()) // a.reps
        for name, us in rec.items():
            key = next((k for k in need if k in name), None)
            if key is None:
                kernels.setdefault("other (torch: the upstream scaling, clones)", dict(launches_per_call=0, median_us_each=[]))
                kernels["other (torch: the upstream scaling, clones)"]["launches_per_call"] += len(us) / a.reps
                kernels["other (torch: the upstream scaling, clones)"]["median_us_each"].append(round(sorted(us)[len(us) // 2], 2))
                continue
            med = sorted(us)[len(us) // 2]
            kernels[key] = dict(launches_per_call=len(us) / a.reps, median_us=round(med, 2), bytes=need[key], bytes_per_s=round(need[key] / (med * 1e-6)),
                                fraction_of_copy_peak=round(need[key] / (med * 1e-6) / peak, 3))
    res["kernels_warm_from_profiler"] = kernels or "not measured: the profiler gave no device records"
    rec_t = device_records(lambda: torch_step(), 3)
    res["launches_per_forward_plus_backward"] = dict(hip=hip_launches, torch=(sum(len(v) for v in rec_t.values()) // 3) if rec_t else None)
    res["launches_inside_emd_trainer_loss"] = 5
    med = lambda r, temp: r[temp]["median_ms"]
    res["forward_plus_backward_ms"] = {temp: dict(hip=med(res["hip_forward_plus_backward"], temp), torch=med(res["torch_fp32_same_formulas_forward_plus_backward"], temp))
                                       for temp in ("warm", "cold")}
    res["hip_faster_than_torch"] = all(v["hip"] < v["torch"] for v in res["forward_plus_backward_ms"].values())
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
