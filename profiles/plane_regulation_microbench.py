"""The HexPlane regularisers (csrc/plane_reg.hip) at the reference configuration -- 32 channels, resolution [64, 64, 64, 25], multires [1, 2, 4, 8]:
24 planes, 143 MB -- beside the yardstick: the same contract in the reference's formulation (tests/plane_reg_ref.py: per plane two slices, two
subtractions, a square and a mean, through autograd) in fp32 torch on the same GPU.

Clock: HIP events on the launch stream around ONE call (a forward, or a backward through a retained graph); `--warmup` untimed calls, then the
median of `--reps`.  The planes fit the 256 MiB Infinity Cache, so every figure is taken twice: `warm` (calls back to back: the planes may still be
on-die from the previous call) and `cold` (a device-to-device copy of 2 x 256 MiB on the same stream before each timed call, outside the event
pair: the planes come from HBM and the cache holds another kernel's lines, half of them dirty, as inside a training step that moves gigabytes
between two calls).  The copy peak is the same `copy_` timed the same way.  `--kernels-only N` runs N cold, then N warm forward + backward calls of the
entry points and nothing else, for a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/plane_regulation_microbench.py --kernels-only 20
(profiles/plane_regulation_kernel_trace.txt is the summary of such a run).  Bytes: what the algorithm has to move, from the shapes: forward the planes once,
backward the planes once and their gradients once.  The outputs of the timed code are compared with the yardstick's before anything is timed.
    python profiles/plane_regulation_microbench.py [--reps 30] [--out profiles/plane_regulation_microbench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emd_amd import _lib as L  # noqa: E402
from emd_amd import hexplane  # noqa: E402
from tests import plane_reg_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--resolution", type=int, nargs=4, default=[64, 64, 64, 25])
    ap.add_argument("--multires", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernels-only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "plane_regulation_microbench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plane_regulation_microbench needs a GPU: a CPU run gives no time")
    dev = "cuda:0"
    resolutions = [[r * m for r in a.resolution[:3]] + a.resolution[3:] for m in a.multires]
    grids = [[p.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for p in g]
             for g in R.make_grids(a.channels, resolutions, 0.05)]
    leaves = [p for g in grids for p in g]
    plane_bytes = 4 * sum(p.numel() for p in leaves)
    w = R.WEIGHTS
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

    def launches(fn):
        """Kernel launches of one call, from the profiler's device-side records; None where the profiler gives none."""
        try:
            from torch.profiler import ProfilerActivity, profile
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
            return n or None
        except Exception:
            return None

    def fwd_bwd(fn):
        loss = fn()
        back = lambda: torch.autograd.grad(loss, leaves, retain_graph=True)
        r = dict(forward=both(fn), backward=both(back), forward_launches=launches(fn), backward_launches=launches(back))
        return r, loss.detach(), back()

    hip = lambda: hexplane.plane_regulation(grids, **w)
    ref = lambda: R.compute_regulation(grids, **w)[0]
    res = dict(channels=a.channels, resolutions=resolutions, planes=len(leaves), plane_bytes=plane_bytes, reps=a.reps, warmup=a.warmup,
               segment_rows=L.PLANE_REG_SEG,
               clock="HIP events on the launch stream around one call; median of reps after warmup; cold = a 2 x 256 MiB copy before each timed call")
    # the entry points on their own
    lib, st = L.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = L.EmdPlaneRegArgs()
    args.channels, args.num_scales = a.channels, len(resolutions)
    args.time_smoothness_weight, args.l1_time_planes_weight, args.plane_tv_weight = (w[k] for k in ("time_smoothness_weight", "l1_time_planes_weight", "plane_tv_weight"))
    flat = torch.empty(plane_bytes // 4, device=dev)
    off = 0
    for s, r in enumerate(resolutions):
        for k in range(4):
            args.res[s][k] = r[k]
        for p in range(6):
            args.planes[s][p], args.dL_dplanes[s][p] = grids[s][p].data_ptr(), flat.data_ptr() + 4 * off
            off += grids[s][p].numel()
    out, gup = torch.empty(4, device=dev), torch.ones(1, device=dev)
    ws = torch.empty(lib.emd_plane_reg_workspace_size(C.byref(args)), dtype=torch.uint8, device=dev)
    args.out, args.g = out.data_ptr(), gup.data_ptr()
    res["workgroups"] = ws.numel() // 16
    kernels = dict(plane_reg_forward=lambda: L.check(lib.emd_plane_reg_forward(C.byref(args), ws.data_ptr(), ws.numel(), st), "fwd"),
                   plane_reg_backward=lambda: L.check(lib.emd_plane_reg_backward(C.byref(args), st), "bwd"))
    if a.kernels_only:
        for cold in (True, False):                    # the first N dispatches of every kernel are cold, the next N warm
            for _ in range(a.kernels_only):
                for fn in kernels.values():
                    if cold:
                        dst.copy_(src)
                    fn()
        torch.cuda.synchronize()
        return

    r_hip, l_hip, g_hip = fwd_bwd(hip)
    r_ref, l_ref, g_ref = fwd_bwd(ref)
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-300))
    res["relative_l2_vs_torch_fp32"] = dict(loss=rel(l_hip, l_ref), worst_plane_gradient=max(rel(x, y) for x, y in zip(g_hip, g_ref)))
    assert res["relative_l2_vs_torch_fp32"]["loss"] < 1e-5 and res["relative_l2_vs_torch_fp32"]["worst_plane_gradient"] < 1e-5
    res["hip_plane_regulation"] = r_hip
    res["torch_fp32_reference_formulation"] = r_ref
    res["entry_points"] = {k: both(fn) for k, fn in kernels.items()}
    assert torch.equal(out[0], l_hip)

    cp = timed(lambda: dst.copy_(src), False)
    peak = 2 * src.numel() / (cp["median_ms"] * 1e-3)
    res["copy_peak"] = dict(bytes=2 * src.numel(), **cp, bytes_per_s=round(peak))
    for k, nbytes in (("plane_reg_forward", plane_bytes), ("plane_reg_backward", 2 * plane_bytes)):
        for temp in ("warm", "cold"):
            t = res["entry_points"][k][temp]["median_ms"] * 1e-3
            res["entry_points"][k][temp].update(bytes=nbytes, bytes_per_s=round(nbytes / t), fraction_of_copy_peak=round(nbytes / t / peak, 3))
    tot = lambda r, temp: r["forward"][temp]["median_ms"] + r["backward"][temp]["median_ms"]
    res["forward_plus_backward_ms"] = {temp: dict(hip=round(tot(r_hip, temp), 4), torch=round(tot(r_ref, temp), 4)) for temp in ("warm", "cold")}
    res["hip_faster_than_torch"] = all(v["hip"] < v["torch"] for v in res["forward_plus_backward_ms"].values())
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
