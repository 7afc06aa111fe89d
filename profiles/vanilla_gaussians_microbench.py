"""VanillaGaussians' per-class dictionary and regularisers (csrc/vanilla.hip) at N = 2 M, M = 16, beside today's formulation on the same GPU, in the
same process, alternating call by call:
  dictionary   `nodes.vanilla_gaussians` (one launch each way) against `nodes._colors` plus the three torch activations, which is what the code base
               offered for this class before: torch.cat of the coefficients, the view directions, `emd_sh_forward`, + 0.5, clamp, exp, sigmoid, norm / div
  regularisers `vanilla.gaussian_regulation` against the reference's expressions in fp32 torch (amax / amin, min, max, the entropy over the visible
               rows written without the reference's host read)
at the active degrees n = 0 and n = 3, forward alone and forward + backward (`torch.autograd.grad` with the upstream gradients given: no loss ops).

Clock: HIP events on the launch stream around ONE call; `--warmup` untimed calls, then the median of `--reps`.  Every figure is taken `warm` (calls
back to back) and `cold` (a device-to-device copy of 2 x 256 MiB on the same stream before each timed call, outside the event pair, as
profiles/trainer_loss_microbench.py does).  The copy peak is that copy timed the same way.  Bytes: what each kernel has to move, from the shapes.
Launch counts of today's formulation: the kernel events of torch.profiler around one call.  The outputs of both sides are compared before anything
is timed.  `--kernels-only N` runs N cold calls of each fused path and nothing else, for a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/vanilla_gaussians_microbench.py --kernels-only 20
`--merge A B` writes A with B's medians beside it as the repeat and the spread between the two runs of the same command.
`--kernel-stats FILE` reads the kernel_stats CSV of that trace (lines before its header row are skipped) and adds to the JSON at --out the mean time,
the bytes and the share of the copy peak of each kernel, and whether the condition holds: both fused paths faster than today's formulation by more
than the spread, judged row by row as the slowest fused median of either run against the fastest median of today's formulation.
    python profiles/vanilla_gaussians_microbench.py [--reps 30] [--out profiles/vanilla_gaussians_microbench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emd_amd import nodes, vanilla  # noqa: E402

W = dict(w_sharp=0.7, max_gauss_ratio=10.0, w_flatten=0.3, w_sparse=0.05, w_max_s_square=1.3)
INTERVAL = 1000


def today_dictionary(p, step):
    rgbs = nodes._colors(p["means"], p["features_dc"], p["features_rest"], p["camera_center"], 3, step, INTERVAL)
    q = p["quats"]
    return torch.sigmoid(p["opacity_logits"]), torch.exp(p["log_scales"]), q / q.norm(dim=-1, keepdim=True), rgbs


def fused_dictionary(p, step):
    gs = nodes.vanilla_gaussians(p["means"], p["quats"], p["opacity_logits"], p["log_scales"], p["features_dc"], p["features_rest"], p["camera_center"],
                                 sh_degree=3, step=step, sh_degree_interval=INTERVAL, check_finite=False)
    return gs["_opacities"], gs["_scales"], gs["_quats"], gs["_rgbs"]


def today_regulation(l, a, radii):
    s = torch.exp(l)
    R = W["max_gauss_ratio"]
    sharp = W["w_sharp"] * (torch.clamp_min(s.amax(dim=-1) / s.amin(dim=-1), R) - R).mean()
    flatten = W["w_flatten"] * torch.abs(torch.clamp(torch.min(s, dim=1).values, 0, 30)).mean()
    msq = W["w_max_s_square"] * torch.mean(torch.max(s, dim=1).values ** 2)
    vis = (radii > 0).float()
    o = torch.clamp(torch.sigmoid(a.reshape(-1)), 1e-6, 1 - 1e-6)
    sparse = W["w_sparse"] * ((-(o * torch.log(o) + (1 - o) * torch.log(1 - o))) * vis).sum() / vis.sum().clamp_min(1.0)
    return torch.stack([sharp, flatten, sparse, msq])


def fused_regulation(l, a, radii):
    return vanilla.gaussian_regulation(l, a, radii, **W)


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if "cuda" in str(e.device_type).lower() and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as exc:  # noqa: BLE001
        return f"not measured ({type(exc).__name__})"


def merge(a_path, b_path, out):
    A, B = json.load(open(a_path)), json.load(open(b_path))
    spread = 0.0

    def walk(x, y):
        nonlocal spread
        for k, v in x.items():
            if isinstance(v, dict) and k in y:
                if "median_ms" in v and "median_ms" in y[k]:
                    v["repeat_median_ms"] = y[k]["median_ms"]
                    spread = max(spread, abs(v["median_ms"] - y[k]["median_ms"]) / v["median_ms"])
                else:
                    walk(v, y[k])
    walk(A["results"], B["results"])
    A["spread_between_two_runs_of_the_same_command"] = round(spread, 4)
    json.dump(A, open(out, "w"), indent=1)
    print(json.dumps({"spread": spread}))


KERNELS = (("k_vanilla_forward<3", "dictionary_n3", "bytes_forward"), ("k_vanilla_backward<3", "dictionary_n3", "bytes_backward"),
           ("k_vanilla_forward<0", "dictionary_n0", "bytes_forward"), ("k_vanilla_backward<0", "dictionary_n0", "bytes_backward"),
           ("k_vanilla_reg_forward", None, 20), ("k_vanilla_reg_finalize", None, None), ("k_vanilla_reg_backward", None, 36))


def kernel_stats(csv_path, out):
    import csv
    A = json.load(open(out))
    lines = open(csv_path).read().splitlines()
    rows = list(csv.DictReader(lines[next(i for i, l in enumerate(lines) if l.startswith('"Name"')):]))
    kernels = {}
    for key, res, b in KERNELS:
        row = next((r for r in rows if key in r["Name"]), None)
        if row is None:
            kernels[key] = "not measured"
            continue
        nbytes = A["results"][res][b] if res else (b * A["points"] if b else None)
        us = float(row["AverageNs"]) / 1e3
        kernels[key] = dict(calls=int(row["Calls"]), mean_us=round(us, 2), bytes=nbytes,
                            share_of_copy_peak=round(nbytes / (us * 1e-6) / A["copy_peak_bytes_per_s"], 3) if nbytes else None)
    A["kernel_trace"] = dict(source=f"a separate rocprofv3 --kernel-trace --stats run of --kernels-only ({os.path.basename(csv_path)}): mean over its cold calls",
                             kernels=kernels)
    worst = None

    def walk(x, where):
        nonlocal worst
        for k, v in x.items():
            if isinstance(v, dict) and "fused" in v and "today" in v:
                both = lambda d: [d["median_ms"]] + ([d["repeat_median_ms"]] if "repeat_median_ms" in d else [])
                margin = min(both(v["today"])) / max(both(v["fused"]))
                if worst is None or margin < worst[0]:
                    worst = (margin, f"{where} {k}".strip())
            elif isinstance(v, dict):
                walk(v, f"{where} {k}".strip())
    walk(A["results"], "")
    A["condition"] = dict(what="both fused paths faster than today's formulation by more than the spread between two runs of the same command, at both "
                               "degrees; row by row: the fastest median of today's formulation over the slowest fused median, either run",
                          holds=bool(worst[0] > 1.0), smallest_margin=round(worst[0], 3), smallest_margin_at=worst[1])
    json.dump(A, open(out, "w"), indent=1)
    print(json.dumps(A["condition"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernels-only", type=int, default=0)
    ap.add_argument("--merge", nargs=2)
    ap.add_argument("--kernel-stats")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "vanilla_gaussians_microbench.json"))
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge[0], a.merge[1], a.out)
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out)
    if not torch.cuda.is_available():
        raise SystemExit("vanilla_gaussians_microbench needs a GPU: a CPU run gives no time")
    dev, N = "cuda:0", a.points
    g = torch.Generator().manual_seed(0)
    n = lambda *s: torch.randn(*s, generator=g)
    leaf = lambda t: t.to(dev).requires_grad_(True)
    p = dict(means=(0.5 * n(N, 3)).to(dev), quats=leaf(n(N, 4)), opacity_logits=leaf(n(N, 1)), log_scales=leaf(0.9 * n(N, 3) - 1.0), features_dc=leaf(n(N, 3)),
             features_rest=leaf(0.3 * n(N, 15, 3)), camera_center=torch.tensor([4.0, -3.0, 3.5], device=dev))
    leaves = [p[k] for k in ("quats", "opacity_logits", "log_scales", "features_dc", "features_rest")]
    ups = [n(N, 1).to(dev), n(N, 3).to(dev), n(N, 4).to(dev), n(N, 3).to(dev)]
    radii = (torch.randint(1, 40, (N,), generator=g) * (torch.rand(N, generator=g) < 0.6)).to(torch.int32).to(dev)
    up4 = torch.tensor([0.37, 1.0, -2.0, 0.5], device=dev)
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def dict_fb(fn, step):
        return lambda: torch.autograd.grad(fn(p, step), leaves, ups, allow_unused=True)

    def reg_fb(fn):
        return lambda: torch.autograd.grad(fn(p["log_scales"], p["opacity_logits"], radii), (p["log_scales"], p["opacity_logits"]), up4)

    if a.kernels_only:
        for _ in range(a.kernels_only):
            for step in (0, 3000):
                dst.copy_(src)
                dict_fb(fused_dictionary, step)()
            dst.copy_(src)
            reg_fb(fused_regulation)()
        torch.cuda.synchronize()
        return

    # the two sides agree before anything is timed
    for step in (0, 3000):
        with torch.no_grad():
            for x, y in zip(fused_dictionary(p, step), today_dictionary(p, step)):
                assert torch.allclose(x.reshape(y.shape), y, rtol=1e-5, atol=1e-6), step
        for x, y in zip(dict_fb(fused_dictionary, step)(), dict_fb(today_dictionary, step)()):
            assert x is not None and y is not None and torch.allclose(x, y, rtol=1e-4, atol=1e-6), step
    assert torch.allclose(fused_regulation(p["log_scales"], p["opacity_logits"], radii), today_regulation(p["log_scales"], p["opacity_logits"], radii), rtol=1e-4)
    for x, y in zip(reg_fb(fused_regulation)(), reg_fb(today_regulation)()):
        assert torch.allclose(x, y, rtol=1e-3, atol=1e-9)

    def pair(fa, fb, cold):
        """fa and fb alternating, call by call -> their two lists of times."""
        ta, tb = [], []
        for _ in range(a.warmup + a.reps):
            for fn, ts in ((fa, ta), (fb, tb)):
                if cold:
                    dst.copy_(src)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
        stat = lambda ts: dict(median_ms=round(statistics.median(ts[a.warmup:]), 5), min_ms=round(min(ts[a.warmup:]), 5), max_ms=round(max(ts[a.warmup:]), 5))
        return stat(ta), stat(tb)

    def both(fa, fb):
        out = {}
        for temp, cold in (("warm", False), ("cold", True)):
            sa, sb = pair(fa, fb, cold)
            out[temp] = dict(fused=sa, today=sb, today_over_fused=round(sb["median_ms"] / sa["median_ms"], 3))
        return out

    copy_ts = []
    for _ in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        copy_ts.append(e0.elapsed_time(e1))
    copy_ms = statistics.median(copy_ts[a.warmup:])
    peak = 2 * src.numel() / (copy_ms * 1e-3)

    results = {}
    for step, deg in ((0, 0), (3000, 3)):
        K3 = 3 * ((deg + 1) ** 2 - 1) * 4
        fwd_bytes = N * (12 + 16 + 4 + 12 + (12 if deg else 0) + K3 + 44 + 1)
        bwd_bytes = N * (12 + 16 + 4 + (12 if deg else 0) + 1 + 44 + 4 + 12 + 16 + 12 + 180)
        with torch.no_grad():
            fwd = both(lambda: fused_dictionary(p, step), lambda: today_dictionary(p, step))
        fb = both(dict_fb(fused_dictionary, step), dict_fb(today_dictionary, step))
        for r, b in ((fwd, fwd_bytes), (fb, fwd_bytes + bwd_bytes)):
            for temp in ("warm", "cold"):
                r[temp]["fused_share_of_copy_peak"] = round(b / (r[temp]["fused"]["median_ms"] * 1e-3) / peak, 3)
        with torch.no_grad():
            n_fwd = launches(lambda: today_dictionary(p, step))
        results[f"dictionary_n{deg}"] = dict(forward=fwd, forward_backward=fb, bytes_forward=fwd_bytes, bytes_backward=bwd_bytes,
                                             today_launches_forward=n_fwd, today_launches_forward_backward=launches(dict_fb(today_dictionary, step)),
                                             fused_launches_forward=1, fused_launches_backward=1)
    reg = both(reg_fb(fused_regulation), reg_fb(today_regulation))
    reg_bytes = N * (20 + 20 + 16)
    for temp in ("warm", "cold"):
        reg[temp]["fused_share_of_copy_peak"] = round(reg_bytes / (reg[temp]["fused"]["median_ms"] * 1e-3) / peak, 3)
    results["regularisers"] = dict(forward_backward=reg, bytes_forward_backward=reg_bytes, today_launches_forward_backward=launches(reg_fb(today_regulation)),
                                   fused_launches_forward=2, fused_launches_backward=1)
    out = dict(what="VanillaGaussians: per-class dictionary and regularisers, fused HIP against today's formulation (profiles/vanilla_gaussians_microbench.py)",
               device=torch.cuda.get_device_name(0), points=N, sh_coeffs=16, reps=a.reps, warmup=a.warmup,
               clock="HIP events on the launch stream around one call; median of reps after warmup; both sides alternate call by call; cold = a 2 x 256 MiB "
                     "copy before each timed call, outside the event pair",
               copy_peak_bytes_per_s=round(peak), copy_ms=round(copy_ms, 5),
               nontemporal_hint="not measured: the kernels use plain loads and stores",
               degrees_not_measured="n = 1 and n = 2 (at M = 16 they gather the first 9 or 24 floats of each 45-float record as dwords, not dwordx4)",
               results=results)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps({k: {m: {t: v[m][t]["today_over_fused"] for t in ("warm", "cold")} for m in v if m.startswith("forward")} for k, v in results.items()}))


if __name__ == "__main__":
    main()
