"""Cost of the deterministic MLP mode (mlp.level_mlp(deterministic=True), csrc/mlp_det.hip) on the reference configuration's
two levels at 2 M rows:
  coarse: 128 HexPlane features + the 4-value embedding -> trunk -> dx (3), do (1), dshs (48) heads and the two-hidden-layer feature head (3);
  fine:   the embedding alone (no HexPlane features) -> the same heads; the regulariser mean |out| on dx and dshs of both levels.
In ONE run per level: forward + backward with and without the mode (median of 30 between HIP events, min - max beside it, the two modes interleaved
in two halves); device time per kernel family from the profiler in both modes (the slab-storing kernels against the atomic ones, and the reduction
launches the mode adds); the slab bytes of a step.
    python profiles/mlp_deterministic_microbench.py [OUT.json]      -> profiles/mlp_deterministic_microbench.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from emd_amd import mlp  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

REPS, PASSES, N = 30, 3, 2_000_000
dev = torch.device("cuda", 0)
HEADS = [(True, 1, 3), (True, 1, 1), (True, 1, 48), (False, 2, 3)]
L1_HEADS = (0, 2)


def timed(step, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "reps": len(ms)}


def families(step):
    fams = {"head forward": ("k_mlp_branch_fwd",), "head backward": ("k_mlp_branch_bwd",), "trunk forward": ("k_mlp_trunk_fwd",),
            "trunk backward": ("k_mlp_trunk_bwd", "k_mlp_embed_bwd"), "reduce": ("k_mlp_det_reduce",)}
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        timed(step, PASSES)
    out = {k: {"ms": 0.0, "launches": 0} for k in fams}
    for ev in prof.key_averages():
        for fam, names in fams.items():
            if any(nm in ev.key for nm in names):
                dt = getattr(ev, "device_time_total", None)
                out[fam]["ms"] += (ev.cuda_time_total if dt is None else dt) / 1e3 / PASSES
                out[fam]["launches"] += ev.count // PASSES
    return {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in out.items()}


def level(ka):
    g = torch.Generator().manual_seed(ka + 1)
    P = lambda *s: (torch.randn(*s, generator=g) / (s[-1] ** 0.5)).to(dev).requires_grad_(True)
    ld = ka + 32 + 4
    w0, b = P(64, ld), P(64)
    branches = [(ri, [(P(64, 64), P(64)) for _ in range(depth)], (P(o, 64), P(o))) for ri, depth, o in HEADS]
    xa = torch.randn(N, ka, device=dev).requires_grad_(True) if ka else None
    xb = torch.randn(N, 4, device=dev).requires_grad_(True)
    gouts = [torch.randn(N, o, device=dev) for _, _, o in HEADS]
    leaves = ([xa] if ka else []) + [xb, w0, b] + [t for _, hid, (wo, bo) in branches for t in [x for wb in hid for x in wb] + [wo, bo]]
    mode = {"det": False}

    def step():
        outs = mlp.level_mlp(xa, xb, w0, b, 0, ka + 32, branches, l1_heads=L1_HEADS, deterministic=mode["det"])
        loss = sum((o * go).sum() for o, go in zip(outs, gouts)) + 0.01 * outs[len(HEADS)] + 0.01 * outs[len(HEADS) + 1]
        torch.autograd.grad(loss, leaves)
    samples = {"default": [], "deterministic": []}
    for m in (False, True, False, True):                    # both modes in two halves, interleaved: two warm-up passes, then the timed repetitions
        mode["det"] = m
        timed(step, 2)
        samples["deterministic" if m else "default"] += timed(step, REPS // 2)
    res = {k: summary(v) for k, v in samples.items()}
    res["op"] = (f"level_mlp forward + backward (outputs' products and sums included), {N} rows, ka = {ka}, kb = 4, heads {[o for _, _, o in HEADS]} "
                 f"(the last with two hidden layers), mean |out| folded in for heads {list(L1_HEADS)}")
    for m in (False, True):
        mode["det"] = m
        res["device_ms_per_kernel_family_" + ("deterministic" if m else "default")] = families(step)
    trace = []
    mlp.DET_TRACE, mode["det"] = trace, True
    step()
    torch.cuda.synchronize()
    mlp.DET_TRACE = None
    res["slab_bytes"] = {t["direction"]: int(t["slab"].numel()) for t in trace}
    res["reduce_jobs"] = {t["direction"]: len(t["jobs"]) for t in trace}
    res["workgroups_per_backward_kernel"] = max(j["groups"] for t in trace if t["direction"] == "backward" for j in t["jobs"])
    return res


res = {"coarse": level(128), "fine": level(0)}
for k in ("coarse", "fine"):
    d, a = res[k]["deterministic"], res[k]["default"]
    res[k]["cost_of_the_mode_ms"] = round(d["median_ms"] - a["median_ms"], 3)
    res[k]["spread_of_the_default_ms"] = round(a["max_ms"] - a["min_ms"], 3)
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "mlp_deterministic_microbench.json")
open(out, "w").write(json.dumps(res, indent=1) + "\n")
print(json.dumps(res))
