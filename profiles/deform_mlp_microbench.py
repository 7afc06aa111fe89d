"""OmniRe's ConditionalDeformNetwork behind DeformableNodes, fused (csrc/deform_mlp.hip) against the default rocBLAS layers, at
the bench scene's actor share: 32 actors x 5 000 points = 160 000 rows, D = 8, W = 256, E = 10 (C_in = 94).
In ONE run: forward + backward of nonrigid_deformation through autograd with fused=True and fused=False (median of 30 after 5 between HIP events, min -
max beside it, the two interleaved in two halves; warm = back to back, cold = a 512 MiB buffer rewritten before every repetition so that neither the
Infinity Cache nor L2 holds the step's data); device time per new kernel from the profiler's records; the work from the shapes against the fp32-MFMA
peak (157.3 TFLOP/s: a floor from the instruction rate, not a time anyone measured); the slab bytes.
On a tree without `fused` (the parent commit) the script measures the default path alone: that is the parent's figure.
    python profiles/deform_mlp_microbench.py [OUT.json]      -> profiles/deform_mlp_microbench.json"""
import inspect
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from emd_amd import _lib as L  # noqa: E402
from emd_amd import deformation  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

REPS, WARMUP, PASSES = 30, 5, 3
ACTORS, PER_ACTOR, D, W, E, LX, LT = 32, 5000, 8, 256, 10, 10, 10
N = ACTORS * PER_ACTOR
PEAK = 157.3e12
dev = torch.device("cuda", 0)
HAS_FUSED = "fused" in inspect.signature(deformation.ConditionalDeformNetwork.__init__).parameters
flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)


def timed(step, reps, cold=False):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        if cold:
            flush.add_(1)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "reps": len(ms)}


def kernels(step):
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        timed(step, PASSES)
    out = {}
    for ev in prof.key_averages():
        if "k_deform_" in ev.key or "Cijk" in ev.key or "gemm" in ev.key.lower():
            dt = getattr(ev, "device_time_total", None)
            out[ev.key[:120]] = {"ms_per_step": round((ev.cuda_time_total if dt is None else dt) / 1e3 / PASSES, 4), "launches_per_step": ev.count // PASSES}
    return out


torch.manual_seed(0)
net = deformation.ConditionalDeformNetwork(D=D, W=W, embed_dim=E, x_multires=LX, t_multires=LT).to(dev)
with torch.no_grad():
    for head in (net.gaussian_warp, net.gaussian_rotation, net.gaussian_scaling):
        head.weight.normal_(0, 0.1)
g = torch.Generator().manual_seed(1)
means = (torch.rand(N, 3, generator=g) - 0.5).to(dev)
ids = torch.arange(ACTORS).repeat_interleave(PER_ACTOR)[torch.randperm(N, generator=g)].to(dev)[:, None]
size = (torch.rand(ACTORS, 3, generator=g) + 1.0).to(dev)
emb = torch.randn(ACTORS, E, generator=g).to(dev).requires_grad_(True)
t = torch.tensor([0.4], device=dev)
gouts = [torch.randn(N, w, generator=g).to(dev) for w in (3, 4, 3)]
leaves = [emb] + list(net.parameters())


def step():
    outs = deformation.nonrigid_deformation(net, means, ids, size, emb, t, deterministic=True)
    return torch.autograd.grad(sum((o * go).sum() for o, go in zip(outs, gouts)), leaves)


modes = (False, True) if HAS_FUSED else (False,)
samples = {(m, c): [] for m in modes for c in (False, True)}
for m in modes * 2:                                             # the modes in two halves, interleaved
    net.fused = m
    timed(step, WARMUP)
    for cold in (False, True):
        samples[m, cold] += timed(step, REPS // 2, cold)
C_in = net.input_ch
k_sum = C_in + (C_in + W) + (D - 2) * W                         # the layers' input widths
flop_fwd = 2 * N * W * k_sum + 2 * N * 10 * W
flop_bwd_w = flop_fwd
flop_bwd_x = 2 * N * W * ((D - 1) * W + 2 * E) + 2 * N * 10 * W
flop = flop_fwd + flop_bwd_w + flop_bwd_x
res = {"op": f"nonrigid_deformation forward + backward through autograd (encoder input, network, the outputs' products and sums), {N} rows = {ACTORS} actors x "
             f"{PER_ACTOR} points, D = {D}, W = {W}, E = {E}, C_in = {C_in}, deterministic=True",
       "flop_per_row": flop // N, "mfma_fp32_floor_ms": round(flop / PEAK * 1e3, 3)}
for m in modes:
    key = "fused" if m else "default_rocblas"
    res[key] = {"warm": summary(samples[m, False]), "cold": summary(samples[m, True])}
    res[key]["share_of_fp32_mfma_peak_warm"] = round(flop / PEAK * 1e3 / res[key]["warm"]["median_ms"], 3)
    net.fused = m
    res[key]["device_ms_per_kernel"] = kernels(step)
if HAS_FUSED:
    lay = L.deform_mlp_layout(N, W, C_in, torch.cuda.get_device_properties(dev).multi_processor_count)
    res["slab"] = lay
    # the same bits from both halves of the run is tests/test_deform_mlp_gpu.py's business; here: the two paths agree to fp32 accuracy at this size
    net.fused = True
    a = [x.clone() for x in step()]
    net.fused = False
    b = step()
    res["largest_gradient_difference_fused_vs_default_over_largest_entry"] = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(a, b))
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "deform_mlp_microbench.json")
open(out, "w").write(json.dumps(res, indent=1) + "\n")
print(json.dumps(res))
