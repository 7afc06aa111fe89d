"""Cost of the deterministic HexPlane backward (HexPlaneField.deterministic) at the configuration and the points of
profiles/bench_hexplane.py: 32 channels, resolution [64,64,64,25], multires [1,2,4,8], 2 M uniformly random points in the box, one shared time.
In ONE run: the backward with and without the mode (median of 30 between HIP events, min - max beside it); the added launches on their own (row
kernel, sort, sum: device time per kernel family from the profiler, summed over the 24 planes); the workspace bytes; the run-length statistics of
the per-texel lists (from the sorted keys the call leaves in its workspace, plane by plane).
    python profiles/hexplane_deterministic_microbench.py [N]      -> profiles/hexplane_deterministic_microbench.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from emd_amd import _lib as L  # noqa: E402
from emd_amd.hexplane import HexPlaneField  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
REPS = 30
dev = torch.device("cuda", 0)
cfg = {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32, "resolution": [64, 64, 64, 25]}
field = HexPlaneField(1.6, cfg, [1, 2, 4, 8]).to(dev)
g = torch.Generator().manual_seed(0)
pts = ((torch.rand(N, 3, generator=g) * 3.2) - 1.6).to(dev).requires_grad_(True)
t = torch.full((N, 1), 0.37, device=dev)                    # one frame per step: every point carries the same time
gout = torch.randn(N, 128, generator=g).to(dev)


def backward_ms(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        pts.grad = None
        for p in field.parameters():
            p.grad = None
        f = field(pts, t)
        e0.record()
        f.backward(gout)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "reps": len(ms)}


res = {"op": "HexPlane backward, 4 scales x 6 planes x 32 channels (planes + points), default against deterministic", "N": N}
samples = {"default": [], "deterministic": []}
for mode in (False, True, False, True):                     # both modes in two halves, interleaved: two warm-up passes, then the timed repetitions
    field.deterministic = mode
    backward_ms(2)
    samples["deterministic" if mode else "default"] += backward_ms(REPS // 2)
for key, ms in samples.items():
    res[key] = summary(ms)

# ---- the added launches on their own: device time per kernel family over three deterministic backward passes
field.deterministic = True
from torch.profiler import ProfilerActivity, profile  # noqa: E402
PASSES = 3
fams = {"row kernel": ("k_hexplane_det_rows",), "sort": ("k_radix_",), "sum": ("k_segsum_",), "per-point pass": ("k_hexplane_det_points",)}
with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
    backward_ms(PASSES)
launches = {k: {"ms": 0.0, "launches": 0} for k in fams}
for ev in prof.key_averages():
    for fam, names in fams.items():
        if any(nm in ev.key for nm in names):
            dt = getattr(ev, "device_time_total", None)
            launches[fam]["ms"] += (ev.cuda_time_total if dt is None else dt) / 1e3 / PASSES
            launches[fam]["launches"] += ev.count // PASSES
res["added_launches_per_backward"] = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in launches.items()}

# ---- workspace and the per-texel lists
a = L.EmdHexArgs()
a.num_points, a.channels, a.num_scales = N, 32, 4
res["workspace_bytes"] = L.hex_det_workspace_size(a)
res["rows_bytes_per_plane"] = 16 * N * 32
lengths, per_plane = [], []
for s in range(4):
    for p in range(6):
        field.det_keep_plane = (s, p)
        backward_ms(1)
        keys = field.det_state["keys"]
        cnt = torch.unique_consecutive(keys, return_counts=True)[1]
        lengths.append(cnt)
        per_plane.append({"scale": s, "plane": p, "sort_passes": field.det_state["passes"], "runs": int(cnt.numel()), "median": float(cnt.median()),
                          "max": int(cnt.max()), "longer_than_a_chunk": int((cnt > L.SEG_CHUNK).sum())})
allc = torch.cat(lengths).double()
res["run_lengths"] = {"runs": int(allc.numel()), "median": float(allc.median()), "mean": round(float(allc.mean()), 2), "max": int(allc.max()),
                      "longer_than_a_chunk": int((allc > L.SEG_CHUNK).sum()), "chunk": L.SEG_CHUNK, "per_plane": per_plane}
out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hexplane_deterministic_microbench.json")
open(out, "w").write(json.dumps(res, indent=1) + "\n")
print(json.dumps({k: v for k, v in res.items() if k != "run_lengths"}))
print(json.dumps({k: v for k, v in res["run_lengths"].items() if k != "per_plane"}))
