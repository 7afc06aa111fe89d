"""Cost of the deterministic actor chain (TrackOffsetHeads.deterministic, csrc/track_det.hip) at the benchmark's size:
32 actors x 5 000 points, temporal tables 150 x 32, 4-wide embeddings.
  chain:    the one-launch chain (pose_table) forward + backward with and without the mode;
  row sum:  emd_actor_row_sum_det against the atomic k_deform_input_bwd (emd_deform_input_backward with its zero fill) at 160 k points x 10 columns,
            ids sorted by actor and interleaved.
In ONE run: both modes interleaved in two halves, median of 30 between HIP events, min - max beside it; the workspace bytes of each call.
    python profiles/track_deterministic_microbench.py [OUT.json]      -> profiles/track_deterministic_microbench.json"""
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from emd_amd import _lib as L  # noqa: E402
from emd_amd import motion  # noqa: E402

REPS = 30
dev = torch.device("cuda", 0)


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
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def interleaved(steps):
    """steps: {"default": f, "deterministic": f} -> summaries; both modes in two halves, two warm-up passes in front of each half"""
    samples = {k: [] for k in steps}
    for k in ("default", "deterministic", "default", "deterministic"):
        timed(steps[k], 2)
        samples[k] += timed(steps[k], REPS // 2)
    res = {k: summary(v) for k, v in samples.items()}
    res["cost_of_the_mode_ms"] = round(res["deterministic"]["median_ms"] - res["default"]["median_ms"], 4)
    res["spread_of_the_default_ms"] = round(res["default"]["max_ms"] - res["default"]["min_ms"], 4)
    return res


def chain():
    A, P, F_, rows, fdim, E = 32, 5000, 50, 150, 32, 4
    g = torch.Generator().manual_seed(7)
    heads = motion.TrackOffsetHeads(A, temporal_embedding_dim=fdim, gaussian_embedding_dim=E, max_embeddings=rows)
    with torch.no_grad():
        for lin, sc in ((heads.track_trans_c, 0.05), (heads.track_trans_f, 0.05), (heads.track_rot_c, 0.01), (heads.track_rot_f, 0.01)):
            lin.weight.copy_(sc * torch.randn(lin.weight.shape, generator=g))
    heads = heads.to(dev)
    ids = torch.repeat_interleave(torch.arange(A), P).to(dev)
    emb = (0.1 * torch.randn(A * P, E, generator=g)).to(dev).requires_grad_(True)
    iq, it = torch.randn(F_, A, 4, generator=g).to(dev).requires_grad_(True), torch.randn(F_, A, 3, generator=g).to(dev).requires_grad_(True)
    fv = torch.ones(F_, A, dtype=torch.bool, device=dev)
    w = torch.randn(A, 12, generator=g).to(dev)
    leaves = [emb, iq, it] + list(heads.parameters())

    def make(det):
        def step():
            heads.deterministic = det
            pose = heads.pose_table(iq, it, fv, 20, emb, ids, 12000)
            torch.autograd.grad((pose * w).sum(), leaves)
        return step
    res = interleaved({"default": make(False), "deterministic": make(True)})
    res["op"] = (f"TrackOffsetHeads.pose_table forward + backward (the product with the pose gradient included), {A} actors x {P} points, tables {rows} x {fdim}, "
                 f"E = {E}, {F_} frames")
    res["workspace_bytes"] = L.track_det_workspace_size(A, fdim + E)
    res["launches"] = {"default": "k_tracked_pose<false>, k_tracked_pose<true>",
                       "deterministic": "k_tracked_pose<false>, k_track_chain_bwd_det<true>, k_head_slab_reduce"}
    return res


def row_sum(sorted_ids):
    n, A, E, col0 = 160_000, 32, 10, 84
    ld = col0 + E
    g = torch.Generator().manual_seed(3)
    ids = torch.repeat_interleave(torch.arange(A, dtype=torch.int32), n // A)
    if not sorted_ids:
        ids = ids[torch.randperm(n, generator=g)]
    ids = ids.to(dev)
    rows = torch.randn(n, ld, generator=g).to(dev)
    lib = L.load()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def default():
        out = torch.zeros(A, E, device=dev)
        L.check(lib.emd_deform_input_backward(n, E, ld, col0, ids.data_ptr(), rows.data_ptr(), out.data_ptr(), st()), "emd_deform_input_backward")

    def deterministic():
        L.actor_row_sum_det(rows, E, ids, A, col0=col0)
    res = interleaved({"default": default, "deterministic": deterministic})
    res["op"] = f"dL/d instances_embedding: {n} points x {E} columns of a [{n}, {ld}] gradient, {A} actors, ids {'sorted by actor' if sorted_ids else 'interleaved'}"
    res["workspace_bytes"] = L.track_det_workspace_size(A, 0, n, E)
    res["launches"] = {"default": "zero fill, k_deform_input_bwd", "deterministic": "k_row_sum_keys, the radix sort's passes, k_segsum_chunks, k_segsum_long"}
    return res


res = {"chain": chain(), "row_sum_sorted": row_sum(True), "row_sum_interleaved": row_sum(False)}
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "track_deterministic_microbench.json")
open(out, "w").write(json.dumps(res, indent=1) + "\n")
print(json.dumps(res))
