"""The k-NN regulariser of SMPLNodes at 64 instances x 6 890 points, K = 3 (two others per point), SH degree 1 (20 columns) and 3 (56 columns).

  (a) `knn.neighbour_std` forward + backward through autograd, and its two kernels alone (the C entry points on buffers kept between calls) with
      their fraction of the copy peak measured in this run; a kernel's bytes count every row, gathered or its own, once per read:
        forward   N (4 k  +  4 T (1 + k)  +  8 T)                         idx row, own + k gathered rows, the stash row written
        backward  N (8  +  12 T  +  d (4 + 12 T)  +  4 T)  with d = k      rev_start, own row + stash, per incoming slot (k on average) its
                                                                          rev_slot entry, row and stash row, the gradient row written
  (b) the torch formulation on the same table: per block act(x)[cat(self, idx)].std(dim=1).mean() * w, summed, and its backward
  (c) `KnnTable.refresh` with `segment_start` (the search and the transposed adjacency), `knn_segments` alone, and a torch loop over the instances of
      `cdist` + `topk`
Medians of `--reps` between HIP events.  Every block is written to the JSON as soon as it is measured:
    python profiles/neighbour_std_microbench.py [--reps 30] [--out profiles/neighbour_std_microbench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV, P, PER, K = "cuda:0", 64, 6890, 3
ACTS = ("identity", "exp", "sigmoid", "identity", "identity")
WEIGHTS = (0.002, 0.002, 0.0005, 0.001, 0.001)


def stats(ts):
    ts = sorted(ts)
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4))


def event_timed(fn, reps):
    ts = []
    for k in range(reps + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= 5:
            ts.append(e0.elapsed_time(e1))
    return stats(ts)


def cloud(seed=0):
    """64 people of 6 890 points: an anisotropic blob per person (a standing body's proportions), the people a few metres apart."""
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(P, PER, 3, generator=g) * torch.tensor([0.25, 0.85, 0.15]) + torch.randn(P, 1, 3, generator=g) * torch.tensor([8.0, 0.0, 8.0])
    return pts.reshape(-1, 3).contiguous(), torch.arange(P + 1, dtype=torch.int32) * PER


def blocks_for(degree, seed=1):
    g = torch.Generator().manual_seed(seed)
    N, rest = P * PER, (degree + 1) ** 2 - 1
    return [torch.randn(N, 4, generator=g), torch.randn(N, 3, generator=g) * 0.3 - 3.0, torch.randn(N, 1, generator=g), torch.rand(N, 3, generator=g),
            torch.randn(N, rest, 3, generator=g) * 0.1]


def torch_formulation(xs, nn):
    fn = dict(identity=lambda x: x, exp=torch.exp, sigmoid=torch.sigmoid)
    total = 0.0
    for x, a, w in zip(xs, ACTS, WEIGHTS):
        total = total + fn[a](x).reshape(x.shape[0], -1)[nn].std(dim=1).mean() * w
    return total


def direct_calls(xs, table):
    """-> (forward, backward): closures over the C entry points with every buffer allocated once."""
    from emd_amd import _lib as L
    lib = L.load()
    n = table.N
    flat = [x.detach().reshape(n, -1).contiguous() for x in xs]
    T = sum(x.shape[1] for x in flat)
    a = L.EmdNeighbourStdArgs()
    a.num_points, a.k, a.num_blocks = n, table.k, len(flat)
    a.idx, a.rev_start, a.rev_slot = table.idx.data_ptr(), table.rev_start.data_ptr(), table.rev_slot.data_ptr()
    keep = [torch.empty_like(x) for x in flat]
    for b, (x, act, w) in enumerate(zip(flat, ACTS, WEIGHTS)):
        a.x[b], a.dx[b], a.cols[b], a.act[b], a.weight[b] = x.data_ptr(), keep[b].data_ptr(), x.shape[1], L.NSTD_ACT[act], w
    stash, terms, g = torch.empty(n * T * 2, device=DEV), torch.empty(len(flat), device=DEV), torch.ones(len(flat), device=DEV)
    ws = torch.zeros(lib.emd_neighbour_std_workspace_size(), dtype=torch.uint8, device=DEV)
    a.stash, a.terms, a.g_terms = stash.data_ptr(), terms.data_ptr(), g.data_ptr()
    keep += flat + [stash, terms, g, ws]
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fwd = lambda: L.check(lib.emd_neighbour_std_forward(C.byref(a), ws.data_ptr(), ws.numel(), st()), "emd_neighbour_std_forward")
    bwd = lambda: L.check(lib.emd_neighbour_std_backward(C.byref(a), st()), "emd_neighbour_std_backward")
    return fwd, bwd, T, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "neighbour_std_microbench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from emd_amd.knn import KnnTable, knn_segments, neighbour_std
    N, k = P * PER, K - 1
    res = dict(instances=P, points_per_instance=PER, K=K, reps=a.reps, device=torch.cuda.get_device_name(0))

    def put(key, value):
        res[key] = value
        json.dump(res, open(a.out, "w"), indent=1)
        print(json.dumps({key: value}), flush=True)

    src = torch.empty(64 << 20, device=DEV)                            # 256 MB each way
    dst = torch.empty_like(src)
    copy = event_timed(lambda: dst.copy_(src), a.reps)
    peak = 2 * src.numel() * 4 / (copy["median_ms"] * 1e-3)
    put("copy_peak", dict(bytes_each_way=src.numel() * 4, **copy, bytes_per_s=round(peak)))
    del src, dst

    pts, seg = cloud()
    pts, seg = pts.to(DEV), seg.to(DEV)
    table = KnnTable(pts, k=k, segment_start=seg)
    nn = torch.cat([torch.arange(N, device=DEV)[:, None], table.idx.long()], dim=1)
    assert int(table.idx.min()) >= 0
    for degree in (1, 3):
        xs = [x.to(DEV).requires_grad_(True) for x in blocks_for(degree)]
        out = {}

        def hip():
            for x in xs:
                x.grad = None
            neighbour_std(xs, table, WEIGHTS, ACTS).sum().backward()

        def eager():
            for x in xs:
                x.grad = None
            torch_formulation(xs, nn).backward()
        out["a_neighbour_std_forward_backward"] = event_timed(hip, a.reps)
        hip_grads = [x.grad.clone() for x in xs]
        hip_value = float(neighbour_std(xs, table, WEIGHTS, ACTS).sum().detach())
        out["b_torch_forward_backward"] = event_timed(eager, a.reps)
        ref_value = float(torch_formulation(xs, nn).detach())
        out["value_hip"], out["value_torch"] = hip_value, ref_value
        out["gradient_relative_l2_hip_vs_torch"] = [float(torch.linalg.norm(h - x.grad) / torch.linalg.norm(x.grad)) for h, x in zip(hip_grads, xs)]
        fwd, bwd, T, keep = direct_calls(xs, table)
        fwd_bytes = N * (4 * k + 4 * T * (1 + k) + 8 * T)
        bwd_bytes = N * (8 + 12 * T + k * (4 + 12 * T) + 4 * T)
        for name, fn, nbytes in (("forward_kernel", fwd, fwd_bytes), ("backward_kernel", bwd, bwd_bytes)):
            t = event_timed(fn, a.reps)
            out[name] = dict(bytes=nbytes, **t, bytes_per_s=round(nbytes / (t["median_ms"] * 1e-3)),
                             fraction_of_copy_peak=round(nbytes / (t["median_ms"] * 1e-3) / peak, 4))
        out["columns"] = T
        put(f"sh_degree_{degree}", out)
        del keep, xs

    out = {}
    out["refresh_with_segments"] = event_timed(lambda: table.refresh(pts), a.reps)
    out["knn_segments_alone"] = event_timed(lambda: knn_segments(pts, seg, k), a.reps)

    def torch_loop():
        rows = []
        for p in range(P):
            q = pts[p * PER:(p + 1) * PER]
            rows.append(torch.cdist(q, q).topk(K, dim=1, largest=False).indices[:, 1:] + p * PER)
        return torch.cat(rows)
    out["torch_cdist_topk_loop"] = event_timed(torch_loop, max(a.reps // 3, 5))
    ref = torch_loop()
    out["rows_equal_to_torch_as_sets"] = float((table.idx.long().sort(dim=1).values == ref.sort(dim=1).values).all(dim=1).float().mean())
    put("c_knn", out)


if __name__ == "__main__":
    main()
