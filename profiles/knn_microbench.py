"""Stand-alone timings of the k-NN search and the embedding regulariser on one MI355X (not called by bench.py).

    python profiles/knn_microbench.py --out profiles/knn_microbench.json [--quick] [--no-scipy]

1. emd_knn at N = 1 M / 2 M / 3 M, k = 3 and 20, uniform box (200 x 200 x 20) and the clustered generator of the tests scaled up: milliseconds,
   median of 20 calls after 3 warm-up calls, device events.  Yardstick on the same host: scipy.spatial.cKDTree(p).query(p, k + 1, workers=16)
   (build + query, one call), when scipy is importable; the ratio is reported, not asserted.
2. embedding_reg forward and backward at N = 2 M, k = 20, E = 4: milliseconds, the bytes the formulation moves (model below), their share of
   8 TB/s; the backward with the stored per-pair factors and with the factors recomputed; yardstick on the same GPU: the torch formulation the
   reference runs (emb[:, None, :].expand, emb[idx], the formula, autograd), five repeats, spread = max - min.
3. table order: the same regulariser with the points (and so the table's rows) in input order against Z-order.

Byte model of the regulariser (fp32, int32; P = N k pairs, R = 4 E bytes per embedding row), compulsory traffic only -- every array once:
    forward            P (4 idx + 4 w) + N R                                     (+ 4 P when the factors are stored)
    backward           P (4 idx + 4 w or factor) + P 4 rev_slot + 4 N rev_start + N R read + N R written
The gathers of neighbour rows are NOT in the model (a row that is in cache costs nothing, one that is not costs a 64-byte sector or more): the
model is the floor, `fraction_of_8TBps` says how far above it the kernels run."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emd_amd import knn as K  # noqa: E402

DEV = "cuda:0"
PEAK_BPS = 8e12


def uniform(n, seed):
    return (torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * torch.tensor([200.0, 200.0, 20.0])).contiguous()


def clustered(n, seed):
    """tests/knn_checks.clustered_points scaled up: the cluster count grows with n (3 125 points per cluster, as at 200 000 points)."""
    g = torch.Generator().manual_seed(seed)
    clusters = max(64, n // 3125)
    centres = torch.randn(clusters, 3, generator=g) * torch.tensor([40.0, 40.0, 2.0]) * (clusters / 64) ** (1 / 3)
    which = torch.randint(0, clusters, (n,), generator=g)
    spread = torch.rand(n, 1, generator=g) * 3.0
    return (centres[which] + torch.randn(n, 3, generator=g) * spread).float().contiguous()


def time_ms(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def summarise(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "calls": len(ms)}


def bench_knn(sizes, reps, use_scipy):
    rows = []
    for n in sizes:
        for name, gen in (("uniform", uniform), ("clustered", clustered)):
            p_cpu = gen(n, 100 + n % 97)
            p = p_cpu.to(DEV)
            for k in (3, 20):
                idx = torch.empty(n, k, dtype=torch.int32, device=DEV)
                d2 = torch.empty(n, k, dtype=torch.float32, device=DEV)
                ws = [None]

                def call():
                    ws[0] = K._knn_into(p, k, idx, d2, None, ws[0])
                row = {"N": n, "k": k, "cloud": name, **summarise(time_ms(call, 3, reps))}
                if use_scipy:
                    from scipy.spatial import cKDTree
                    x = p_cpu.numpy()
                    t0 = time.perf_counter()
                    _, ref = cKDTree(x).query(x, k + 1, workers=16)
                    row["scipy_ckdtree_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    row["scipy_over_hip"] = round(row["scipy_ckdtree_ms"] / row["median_ms"], 1)
                    # not a test, a sanity line: rows whose neighbour SETS differ from scipy's (ties aside, there should be none)
                    got = idx.cpu().long().sort(dim=1).values
                    want = torch.from_numpy(ref[:, 1:]).long().sort(dim=1).values
                    row["rows_differing_from_scipy"] = int((got != want).any(dim=1).sum())
                else:
                    row["scipy_ckdtree_ms"] = "not measured"
                print(json.dumps(row), flush=True)
                rows.append(row)
            del p
    return rows


def torch_reg(e, idx, w):
    """what the reference runs: weighted_l2_loss_v2(emb[:, None, :].expand(-1, k, -1), emb[idx], w)"""
    x = e[:, None, :].expand(-1, idx.shape[1], -1)
    y = e[idx]
    return torch.sqrt(((x - y) ** 2).sum(-1) * w + 1e-20).mean()


def bench_reg(n, k, E, reps, order):
    p = uniform(n, 7)
    if order == "z-order":
        q = ((p - p.min(0).values) / (p.max(0).values - p.min(0).values) * 1023).long()

        def spread(v):
            v = (v | (v << 16)) & 0x030000FF
            v = (v | (v << 8)) & 0x0300F00F
            v = (v | (v << 4)) & 0x030C30C3
            return (v | (v << 2)) & 0x09249249
        p = p[torch.argsort(spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2))].contiguous()
    t = K.KnnTable(p.to(DEV), k=k, weight_fn=lambda d2: torch.exp(-d2))
    e = (torch.randn(n, E, generator=torch.Generator().manual_seed(8)) * 0.3).to(DEV)
    g = torch.ones(1, device=DEV)
    grad = torch.empty_like(e)
    P, R = n * k, 4 * E
    out = {"N": n, "k": k, "E": E, "table_order": order}
    for store in (False, True):
        t.store_factors, t.factors = store, (torch.empty_like(t.w) if store else None)
        fwd = K.embed_reg_forward(e, t)
        f = summarise(time_ms(lambda: K.embed_reg_forward(e, t), 3, reps))
        b = summarise(time_ms(lambda: K.embed_reg_backward(e, t, fwd, g, grad), 3, reps))
        fb = P * 8 + n * R + (4 * P if store else 0)
        bb = P * 8 + P * 4 + 4 * n + 2 * n * R
        tag = "stored_factors" if store else "recomputed_factors"
        out[tag] = {"forward": {**f, "model_bytes": fb, "fraction_of_8TBps": round(fb / (f["median_ms"] * 1e-3) / PEAK_BPS, 4)},
                    "backward": {**b, "model_bytes": bb, "fraction_of_8TBps": round(bb / (b["median_ms"] * 1e-3) / PEAK_BPS, 4)},
                    "pair_median_ms": round(f["median_ms"] + b["median_ms"], 4)}
    t.store_factors, t.factors = False, None
    if order == "input":
        idx_l, w = t.idx.long(), t.w

        def torch_pair():
            ee = e.detach().requires_grad_(True)
            torch_reg(ee, idx_l, w).backward()

        def hip_pair():
            fw = K.embed_reg_forward(e, t)
            K.embed_reg_backward(e, t, fw, g, grad)
        yard = [statistics.median(time_ms(torch_pair, 2, 5)) for _ in range(5)]
        hip = [statistics.median(time_ms(hip_pair, 2, 5)) for _ in range(5)]
        out["torch_formulation_pair_ms"] = {"repeats": [round(v, 4) for v in yard], "median_ms": round(statistics.median(yard), 4),
                                            "spread_ms": round(max(yard) - min(yard), 4)}
        out["hip_pair_ms"] = {"repeats": [round(v, 4) for v in hip], "median_ms": round(statistics.median(hip), 4),
                              "spread_ms": round(max(hip) - min(hip), 4)}
        out["torch_over_hip"] = round(statistics.median(yard) / statistics.median(hip), 2)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="1 M points only, 5 calls (a rehearsal, not a result)")
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_microbench needs a GPU: a CPU run says nothing about these timings")
    use_scipy = not a.no_scipy
    if use_scipy:
        try:
            import scipy.spatial  # noqa: F401
        except ImportError:
            use_scipy = False
    sizes = [1_000_000] if a.quick else [1_000_000, 2_000_000, 3_000_000]
    reps = 5 if a.quick else 20
    n_reg = 1_000_000 if a.quick else 2_000_000
    res = {"device": torch.cuda.get_device_name(0), "quick": a.quick,
           "knn": bench_knn(sizes, reps, use_scipy),
           "embedding_reg": [bench_reg(n_reg, 20, 4, reps, "input"), bench_reg(n_reg, 20, 4, reps, "z-order")]}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
