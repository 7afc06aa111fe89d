"""The refinement event of OmniRe's actor classes (RigidNodes / DeformableNodes.refinement_after, models/nodes/rigid.py:278-465) restated
literally with torch on the CPU -- the reference of tests/test_nodes_refine_cpu.py and tests/test_nodes_refine_gpu.py:

  split with `cat` (the original stays, its log-scale reduced in place), then duplicate (decided AFTER the reduction), then cull on the GROWN arrays
  -- opacity, world size, screen size with 0 on new rows, and `cull_out_of_bound`: |mean_c| > instances_size[id]_c / 2 for any c, so a split sample is
  tested at its sampled position -- carrying the ids, one Adam moment (zero on new rows) and the source row / kind of every row; then optionally the
  stable sort by id.

`refine(case, dtype)` evaluates every decision in `dtype` (float32 or float64) on the float32 inputs.  Where both agree, no decision hangs on a
rounding, and a float32 evaluation with another exp() agrees as well: that is what lets the GPU comparison be exact.  To show it, the result
also carries, for every row of the grown arrays, the smallest distance of any coordinate to its box face next to the rounding bound of the
position (8 u times the sum of magnitudes of ((R0 e0 + R1 e1) + R2 e2) + v, u = 2^-24), and the relative distances of the threshold quantities to
their thresholds.  `make_case` builds inputs and `settle` moves the rows whose decisions would hang on a rounding until none is left."""
import functools
import types

import numpy as np
import torch

U = 2.0 ** -24
BOX_FACTOR = 16.0             # a box-face distance must be at least this many rounding bounds
REL_MARGIN = 2.0 ** -12       # a threshold quantity must be at least this far (relative) from its threshold: float32 exp() / sigmoid are good to a few ulp


def _f32(v):
    return float(np.float32(v))


def default_cfg(**over):
    """thresholds as the host hands them to the kernel: rounded to float once"""
    cfg = dict(do_densify=True, do_cull=True, use_split_screen=True, cull_big=True, use_cull_screen=True, cull_out_of_bound=True,
               grad_threshold=_f32(0.0003), size_threshold=_f32(0.05), split_screen=_f32(0.05), cull_alpha=_f32(0.005), cull_size=_f32(1.0),
               cull_screen=_f32(0.15))
    cfg.update(over)
    return cfg


def rotation_rows(q):
    """R(q / |q|) as build_rotation writes it -> [n,3,3]"""
    qn = q / q.norm(dim=-1, keepdim=True)
    r, x, y, z = qn.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def refine(case, dtype=torch.float32, group=False):
    """-> namespace: means, log_scales, ids, moment, src, kind of the output rows (kind 0 original, 1 duplicate, 2 + r sample of replica r), counts
    (n_keep, n_dup, n_split, [n_samp_r]), and the margins (see the module docstring)."""
    c, ns = case.cfg, case.num_samples
    t = lambda x: x.to(dtype)
    m, s, q, o = t(case.means).clone(), t(case.log_scales).clone(), t(case.quats), t(case.opacity)
    gn, vis, m2d = t(case.grad_norm), t(case.vis_counts), t(case.max_2Dsize)
    size, ids, N = t(case.instances_size), case.ids.long(), case.means.shape[0]
    mom = case.moment.clone()
    thr = {k: torch.tensor(c[k], dtype=dtype) for k in ("grad_threshold", "size_threshold", "split_screen", "cull_alpha", "cull_size", "cull_screen")}
    rel = lambda v, th: ((v - th).abs() / th.abs()).double()
    margins = {}
    src, kind = torch.arange(N), torch.zeros(N, dtype=torch.long)
    M_, S_, O_, I_, D_, K_, SRC_ = m, s, o, ids, mom, kind, src
    m2d_ = m2d
    bound = torch.zeros(N, dtype=torch.float64)
    n_split = 0
    if c["do_densify"]:
        ratio = gn / vis
        high = ratio > thr["grad_threshold"]
        smax = torch.exp(s).max(dim=-1).values
        splits = smax > thr["size_threshold"]
        if c["use_split_screen"]:
            splits = splits | (m2d > thr["split_screen"])
        splits = splits & high
        margins["grad"], margins["split_size"] = rel(ratio, thr["grad_threshold"]), rel(smax, thr["size_threshold"])
        n_split = int(splits.sum())
        R = rotation_rows(q[splits])
        std = torch.exp(s[splits])
        new_means, new_bound = [], []
        for r in range(ns):
            e = std * t(case.normals[r])[splits]                                         # [n_split, 3]
            terms = R * e[:, None, :]                                                    # R[c][k] e[k]
            new_means.append(((terms[..., 0] + terms[..., 1]) + terms[..., 2]) + m[splits])
            new_bound.append(8 * U * (terms.abs().sum(-1) + m[splits].abs()).max(dim=-1).values.double())
        new_scales = torch.log(std / 1.6)
        s[splits] = new_scales                                                           # the original takes the reduced scale in place
        smax_after = torch.exp(s).max(dim=-1).values
        dups = (smax_after <= thr["size_threshold"]) & high
        margins["dup_size"] = rel(smax_after, thr["size_threshold"])
        n_dup = int(dups.sum())
        sp, du = splits.nonzero().squeeze(-1), dups.nonzero().squeeze(-1)
        z = lambda n, like: torch.zeros((n,) + tuple(like.shape[1:]), dtype=like.dtype)
        M_ = torch.cat([m] + new_means + [m[dups]])
        S_ = torch.cat([s] + [new_scales] * ns + [s[dups]])
        O_ = torch.cat([o] + [o[splits]] * ns + [o[dups]])
        I_ = torch.cat([ids] + [ids[splits]] * ns + [ids[dups]])
        D_ = torch.cat([mom, z(ns * n_split + n_dup, mom)])
        K_ = torch.cat([kind] + [torch.full((n_split,), 2 + r) for r in range(ns)] + [torch.ones(n_dup, dtype=torch.long)])
        SRC_ = torch.cat([src] + [sp] * ns + [du])
        m2d_ = torch.cat([m2d, z(ns * n_split + n_dup, m2d)])                             # new rows carry max_2Dsize 0
        bound = torch.cat([bound] + new_bound + [torch.zeros(n_dup, dtype=torch.float64)])
    half = size[I_] / 2
    box_distance = (M_.abs() - half).abs().min(dim=-1).values.double()
    culls = torch.zeros(M_.shape[0], dtype=torch.bool)
    if c["do_cull"]:
        op, big_s = torch.sigmoid(O_), torch.exp(S_).max(dim=-1).values
        culls = op < thr["cull_alpha"]
        margins["alpha"] = rel(op, thr["cull_alpha"])
        if c["cull_big"]:
            culls = culls | (big_s > thr["cull_size"])
            margins["cull_size"] = rel(big_s, thr["cull_size"])
            if c["use_cull_screen"]:
                culls = culls | (m2d_ > thr["cull_screen"])
        if c["cull_out_of_bound"]:
            culls = culls | (M_.abs() > half).any(dim=-1)
    keep = ~culls
    out = types.SimpleNamespace(means=M_[keep], log_scales=S_[keep], ids=I_[keep], moment=D_[keep], src=SRC_[keep], kind=K_[keep])
    if group:
        order = torch.argsort(out.ids, stable=True)
        for k in ("means", "log_scales", "ids", "moment", "src", "kind"):
            setattr(out, k, getattr(out, k)[order])
    out.counts = (int((out.kind == 0).sum()), int((out.kind == 1).sum()), n_split, [int((out.kind == 2 + r).sum()) for r in range(ns)])
    out.split_mask = splits if c["do_densify"] else torch.zeros(N, dtype=torch.bool)
    out.box_distance, out.box_bound, out.margins, out.grown_src = box_distance, bound, margins, SRC_
    out.box_active = bool(c["do_cull"] and c["cull_out_of_bound"])
    return out


def hanging_rows(ref):
    """source rows one of whose decisions is closer to its threshold (or box face) than the margins the module promises"""
    bad = torch.zeros(int(ref.grown_src.max()) + 1 if ref.grown_src.numel() else 0, dtype=torch.bool)
    for v in ref.margins.values():
        bad[ref.grown_src[:v.shape[0]][v < REL_MARGIN]] = True
    if ref.box_active:
        bad[ref.grown_src[ref.box_distance < BOX_FACTOR * ref.box_bound]] = True
    return bad


def ids_layout(layout, N, A, g):
    if layout == "sorted":
        return torch.sort(torch.randint(0, A, (N,), generator=g)).values
    if layout == "interleaved":
        return torch.arange(N) % A
    if layout == "one":
        return torch.full((N,), A - 1, dtype=torch.long)
    if layout == "gaps":                                        # only every third actor owns points, in random order
        return torch.randint(0, (A + 2) // 3, (N,), generator=g) * 3 % A
    if layout == "random":
        return torch.randint(0, A, (N,), generator=g)
    raise ValueError(layout)


def make_case(N, A, num_samples, layout="random", seed=0, **cfg):
    """Rows of A actors with boxes of about 2 x 1 x 1.5: most means inside, some outside, stds such that a good share of the split samples crosses a
    face; gradients on both sides of the threshold, scales on both sides of the split and the cull size, some rows transparent."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + A + num_samples)
    r = lambda *s: torch.rand(*s, generator=g)
    case = types.SimpleNamespace(num_samples=num_samples, num_actors=A, cfg=default_cfg(**cfg))
    case.ids = ids_layout(layout, N, A, g)
    case.instances_size = torch.tensor([2.0, 1.0, 1.5]) * (0.75 + 0.5 * r(A, 1))
    case.means = (r(N, 3) * 2 - 1) * 0.56 * case.instances_size[case.ids]
    case.log_scales = torch.log(torch.tensor(0.004)) + r(N, 3) * 6.5                              # exp: 0.004 .. 2.7
    case.quats = torch.randn(N, 4, generator=g)
    case.opacity = torch.randn(N, generator=g) * 3.0 - 1.0
    case.grad_norm = r(N) * 1.2e-3
    case.vis_counts = torch.randint(1, 4, (N,), generator=g).float()
    case.max_2Dsize = r(N) * 0.2
    case.normals = torch.randn(num_samples, N, 3, generator=g)
    case.moment = torch.randn(N, 3, generator=g)
    return settle(case)


def settle(case):
    """Move the rows one of whose decisions would hang on a rounding (a little larger, more opaque, a little further from the face) until the
    float64 evaluation sees none."""
    for _ in range(20):
        bad = hanging_rows(refine(case, torch.float64))
        if not bool(bad.any()):
            return case
        case.log_scales[bad] += 0.013
        case.opacity[bad] += 0.021
        case.grad_norm[bad] *= 1.017
        case.means[bad] *= 0.983
    raise AssertionError("the inputs did not settle")


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """every input tests/test_nodes_refine_gpu.py compares with this reference, built once: [(name, case)]"""
    cases = [("box", make_case(3000, 7, 3, "random", seed=1))]
    k = 0
    for N in (0, 1, 255, 256, 257, 513, 1000):
        for A in (1, 3, 33, 513):
            for layout in ("sorted", "interleaved", "one", "gaps"):
                cases.append((f"N{N} A{A} {layout}", make_case(N, A, 1 + k % 3, layout, seed=2)))
                k += 1
    return tuple(cases)
