"""The HexPlane regularisers restated in torch (the K-Planes / 4DGaussians formulation compute_regulation inherits, S3Gaussian/scene/
gaussian_model.py:745-784), run in fp64 through autograd: the reference of tests/test_plane_reg_{cpu,gpu}.py.  Also the case builder and the
criterion of DESIGN.md section 5.  No emd_amd import except the segment length: the reference shares no code with what it checks."""
import functools
import itertools

import torch

from emd_amd import _lib as L

PAIRS = list(itertools.combinations(range(4), 2))
SPATIAL, TIME = (0, 1, 3), (2, 4, 5)
UPSTREAM = 0.37                       # (0.37 * loss + 1).backward(): a non-trivial upstream gradient
WEIGHTS = dict(time_smoothness_weight=0.013, l1_time_planes_weight=0.0071, plane_tv_weight=0.029)      # three distinct weights
SEG = L.PLANE_REG_SEG


def compute_plane_smoothness(t):
    """torch.square(second difference along H).mean() of one plane [1, C, H, W]."""
    first_difference = t[..., 1:, :] - t[..., :-1, :]
    second_difference = first_difference[..., 1:, :] - first_difference[..., :-1, :]
    return torch.square(second_difference).mean()


def plane_regulation(grids):
    return sum(compute_plane_smoothness(g[p]) for g in grids for p in SPATIAL)


def time_regulation(grids):
    return sum(compute_plane_smoothness(g[p]) for g in grids for p in TIME)


def l1_regulation(grids):
    return sum(torch.abs(1 - g[p]).mean() for g in grids for p in TIME)


def compute_regulation(grids, time_smoothness_weight, l1_time_planes_weight, plane_tv_weight):
    """-> loss, (tv, ts, l1)"""
    tv, ts, l1 = plane_regulation(grids), time_regulation(grids), l1_regulation(grids)
    return plane_tv_weight * tv + time_smoothness_weight * ts + l1_time_planes_weight * l1, torch.stack([tv, ts, l1])


# name -> (channels, resolutions per scale, sigma of the time planes).  What each shape is for is in tests/test_plane_reg_gpu.py.
CASES = {
    "tiny-s5e-2": (5, [[5, 3, 4, 3]], 0.05),
    "tiny-s1e-3": (5, [[5, 3, 4, 3]], 1e-3),
    "tiny_h5-s5e-2": (5, [[4, 5, 3, 4]], 0.05),           # ([5, 3, 4, 3] has no plane with H = 5: 5 is only ever a W there)
    "two_scales-s5e-2": (32, [[9, 7, 6, 5], [18, 14, 12, 5]], 0.05),
    "two_scales-s1e-3": (32, [[9, 7, 6, 5], [18, 14, 12, 5]], 1e-3),
    "segments-s5e-2": (16, [[10, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1]], 0.05),
    "segments-s1e-3": (16, [[10, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1]], 1e-3),
    "chunks-s5e-2": (32, [[40, 5, 4, 3]], 0.05),          # W * C = 1280: two column chunks of 1024, the second partly filled, wide accesses
    "chunks_odd-s1e-3": (5, [[300, 4, 3, 5]], 1e-3),      # W * C = 1500: the same with dword accesses and rows off 16-byte alignment
    "workload-s1e-3": (32, [[512, 512, 512, 25]], 1e-3),
}
SMALL_CASES = [k for k in CASES if not k.startswith("workload")]


def make_grids(channels, resolutions, sigma, seed=0):
    """fp32 CPU planes [scale][plane] of logical shape [1, C, H, W] in channel-last memory, with init_grid_param's value ranges: spatial planes
    U(0.1, 0.5), time planes 1 + sigma * randn with a fixed tenth of the entries (every tenth in memory order) set back to exactly 1."""
    g = torch.Generator().manual_seed(seed)
    grids = []
    for res in resolutions:
        planes = []
        for p, (a, b) in enumerate(PAIRS):
            H, W = res[b], res[a]
            if p in TIME:
                cl = 1 + sigma * torch.randn(H, W, channels, generator=g)
                cl.view(-1)[::10] = 1.0
            else:
                cl = 0.1 + 0.4 * torch.rand(H, W, channels, generator=g)
            planes.append(cl.permute(2, 0, 1)[None])
        grids.append(planes)
    return grids


@functools.lru_cache(maxsize=None)
def case(name):
    return make_grids(*CASES[name])


def run(grids, dtype, device, fn=compute_regulation, weights=WEIGHTS):
    """The restatement in `dtype` on `device` through autograd -> dict(loss, terms, grads [scale][plane], each [1, C, H, W])."""
    leaves = [[p.detach().to(device=device, dtype=dtype, copy=True).requires_grad_(True) for p in g] for g in grids]     # (copies: the case stays as it is)
    loss, terms = fn(leaves, **weights)
    (UPSTREAM * loss + 1).backward()
    return dict(loss=loss.detach(), terms=terms.detach(), grads=[[p.grad for p in g] for g in leaves])


_REF = {}


def reference(name, device="cpu"):
    """fp64, computed once per (case, device) and shared; callers leave it unchanged."""
    key = (name, str(device))
    if key not in _REF:
        _REF[key] = run(case(name), torch.float64, device)
    return _REF[key]


def criterion(got, ref, what=""):
    """element-wise 1e-4 |ref| + 1e-6 max |ref| and relative L2 1e-5 per plane gradient, relative 1e-5 on the loss and on each
    term.  Prints every figure before it asserts."""
    for k, g, r in [("loss", got["loss"].reshape(1), ref["loss"].reshape(1))] + [(n, got["terms"][i:i + 1], ref["terms"][i:i + 1]) for i, n in enumerate(("tv", "ts", "l1"))]:
        g, r = g.double().cpu(), r.double().cpu()
        err, tol = float((g - r).abs()), 1e-5 * float(r.abs())
        print(f"{what} {k}: got {float(g):.9e} ref {float(r):.9e} |err| {err:.3e} tol {tol:.3e}")
        assert err <= tol, (what, k, float(g), float(r))
    for s, (gs, rs) in enumerate(zip(got["grads"], ref["grads"])):
        for p, (g, r) in enumerate(zip(gs, rs)):
            assert g.shape == r.shape, (what, s, p, g.shape, r.shape)
            g, r = g.double().to(r.device), r.double()
            assert bool(torch.isfinite(g).all()), (what, s, p)
            err = (g - r).abs()
            tol = 1e-4 * r.abs() + 1e-6 * r.abs().max()
            worst = float((err / tol.clamp_min(1e-300)).max())
            rel_l2 = float((g - r).norm() / r.norm().clamp_min(1e-300))
            print(f"{what} grad scale {s} plane {p} {tuple(r.shape)}: worst element {worst:.3f} of its tolerance, relative L2 {rel_l2:.3e}")
            assert bool((err <= tol).all()), (what, s, p, worst)
            assert rel_l2 <= 1e-5, (what, s, p, rel_l2)
