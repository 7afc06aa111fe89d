"""The image tail of an OmniRe step restated in plain torch (the formulas of include/emd_raster.h, EmdTrainerLossArgs: compute_losses with
models/losses.py, pytorch_msssim.SSIM(data_range=1, channel=3) and kornia.losses.inverse_depth_smoothness_loss), run in fp64 through autograd:
the reference of tests/test_trainer_loss_{cpu,gpu}.py.  Also the named cases and the criterion.  No emd_amd import except the two exported
constants: the reference shares no code with what it checks."""
import functools
import itertools
import math

import torch
import torch.nn.functional as F

from emd_amd import _lib as L

UPSTREAM = 0.37                      # (0.37 * loss + 1).backward(): a non-trivial upstream gradient
CHUNK, TILE = L.TRAINER_LOSS_CHUNK, L.TRAINER_SSIM_TILE
TERMS = ("rgb_loss", "ssim_loss", "mask_loss", "depth_loss", "opacity_entropy_loss", "inverse_depth_smoothness_loss")
# every term on, six distinct weights
FULL = dict(w_rgb=0.8, w_ssim=0.2, w_mask=0.05, mask_type="bce", safe_limit=0.1, w_depth=0.1, depth_type="l1", normalize=False, inverse=False,
            upper_bound=80.0, w_entropy=0.03, w_smooth=0.02)
DEPTH_OPTIONS = [dict(depth_type=t, normalize=n, inverse=i) for t, n, i in itertools.product(("l1", "l2", "smooth_l1"), (False, True), (False, True))]


# ---- the formulas ----------------------------------------------------------------------------------------

def gaussian_window(dtype, device):
    k = torch.arange(11, dtype=torch.float64, device=device) - 5
    g = torch.exp(-(k * k) / (2 * 1.5 ** 2))
    return (g / g.sum()).to(dtype)


def ssim_map(x, y):
    """[H,W,3] x 2 -> [3, H-10, W-10]: the separable 11-tap window without padding."""
    win = gaussian_window(x.dtype, x.device)
    wv, wh = win.view(1, 1, 11, 1).expand(3, 1, 11, 1), win.view(1, 1, 1, 11).expand(3, 1, 1, 11)
    filt = lambda u: F.conv2d(F.conv2d(u, wv, groups=3), wh, groups=3)
    X, Y = x.permute(2, 0, 1)[None], y.permute(2, 0, 1)[None]
    mu1, mu2 = filt(X), filt(Y)
    s1, s2, s12 = filt(X * X) - mu1 * mu1, filt(Y * Y) - mu2 * mu2, filt(X * Y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * (2 * s12 + C2) / (s1 + s2 + C2))[0]


class _SafeBCE(torch.autograd.Function):
    """The value of the clipped form with the gradient that survives the clip (autograd would zero it there)."""

    @staticmethod
    def forward(ctx, o, t, limit):
        oc = o.clamp(0, 1)
        ctx.save_for_backward(oc.clamp(limit, 1 - limit), t)
        return -torch.log(torch.where(t > 0, oc, 1 - oc)).clamp_min(math.log(limit))

    @staticmethod
    def backward(ctx, g):
        oh, t = ctx.saved_tensors
        return g * torch.where(t > 0, -1 / oh, 1 / (1 - oh)), None, None


def mask_loss(o, t, mask_type, limit):
    if mask_type == "bce":
        return F.binary_cross_entropy(o, t)          # log clamped at -100, gradient (o - t) / max(o (1 - o), 1e-12)
    return _SafeBCE.apply(o, t, limit).mean()


def depth_loss(d, l, t, depth_type, normalize, inverse, upper):
    v = (t > 0) & (l > 0.01) & (l < upper) & (d > 1e-4)
    a, b = d[v], l[v]
    if normalize:
        a, b = a / upper, b / upper
    if inverse:
        a, b = 1 / (a + 1e-5), 1 / (b + 1e-5)
    e = {"l1": lambda: (a - b).abs(), "l2": lambda: (a - b) ** 2, "smooth_l1": lambda: F.smooth_l1_loss(a, b, reduction="none", beta=1.0)}[depth_type]()
    return e.sum() / max(int(v.sum()), 1)             # an empty hit set: 0 (the trainer's mean of nothing is NaN)


def entropy_loss(o):
    oc = o.clamp(1e-6, 1 - 1e-6)
    return (-oc * oc.log()).mean()


def smoothness_loss(d, y):
    q = 1 / (d + 1e-5)
    y = y.detach()
    wx = torch.exp(-(y[:, :-1] - y[:, 1:]).abs().mean(-1))
    wy = torch.exp(-(y[:-1] - y[1:]).abs().mean(-1))
    return ((q[:, :-1] - q[:, 1:]) * wx).abs().mean() + ((q[:-1] - q[1:]) * wy).abs().mean()


def losses(x, y, o, s, d, l, cfg):
    """-> total, [6] weighted terms in the order of TERMS; a term whose weight is 0 or whose input is None is 0."""
    zero = x.new_zeros(())
    t = None if s is None else 1 - s
    terms = [
        cfg["w_rgb"] * (y - x).abs().mean() if cfg["w_rgb"] else zero,
        cfg["w_ssim"] * (1 - ssim_map(x, y).mean()) if cfg["w_ssim"] else zero,
        cfg["w_mask"] * mask_loss(o, t, cfg["mask_type"], cfg["safe_limit"]) if (cfg["w_mask"] and o is not None and s is not None) else zero,
        cfg["w_depth"] * depth_loss(d, l, t, cfg["depth_type"], cfg["normalize"], cfg["inverse"], cfg["upper_bound"])
        if (cfg["w_depth"] and d is not None and l is not None and s is not None) else zero,
        cfg["w_entropy"] * entropy_loss(o) if (cfg["w_entropy"] and o is not None) else zero,
        cfg["w_smooth"] * smoothness_loss(d, y) if (cfg["w_smooth"] and d is not None) else zero,
    ]
    return sum(terms), torch.stack(terms)


# ---- the cases -------------------------------------------------------------------------------------------

def _apart(t, step):
    """Nudge entries until no pixel is within 2e-3 of its right or lower neighbour (the smoothness term's kink)."""
    for _ in range(50):
        near = torch.zeros_like(t, dtype=torch.bool)
        near[:, :-1] |= (t[:, :-1] - t[:, 1:]).abs() < 2e-3
        near[:-1] |= (t[:-1] - t[1:]).abs() < 2e-3
        if not bool(near.any()):
            return t
        t = torch.where(near, t + step, t)
    raise AssertionError("could not separate neighbours")


def _away(t, kink, margin=5e-3):
    return torch.where((t - kink).abs() < margin, torch.full_like(t, kink + margin), t)


def make_inputs(H, W, seed=0, hits=True):
    """fp32 CPU inputs, every value at least 1e-3 away from every kink of every term and option."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    y = 0.25 + 0.5 * r(H, W, 3)
    x = y + (0.002 + 0.2 * r(H, W, 3)) * (1 - 2 * (r(H, W, 3) < 0.5).float())          # |x - y| >= 2e-3, both inside (0, 1)
    o = _away(_away(0.02 + 0.96 * r(H, W), 0.1), 0.9)                                  # safe-BCE clips at 0.1 and 0.9
    s = (r(H, W) < 0.3).float()
    d = _apart(5 + 55 * r(H, W), 0.0137)
    # the lidar depth within 0.1 .. 3 m of the rendered one, on either side (errors of a size that keeps every option's scalar of order one, where
    # fp32 can hold 1e-6 absolute); a tenth of the pixels beyond the upper bound, a fifth without a return
    l = d + (0.1 + 2.9 * r(H, W)) * (1 - 2 * (r(H, W) < 0.5).float())
    pick = r(H, W)
    l = torch.where(pick < 0.1, 81 + 19 * r(H, W), l)
    l = torch.where((pick >= 0.1) & (pick < 0.3), torch.zeros_like(l), l)
    if not hits:
        l = torch.zeros_like(l)
    return dict(x=x, y=y, o=o, s=s, d=d, l=l)


def make_edges(H=13, W=16):
    """The kinks themselves, where fp32 and fp64 still agree on the branch: x == y on every fifth pixel; constant depth runs along a row band and a
    column band; o cycling through {0, 1e-7, 0.05, 0.95, 1} against both mask values; l at 0 and just inside and outside (0.01, 80)."""
    c = make_inputs(H, W, seed=5)
    n = torch.arange(H * W).view(H, W)
    c["x"] = torch.where((n % 5 == 0)[..., None], c["y"], c["x"])
    c["d"][:, 4:9] = 7.5
    c["d"][3:6, :] = 12.0
    c["o"] = torch.tensor([0.0, 1e-7, 0.05, 0.95, 1.0])[n % 5]
    c["s"] = ((n // 5) % 2).float()
    c["l"] = torch.tensor([0.0, 0.0101, 0.0099, 79.99, 80.01, 30.0])[n % 6]
    return c


# name -> (builder, what it is for)
CASES = {
    "11x11": (lambda: make_inputs(11, 11, 1), "a single SSIM output per channel"),
    "12x13": (lambda: make_inputs(12, 13, 2), "the smallest odd W: rows of 39 floats, off 16-byte alignment"),
    "tiles": (lambda: make_inputs(TILE + 11, (TILE * 4 + 1) // 3 + 10, 3), "SSIM map one row and one float above whole tiles, three chunks of pixels"),
    "wide": (lambda: make_inputs(70, 531, 4), "many tiles and chunks; rows of 1593 floats"),
    "empty_hits": (lambda: make_inputs(12, 13, 6, hits=False), "no lidar return at all: the depth term is 0 with a zero gradient"),
    "edges": (make_edges, "the kinks: sign(0), the clips of both mask types, the thresholds of the hit set"),
}
SMOOTH_CASES = [k for k in CASES if k != "edges"]            # inputs away from every kink


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name][0]()


def config(**over):
    cfg = dict(FULL)
    cfg.update(over)
    return cfg


ONLY = {                                                       # the `edges` case term by term
    "rgb": dict(w_rgb=0.8), "ssim": dict(w_ssim=0.2), "mask_bce": dict(w_mask=0.05, mask_type="bce"), "mask_safe_bce": dict(w_mask=0.05, mask_type="safe_bce"),
    "depth": dict(w_depth=0.1), "entropy": dict(w_entropy=0.03), "smooth": dict(w_smooth=0.02),
}


def only(term):
    cfg = config(w_rgb=0.0, w_ssim=0.0, w_mask=0.0, w_depth=0.0, w_entropy=0.0, w_smooth=0.0)
    cfg.update(ONLY[term])
    return cfg


def run(inputs, cfg, dtype, device):
    """The restatement in `dtype` on `device` through autograd -> dict(loss, terms [6], g_rgb, g_opacity, g_depth)."""
    c = {k: v.detach().to(device=device, dtype=dtype, copy=True) for k, v in inputs.items()}          # (copies: the case stays as it is)
    for k in ("x", "o", "d"):
        c[k].requires_grad_(True)
    loss, terms = losses(c["x"], c["y"], c["o"], c["s"], c["d"], c["l"], cfg)
    (UPSTREAM * loss + 1).backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(loss=loss.detach(), terms=terms.detach(), g_rgb=z(c["x"]), g_opacity=z(c["o"]), g_depth=z(c["d"]))


_REF = {}


def reference(name, cfg, device="cpu"):
    """fp64, computed once per (case, configuration, device) and shared; callers leave it unchanged."""
    key = (name, tuple(sorted(cfg.items())), str(device))
    if key not in _REF:
        _REF[key] = run(case(name), cfg, torch.float64, device)
    return _REF[key]


def criterion(got, ref, cfg, what=""):
    """Scalars within 1e-6 absolute.  Gradients element-wise within 1e-4 |ref| + 1e-6 max |ref|, except a colour gradient
    that holds an SSIM term: within 1e-4 of its largest entry, the existing loss tail's rule (fp32 torch itself misses the element-wise bound by
    1.5 - 2.1 x there).  A gradient no term reaches may be None.  Prints every figure before it asserts."""
    for k, g, r in [("loss", got["loss"], ref["loss"])] + [(n, got["terms"][i], ref["terms"][i]) for i, n in enumerate(TERMS)]:
        g, r = float(g.double().cpu()), float(r.double().cpu())
        print(f"{what} {k}: got {g:.9e} ref {r:.9e} |err| {abs(g - r):.3e} tol 1.000e-06")
        assert abs(g - r) <= 1e-6, (what, k, g, r)
    for k in ("g_rgb", "g_opacity", "g_depth"):
        r = ref[k].double()
        g = got[k]
        if g is None:
            assert float(r.abs().max()) == 0.0, (what, k, "no gradient where the reference has one")
            continue
        g = g.double().to(r.device).reshape(r.shape)
        assert bool(torch.isfinite(g).all()), (what, k)
        err, top = (g - r).abs(), float(r.abs().max())
        if k == "g_rgb" and cfg["w_ssim"]:
            worst, tol = float(err.max()), 1e-4 * top
            print(f"{what} {k} {tuple(r.shape)} (SSIM rule): worst error {worst:.3e}, tolerance {tol:.3e} ({worst / max(tol, 1e-300):.3f} of it)")
            assert worst <= tol, (what, k, worst, tol)
        else:
            tol = 1e-4 * r.abs() + 1e-6 * top
            worst = float((err / tol.clamp_min(1e-300)).max()) if top > 0 else float(err.max())
            print(f"{what} {k} {tuple(r.shape)}: worst element {worst:.3f} of its tolerance (largest entry {top:.3e})")
            assert bool((err <= tol).all()), (what, k, worst)
