"""The two contracts of csrc/vanilla.hip in plain torch, fp64 on the CPU: the per-class dictionary of VanillaGaussians.get_gaussians
(OmniRe/models/gaussians/vanilla.py:378-414) and the regularisers of its compute_reg_loss, exactly as include/emd_raster.h states them at
EmdVanillaArgs and EmdVanillaRegArgs.  The reference's own files are not available to record a golden from, so this restatement IS the pinned
contract, in the manner of tests/skinning_ref.py and tests/trainer_loss_ref.py.  It shares no code with the kernels: the
SH colour is `sh_ref.sh_colour` (the reference's polynomial, pinned by tests/golden/s3g_sh.npz), autograd supplies the gradients, and the tie rules
of the regularisers are explicit index selections, not whatever torch.amax / torch.min do in the installed version.

Every function takes a `dtype`: float64 is the reference, float32 the same formula at the kernels' precision (tests/test_vanilla_gaussians_cpu.py
holds it to the same criteria, so a later GPU failure is the kernel's, not the formula's).  `criterion` is tests/skinning_ref.criterion (DESIGN.md
section 5), imported and never restated; scalars are held to relative 1e-5, plane_reg_ref.criterion's rule for loss terms.

Inputs are fp32 tensors built from fixed seeds and are cached together with their references: treat both as read-only."""
import functools

import torch
import torch.nn.functional as F

from emd_amd import _lib as L
from tests.sh_ref import CLAMP_MARGIN, SH_COUNTS, SH_DEG_ROWS, sh_colour
from tests.skinning_ref import criterion  # noqa: F401  (the bar of every comparison: imported, never restated)

F64 = torch.float64
INTERVAL = 1000
CHUNK = L.VANILLA_REG_CHUNK

# ---- the dictionary --------------------------------------------------------------------------------------------------------------------
# (sh_degree, step, M): the class's degree, the training step (n = min(step // INTERVAL, sh_degree)) and the coefficient rows of
# [features_dc, features_rest].  The sh-mode entries give every (n, M) of sh_ref.SH_DEG_ROWS; sh_degree 0 is dc mode (with and without rest rows).
DICT_CONFIGS = ((1, 0, 1), (3, 0, 16), (1, 1000, 4), (3, 1000, 16), (2, 5000, 9), (3, 2000, 16), (3, 3000, 16), (0, 0, 1), (0, 0, 4))
DICT_COUNTS = SH_COUNTS                                                                   # 1, 255, 256, 257, 1000: the block seams; four blocks
DICT_CASES = tuple(cfg + (N,) for cfg in DICT_CONFIGS for N in DICT_COUNTS)
NUDGE = 0.01                                                                              # what an offending features_dc entry moves by
assert tuple(sorted({(min(s // INTERVAL, d), M) for d, s, M in DICT_CONFIGS if d > 0})) == tuple(sorted(SH_DEG_ROWS))


def _gen(seed):
    g = torch.Generator().manual_seed(seed)
    return (lambda *s: torch.rand(*s, generator=g, dtype=F64)), (lambda *s: torch.randn(*s, generator=g, dtype=F64)), g


def pre_colour(c, dtype=F64, dc=None, rest=None):
    """The SH colour in front of + 0.5 and the clamp (sh mode)."""
    dc = c["features_dc"] if dc is None else dc
    rest = c["features_rest"] if rest is None else rest
    coeffs = torch.cat((dc[:, None, :].to(dtype), rest.to(dtype)), dim=1)
    return sh_colour(c["n"], coeffs, c["means"].to(dtype) - c["camera_center"].to(dtype), dtype)


@functools.lru_cache(maxsize=None)
def dict_case(sh_degree, step, M, N):
    """The arguments of nodes.vanilla_gaussians and an upstream gradient per output.  An element of pre + 0.5 within CLAMP_MARGIN of 0 or 1 has
    its features_dc entry moved by NUDGE (repeatedly, should it land on the other edge): nothing is left out of a comparison."""
    r, n, _ = _gen(17000 + 1000 * sh_degree + 10 * M + step // INTERVAL + 7 * N)
    f = lambda t: t.float().contiguous()
    c = dict(sh_degree=sh_degree, step=step, M=M, N=N, n=min(step // INTERVAL, sh_degree), sh_mode=sh_degree > 0,
             means=f(0.5 * n(N, 3)), quats=f(n(N, 4)), opacity_logits=f(n(N, 1)), log_scales=f(0.3 * n(N, 3) - 1.0), features_dc=f(n(N, 3)),
             features_rest=f(n(N, M - 1, 3)), camera_center=f(6.0 * F.normalize(n(3), dim=-1)),
             g_opacities=f(n(N, 1)), g_rgbs=f(n(N, 3)), g_scales=f(n(N, 3)), g_quats=f(n(N, 4)))
    c["K"] = (c["n"] + 1) ** 2
    c["nudged"] = 0
    if c["sh_mode"]:
        for _ in range(20):
            v = pre_colour(c) + 0.5
            bad = (v.abs() < 2 * CLAMP_MARGIN) | ((v - 1).abs() < 2 * CLAMP_MARGIN)
            if not bool(bad.any()):
                break
            c["features_dc"] = (c["features_dc"].double() + NUDGE * bad).float()
            c["nudged"] += int(bad.sum())
    return c


def dictionary(c, dtype=F64):
    """Outputs and the five gradients of L = sum(output * upstream) in `dtype`."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    q, a, l, dc, rest = (leaf(c[k]) for k in ("quats", "opacity_logits", "log_scales", "features_dc", "features_rest"))
    opac, scales = torch.sigmoid(a), torch.exp(l)
    quats = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    pre = None
    if c["sh_mode"]:
        pre = pre_colour(c, dtype, dc, rest)
        rgbs = torch.clamp(pre + 0.5, 0.0, 1.0)
    else:
        rgbs = torch.sigmoid(dc)
    loss = sum((o * c[g].to(dtype)).sum() for o, g in ((opac, "g_opacities"), (scales, "g_scales"), (quats, "g_quats"), (rgbs, "g_rgbs")))
    grads = torch.autograd.grad(loss, (q, a, l, dc, rest), allow_unused=True)
    zero = lambda g, t: torch.zeros_like(t) if g is None else g
    return dict(_opacities=opac.detach(), _scales=scales.detach(), _quats=quats.detach(), _rgbs=rgbs.detach(), pre=None if pre is None else pre.detach(),
                d_quats=zero(grads[0], q), d_opacity_logits=zero(grads[1], a), d_log_scales=zero(grads[2], l), d_features_dc=zero(grads[3], dc),
                d_features_rest=zero(grads[4], rest))


@functools.lru_cache(maxsize=None)
def dict_reference(sh_degree, step, M, N, dtype=F64):
    return dictionary(dict_case(sh_degree, step, M, N), dtype)


def compare(got, ref, what):
    """`criterion`; an empty tensor (features_rest at M = 1) has only its shape to compare."""
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    if ref.numel():
        criterion(got, ref, what)


OUTPUTS = ("_opacities", "_scales", "_quats", "_rgbs")
GRADS = ("d_quats", "d_opacity_logits", "d_log_scales", "d_features_dc", "d_features_rest")


# ---- the regularisers ------------------------------------------------------------------------------------------------------------------
TERMS = ("sharp_shape", "flatten", "sparse", "max_s_square")
RATIO = 10.0
WEIGHTS = dict(w_sharp=0.7, w_flatten=0.3, w_sparse=0.05, w_max_s_square=1.3)               # four distinct weights
WEIGHT_SETS = {"sharp": ("w_sharp",), "flatten": ("w_flatten",), "sparse": ("w_sparse",), "max_s_square": ("w_max_s_square",), "all": tuple(WEIGHTS)}
UPSTREAM = (0.37, 1.0, -2.0, 0.0)                                                          # the upstream scalar of each term
REG_COUNTS = (CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17, 300_000)                       # the chunk seams; more chunks than the finalize workgroup has lanes
EDGE_LOGITS = (-20.0, -13.9, -13.7, 0.0, 13.7, 13.9, 20.0)                                # the clip of sigmoid at 1e-6 is |a| = 13.8155
REG_CASES = tuple(f"n{N}" for N in REG_COUNTS) + ("ties", "edges_all", "edges_none", "edges_one")
GAP = 1e-3


def weights(name):
    return dict({k: (v if k in WEIGHT_SETS[name] else 0.0) for k, v in WEIGHTS.items()}, max_gauss_ratio=RATIO)


@functools.lru_cache(maxsize=None)
def reg_case(name):
    """log_scales [N,3], opacity_logits [N,1], radii [N] int32.
    n<N>: l = 0.9 randn - 1 (about 16 % of the ratios above RATIO), a = 3 randn, 60 % visible.  A ratio within 2 GAP of RATIO has the log-scale
    of its smallest column lowered by 0.01 (the ratio moves by 1 %).
    ties: every pattern of equal columns in every position -- all three equal; two equal largest with a ratio above and below RATIO; two equal
    smallest likewise -- on top of 40 random rows.
    edges_*: a = EDGE_LOGITS repeated, inside and outside the clip; all rows visible, none, or one (a row outside the clip)."""
    f = lambda t: t.float().contiguous()
    if name.startswith("n"):
        N = int(name[1:])
        r, n, g = _gen(23000 + N)
        l = f(0.9 * n(N, 3) - 1.0)
        for _ in range(20):
            s = torch.exp(l.double())
            ratio = s.amax(-1) / s.amin(-1)
            bad = (ratio - RATIO).abs() < 2 * GAP
            if not bool(bad.any()):
                break
            rows = bad.nonzero().reshape(-1)
            l[rows, s.argmin(-1)[rows]] -= 0.01
        radii = (torch.randint(1, 40, (N,), generator=g) * (r(N) < 0.6)).to(torch.int32)
        return dict(N=N, log_scales=l, opacity_logits=f(3.0 * n(N, 1)), radii=radii)
    r, n, g = _gen(29000 + REG_CASES.index(name))
    if name == "ties":
        rows = []
        for big, small in ((1.5, -2.0), (0.5, -1.0)):                                     # e^3.5 = 33 > RATIO, e^1.5 = 4.5 < RATIO
            for p in range(3):
                two_max, two_min = [big] * 3, [small] * 3
                two_max[p], two_min[p] = small, big
                rows += [two_max, two_min]
        rows += [[0.3, 0.3, 0.3], [-2.5, -2.5, -2.5]]
        l = torch.cat([torch.tensor(rows, dtype=F64), 0.9 * n(40, 3) - 1.0])
        N = l.shape[0]
        return dict(N=N, log_scales=f(l), opacity_logits=f(3.0 * n(N, 1)), radii=(torch.randint(1, 40, (N,), generator=g) * (r(N) < 0.6)).to(torch.int32))
    a = torch.tensor(EDGE_LOGITS * 3, dtype=F64).reshape(-1, 1)
    N = a.shape[0]
    radii = torch.zeros(N, dtype=torch.int32)
    if name == "edges_all":
        radii += 5
    elif name == "edges_one":
        radii[EDGE_LOGITS.index(13.9)] = 3
    return dict(N=N, log_scales=f(0.9 * n(N, 3) - 1.0), opacity_logits=f(a), radii=radii)


def _first(eq):
    """[N,3] bool with a true entry per row -> the lowest true column."""
    return torch.where(eq[:, 0], 0, torch.where(eq[:, 1], 1, 2))


def regulation(c, w, dtype=F64, upstream=UPSTREAM, use_logits=True, use_radii=True):
    """terms [4] (weighted) and the gradients of sum_k upstream[k] terms[k].  Skipped terms are 0 with no gradient."""
    l = c["log_scales"].detach().to(dtype).clone().requires_grad_(True)
    a = c["opacity_logits"].detach().to(dtype).clone().requires_grad_(True)
    s = torch.exp(l)
    hi, lo = s.detach().max(-1, keepdim=True).values, s.detach().min(-1, keepdim=True).values
    is_max, is_min = s.detach() == hi, s.detach() == lo
    zero = l.sum() * 0
    terms = [zero, zero, zero, zero]
    if w["w_sharp"] != 0:                                                                  # equal columns share: the mean of the equal columns IS amax / amin
        smax, smin = (s * is_max).sum(-1) / is_max.sum(-1), (s * is_min).sum(-1) / is_min.sum(-1)
        ratio = smax / smin
        R = torch.tensor(w["max_gauss_ratio"], dtype=dtype)
        terms[0] = w["w_sharp"] * torch.where(ratio > R, ratio - R, torch.zeros_like(ratio)).mean()
    if w["w_flatten"] != 0:                                                                # the lowest of equal columns takes all
        smin = s.gather(1, _first(is_min)[:, None])[:, 0]
        terms[1] = w["w_flatten"] * torch.where(smin < 30.0, smin, torch.full_like(smin, 30.0)).abs().mean()
    if w["w_max_s_square"] != 0:
        smax = s.gather(1, _first(is_max)[:, None])[:, 0]
        terms[3] = w["w_max_s_square"] * (smax ** 2).mean()
    if w["w_sparse"] != 0 and use_logits and use_radii:
        V = c["radii"] > 0
        if int(V.sum()) > 0:
            # 1 - o is sigmoid(-a) and ln(1 - x) is log1p(-x): the same function of a, written so that the fp32 run does not lose the small side
            av = a.reshape(-1)[V]
            o, om = torch.clamp(torch.sigmoid(av), 1e-6, 1 - 1e-6), torch.clamp(torch.sigmoid(-av), 1e-6, 1 - 1e-6)
            ln_o, ln_om = torch.where(av > 0, torch.log1p(-om), torch.log(o)), torch.where(av > 0, torch.log(om), torch.log1p(-o))
            terms[2] = w["w_sparse"] * (-(o * ln_o + om * ln_om)).mean()
    terms = torch.stack(terms)
    gl, ga = torch.autograd.grad((terms * torch.tensor(upstream, dtype=dtype)).sum(), (l, a), allow_unused=True)
    return dict(terms=terms.detach(), d_log_scales=torch.zeros_like(l) if gl is None else gl, d_opacity_logits=torch.zeros_like(a) if ga is None else ga)


def sparse_gradient(c, w, dtype=F64, upstream=UPSTREAM):
    """dL/dopacity_logits in the closed form the contract states: -a o (1 - o) / |V| inside the clip, 0 outside and off V, with o (1 - o) formed
    as sigmoid(a) sigmoid(-a).  (Autograd in fp32 goes through torch's sigmoid backward, o * (1 - o) with a rounded o: 3 % off at |a| = 13.7.)"""
    a = c["opacity_logits"].to(dtype)
    out = torch.zeros_like(a)
    V = c["radii"] > 0
    if w["w_sparse"] != 0 and int(V.sum()) > 0:
        av = a.reshape(-1)
        o, om = torch.sigmoid(av), torch.sigmoid(-av)
        inside = (torch.minimum(o, om) >= 1e-6) & V
        out = (torch.where(inside, -av * (o * om), torch.zeros_like(av)) * (upstream[2] * w["w_sparse"] / int(V.sum()))).reshape(a.shape)
    return out


@functools.lru_cache(maxsize=None)
def reg_reference(name, wname, dtype=F64):
    return regulation(reg_case(name), weights(wname), dtype)


def scalar_criterion(got, ref, what):
    """Relative 1e-5 per term (plane_reg_ref.criterion's rule for scalars); a term whose reference is 0 must be 0."""
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for k, (g, r) in enumerate(zip(got.tolist(), ref.tolist())):
        err, tol = abs(g - r), 1e-5 * abs(r)
        print(f"{what} {TERMS[k] if len(got) == 4 else k}: got {g:.9e} ref {r:.9e} |err| {err:.3e} tol {tol:.3e}")
        assert err <= tol, (what, k, g, r)
