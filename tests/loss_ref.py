"""Float64 reference of the image-loss tail (emd_image_loss, csrc/loss.hip) and the cases its tests share.  No GPU.  TEST INFRASTRUCTURE ONLY.

`reference(case, ...)` restates S3Gaussian/utils/loss_utils.py:21-98 and train.py:226-363, as documented in oracle/loss_oracle.py, in float64:
    l1_loss + lambda_depth * compute_depth("l2", depth * mask, gt_depth * mask) + lambda_dssim * (1 - ssim) + lambda_sky * sky BCE
It shares no code with the kernel and none with the oracle: the 11x11 window is the outer product of the float32 1-D window the reference's Python
builds (torch.Tensor of math.exp values, normalised in float32), the five convolutions are zero-padded grouped conv2d in float64, the gradients
come from torch autograd in float64.

Every discontinuous decision is taken on the float32 inputs, in float32, exactly as the reference takes it, and enters the float64 arithmetic as a
fixed mask: the valid-depth mask `0.01 < gt_depth * mask < max_depth`, the pass masks of both clamps (torch.clamp hands the gradient on where
min <= x <= max), and sign(image - gt).  The reference and a float32 implementation therefore never disagree about the side of a gate a pixel is
on; the builders below keep every drawn pixel away from the gates (MARGIN) and then place pixels exactly ON them, where the float32 outcome is
exact.  One deviation, which is the kernel's contract (include/emd_raster.h): without a single valid lidar pixel the depth term is 0 with a zero
gradient (the reference's mean over no element is NaN), and a term that is switched off has a zero gradient.

FLOORS holds, per image family and output, the worst error of the reference's own float32 formulation (oracle.loss_oracle.loss_tail on the CPU)
against this reference over every shape of SHAPES.  The kernel's allowance is 4 x that floor, never more than the 1e-4 of the largest entry /
1e-5 relative that tests/test_loss_gpu.py grants: `allowance(family, output)`.  Regenerate the table with
    python -m tests.loss_ref
and paste its output over FLOORS; tests/test_loss_ref_cpu.py asserts that the table is current within a factor of 2."""
import math

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
MARGIN = 1e-5                     # relative distance every DRAWN pixel keeps from a gate (a condition on the inputs, not a tolerance)
MAX_DEPTH = 80.0
DEPTH_LO = F32(0.01)              # the thresholds as float32, the type the reference compares in
W_LO, W_HI = F32(1e-6), F32(1.0 - 1e-6)
LAMBDAS = dict(lambda_dssim=0.2, lambda_depth=0.5, lambda_sky=0.05)

TERMS = ("l1", "ssim", "depth", "sky")
LOSSES = ("total",) + TERMS       # the layout of EmdLossArgs.losses
GRADS = ("g_image", "g_depth", "g_weight")
FAMILIES = ("random", "equal", "blocks", "pixel", "wide")

# (H, W), non-square so that a row / column swap shows
SHAPES = {
    "window": [(1, 1), (1, 40), (40, 1), (5, 7), (10, 11), (11, 10)],              # smaller than the window radius (5) or the window (11)
    "seams": [(32, 32), (33, 31), (31, 65), (64, 33), (35, 97), (37, 43)],         # the 32 x 32 tile, its 42 x 42 halo, four rows per thread
    "block": [(1, 255), (1, 256), (1, 257)],                                       # the 256-pixel block of the point-wise pass
    "slots": [(257, 289)],                                                         # 90 tiles per channel, 291 point-wise blocks: both wrap the 64 slots
}
ALL_SHAPES = [s for group in SHAPES.values() for s in group]
PLACE_MIN = 64                    # a case of at least this many pixels carries the placed rows


def next_up(x):
    return np.nextafter(F32(x), F32(np.inf))


def next_down(x):
    return np.nextafter(F32(x), F32(-np.inf))


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------
def window_2d():
    """loss_utils.py:56-64: gaussian(11, 1.5) as a float32 tensor normalised in float32, its outer product in float32; then widened."""
    g = torch.tensor([math.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().double()


def _ssim64(x, y):
    win = window_2d()[None, None].expand(3, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t[None], win, padding=5, groups=3)[0]
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu12
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))).mean()


def decisions(case, max_depth=MAX_DEPTH):
    """The discontinuous decisions, each in float32 on the float32 inputs (numpy float32 arithmetic is IEEE, as the reference's is)."""
    d = {"sign": np.sign(case["image"] - case["gt"]).astype(np.float64)}
    if case.get("depth") is not None:
        m = case["mask"] if case.get("mask") is not None else np.ones_like(case["depth"])
        pd, gd = case["depth"] * m, case["gt_depth"] * m
        assert pd.dtype == F32 and gd.dtype == F32
        d["valid"] = (gd > DEPTH_LO) & (gd < F32(max_depth))
        pn = pd / F32(max_depth)
        d["pn_pass"], d["pn_const"] = (pn >= 0) & (pn <= 1), np.where(pn > 1, 1.0, 0.0)
    if case.get("weight") is not None:
        w = case["weight"]
        d["w_pass"], d["w_const"] = (w >= W_LO) & (w <= W_HI), np.where(w > W_HI, np.float64(W_HI), np.float64(W_LO))
    return d


def reference(case, lambda_dssim=0.2, lambda_depth=0.5, lambda_sky=0.05, max_depth=MAX_DEPTH, use_depth=True, use_sky=True):
    """-> dict of float64: total, l1, ssim, depth, sky (a term that is not applied is 0.0) and g_image [3,H,W], g_depth [H,W], g_weight [H,W]
    (zeros where the reference applies no term).  `use_depth` / `use_sky` False stand for depth / weight handed over as None."""
    t = lambda k: torch.from_numpy(np.asarray(case[k], np.float64))
    dec = decisions(case, max_depth)
    H, W = case["image"].shape[-2:]
    image, gt = t("image").requires_grad_(True), t("gt")
    out = {k: 0.0 for k in LOSSES}
    out["lambdas"] = (lambda_dssim, lambda_depth if use_depth else 0.0, lambda_sky if use_sky else 0.0)
    l1 = (torch.from_numpy(dec["sign"]) * (image - gt)).mean()                      # |d| = sign(d) d with the sign fixed
    total = l1
    depth = weight = None
    if use_depth and case.get("depth") is not None and lambda_depth != 0:
        depth = t("depth").requires_grad_(True)
        m = t("mask") if case.get("mask") is not None else torch.ones(H, W, dtype=torch.float64)
        valid = torch.from_numpy(dec["valid"])
        if bool(valid.any()):
            pn, gn = depth * m / max_depth, t("gt_depth") * m / max_depth           # gn of a valid pixel lies inside (0, 1): its clamp is the identity
            pcl = torch.where(torch.from_numpy(dec["pn_pass"]), pn, torch.from_numpy(dec["pn_const"]))
            term = ((pcl - gn) ** 2)[valid].mean()
            out["depth"] = term.item()
            total = total + lambda_depth * term
    if lambda_dssim != 0:
        term = _ssim64(image, gt)
        out["ssim"] = term.item()
        total = total + lambda_dssim * (1.0 - term)
    if use_sky and case.get("weight") is not None and lambda_sky > 0 and int(case["sky_mask"].sum()) > 0:
        weight = t("weight").requires_grad_(True)
        w = torch.where(torch.from_numpy(dec["w_pass"]), weight, torch.from_numpy(dec["w_const"]))
        term = torch.where(torch.from_numpy(case["sky_mask"] != 0), -torch.log(1 - w), -torch.log(w)).mean()
        out["sky"] = term.item()
        total = total + lambda_sky * term
    total.backward()
    out["total"], out["l1"] = total.item(), l1.item()
    # a sum is no more accurate than the rounding of its largest summand (the 1 of 1 - ssim among them): what the total's error is relative to
    out["total_scale"] = max(abs(out["total"]), out["l1"], lambda_dssim if lambda_dssim != 0 else 0.0, abs(lambda_depth) * out["depth"],
                             abs(lambda_sky) * out["sky"])
    grad = lambda x, shape: np.zeros(shape) if x is None or x.grad is None else x.grad.numpy()
    out["g_image"], out["g_depth"], out["g_weight"] = grad(image, (3, H, W)), grad(depth, (H, W)), grad(weight, (H, W))
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
def seam_pixels(H, W):
    """Where a single bright pixel probes the tiling: the image corners, both sides of every 32-pixel tile seam, both sides of the first boundary
    between two groups of four rows, and the last pixel a window centred on the first still reaches."""
    ys = sorted({y for y in (0, 3, 4, 5, 31, 32, 63, 64, H - 1) if y < H})
    xs = sorted({x for x in (0, 5, 31, 32, 63, 64, W - 1) if x < W})
    pairs = [(ys[i % len(ys)], xs[(i * 3 + i // len(ys)) % len(xs)]) for i in range(max(len(ys), len(xs)))]
    return sorted(set(pairs + [(0, 0), (H - 1, W - 1), (ys[-1], xs[0]), (ys[0], xs[-1])]))


def _images(family, H, W, rng, pixel=None):
    if family == "random":
        gt = rng.random((3, H, W))
        return np.clip(gt + 0.2 * rng.standard_normal((3, H, W)), 0, 1), gt
    if family == "equal":
        gt = rng.random((3, H, W))
        return gt.copy(), gt
    if family == "blocks":                                     # 6 x 9 blocks of one level each: no variance inside a window that sees one block
        by, bx = np.arange(H) // 6, np.arange(W) // 9
        level = lambda: rng.random((3, H // 6 + 1, W // 9 + 1))[:, by][:, :, bx]
        gt = level()
        return np.where(rng.random((1, H // 6 + 1, W // 9 + 1))[:, by][:, :, bx] < 0.3, gt, level()), gt
    if family == "pixel":                                      # one bright pixel on black; the target's, dimmer, two rows and three columns on
        y, x = pixel if pixel is not None else (H // 2, W // 2)
        image, gt = np.zeros((3, H, W)), np.zeros((3, H, W))
        image[:, y, x] = (1.0, 0.75, 0.5)
        gt[:, (y + 2) % H, (x + 3) % W] = 0.5
        return image, gt
    if family == "wide":                                       # renders are not clamped
        gt = rng.random((3, H, W)) * 1.6 - 0.3
        return gt + 0.5 * rng.standard_normal((3, H, W)), gt
    raise ValueError(family)


def _near(value, t):
    return np.abs(value / t - 1.0) < MARGIN


def build_case(H, W, family="random", seed=0, mask="binary", sky="many", pixel=None, place=True, max_depth=MAX_DEPTH):
    """One case as float32 / uint8 numpy arrays: image, gt [3,H,W]; depth, gt_depth, weight [H,W]; mask [H,W] or None ("none", "binary", or "float":
    values of {0, 0.5, 1, 2}); sky_mask uint8 [H,W] holding "many", "one" or "none" sky pixels.  case["placed"] maps the name of every hand-placed
    row to its flat pixel indices (empty below PLACE_MIN pixels or with place=False)."""
    rng = np.random.default_rng([H, W, FAMILIES.index(family), seed])
    image, gt = (a.astype(F32) for a in _images(family, H, W, rng, pixel))
    md = F32(max_depth)
    gt_depth = (rng.random((H, W)) * 90.0 * (rng.random((H, W)) > 0.4)).astype(F32)
    depth = (gt_depth + 2.0 * rng.standard_normal((H, W))).astype(F32)                  # below 0 and above max_depth both occur
    weight = rng.random((H, W)).astype(F32)
    if H * W >= PLACE_MIN:                                                              # saturated opacities are common in a render.  (Not in an image
        weight[rng.random((H, W)) < 0.1] = 0.0                                          # of a few pixels: a sky pixel of weight 0 contributes
        weight[rng.random((H, W)) < 0.1] = 1.0                                          # -log(1 - 1e-6), which float32 forms 1.3 % off, and would BE the term)
    sky_mask = np.zeros((H, W), np.uint8)
    if sky == "many":
        sky_mask = (rng.random((H, W)) < 0.3).astype(np.uint8)
        sky_mask.flat[0] = 1
    elif sky == "one":
        sky_mask.flat[(H * W) // 2] = 1
    m = None
    if mask == "binary":
        m = (rng.random((H, W)) < 0.7).astype(F32)
    elif mask == "float":
        m = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], F32), (H, W))
    # the margin rule: a drawn pixel inside the margin of a gate is moved, never dropped
    mm = m if m is not None else np.ones((H, W), F32)
    for _ in range(8):
        gd, pn = gt_depth * mm, depth * mm / md
        bad_g = _near(gd, DEPTH_LO) | _near(gd, md)
        bad_p = (gd > DEPTH_LO) & (gd < md) & ((np.abs(pn) < MARGIN) | _near(pn, 1.0))     # the clamp matters on a valid pixel only
        bad_w = ((weight != 0) & (weight != 1)) & (_near(weight, W_LO) | _near(weight, W_HI) | (weight < 1e-3) | (weight > 1 - 1e-3))
        if not (bad_g.any() or bad_p.any() or bad_w.any()):
            break
        gt_depth[bad_g] *= F32(1.001)
        depth[bad_p] += F32(0.01)
        weight[bad_w] = F32(0.5)
    else:
        raise AssertionError("a drawn pixel does not leave the margin")
    case = dict(H=H, W=W, family=family, image=image, gt=gt, depth=depth, gt_depth=gt_depth, mask=m, weight=weight, sky_mask=sky_mask,
                max_depth=float(max_depth), placed={})
    if place and H * W >= PLACE_MIN:
        _place(case, rng, sky == "many")
    return case


DEPTH_ROWS = (  # name, gd (gt_depth * mask), pd (depth * mask), valid?, gradient passes the clamp?
    ("gd == 0.01", lambda md: DEPTH_LO, lambda md: F32(30), False, None),
    ("gd just above 0.01", lambda md: next_up(DEPTH_LO), lambda md: F32(30), True, True),
    ("gd == max_depth", lambda md: md, lambda md: F32(30), False, None),
    ("gd just below max_depth", lambda md: next_down(md), lambda md: F32(30), True, True),
    ("pd == max_depth", lambda md: md / 2, lambda md: md, True, True),
    ("pd == 0", lambda md: md / 2, lambda md: F32(0), True, True),
    ("pd just above max_depth", lambda md: md / 2, lambda md: next_up(md), True, False),
    ("pd below 0", lambda md: md / 2, lambda md: F32(-1), True, False),
)
WEIGHT_ROWS = (  # name, weight, gradient passes the clamp?
    ("w == 1e-6", W_LO, True), ("w == 1 - 1e-6", W_HI, True), ("w just below 1e-6", next_down(W_LO), False),
    ("w just above 1 - 1e-6", next_up(W_HI), False), ("w == 0", F32(0), False), ("w == 1", F32(1), False),
)
L1_ROWS = 5


def _place(case, rng, with_sky):
    """Pixels exactly ON the gates.  Under a float mask the placed pixels take the factors 0.5, 1, 2 in turn and the depths are divided by them:
    a power of two scales exactly, so depth * mask is the stated value bit for bit."""
    H, W = case["H"], case["W"]
    md = F32(case["max_depth"])
    n = len(DEPTH_ROWS) + 2 * len(WEIGHT_ROWS) + L1_ROWS
    free = np.arange(H * W)
    if case["family"] == "pixel":                              # the two bright pixels stay what they are
        free = free[~(case["image"].any(0) | case["gt"].any(0)).ravel()]
    at = iter(rng.choice(free, n, replace=False).tolist())
    placed = case["placed"]
    factors = [F32(1)] if case["mask"] is None or set(np.unique(case["mask"]).tolist()) <= {0.0, 1.0} else [F32(0.5), F32(1), F32(2)]
    for i, (name, gd, pd, _valid, _passes) in enumerate(DEPTH_ROWS):
        p, f = next(at), factors[i % len(factors)]
        if case["mask"] is not None:
            case["mask"].flat[p] = f
        case["gt_depth"].flat[p], case["depth"].flat[p] = gd(md) / f, pd(md) / f
        placed[name] = [p]
    for name, w, _passes in WEIGHT_ROWS:                       # each on a pixel that is not sky and, where the mask has many sky pixels, on one that is
        placed[name] = []
        for is_sky in (0, 1):
            p = next(at)
            case["weight"].flat[p] = w
            if with_sky:
                case["sky_mask"].flat[p] = is_sky
            placed[name].append(p)
    placed["image == gt"] = [next(at) for _ in range(L1_ROWS)]
    for p in placed["image == gt"]:
        for c in range(3):
            case["image"][c].flat[p] = case["gt"][c].flat[p]


def conditions_hold(case):
    """The builders' conditions on a finished case: every drawn pixel keeps MARGIN from every gate, every placed row is what its name says."""
    md = F32(case["max_depth"])
    hand = np.zeros(case["H"] * case["W"], bool)
    for rows in case["placed"].values():
        hand[rows] = True
    free = ~hand.reshape(case["H"], case["W"])
    m = case["mask"] if case["mask"] is not None else np.ones_like(case["depth"])
    gd, pd, w = case["gt_depth"] * m, case["depth"] * m, case["weight"]
    ok = not (free & (_near(gd, DEPTH_LO) | _near(gd, md))).any()
    ok &= not (free & (gd > DEPTH_LO) & (gd < md) & ((np.abs(pd / md) < MARGIN) | _near(pd / md, 1.0))).any()
    ok &= not (free & (w != 0) & (w != 1) & (_near(w, W_LO) | _near(w, W_HI))).any()
    if case["placed"]:
        for name, g, p, _valid, _passes in DEPTH_ROWS:
            (at,) = case["placed"][name]
            ok &= gd.flat[at] == g(md) and pd.flat[at] == p(md)
        for name, value, _passes in WEIGHT_ROWS:
            ok &= all(w.flat[at] == value for at in case["placed"][name])
        ok &= all((case["image"][:, at // case["W"], at % case["W"]] == case["gt"][:, at // case["W"], at % case["W"]]).all()
                  for at in case["placed"]["image == gt"])
    return bool(ok)


def family_cases(family, shapes=None):
    """The cases of one family over the shape list: the mask kinds and sky counts in turn; the single pixel at every seam position of its shape."""
    masks, skies = ("binary", "float", "none"), ("many", "many", "one", "none")
    cases = []
    for H, W in (shapes if shapes is not None else ALL_SHAPES):
        i = ALL_SHAPES.index((H, W))                           # (a shape's cases are the same whichever list asks for them)
        pixels = seam_pixels(H, W)[::1 if H * W < 20000 else 4] if family == "pixel" else [None]      # (the float64 convolutions take 1.5 s there)
        for j, px in enumerate(pixels):
            cases.append(build_case(H, W, family, seed=j, mask=masks[(i + j) % 3], sky=skies[(i + j) % 4], pixel=px))
    return cases


# ---- the float32 floor ---------------------------------------------------------------------------------------------------------------------------
HALF_ULP = 2.0 ** -24            # no float32 result is expected to do better: a measured floor below it counts as this

# worst error of oracle.loss_oracle.loss_tail in float32 on the CPU against reference(), over family_cases(family): terms relative, gradients as a
# fraction of the largest reference entry (GRAD_SCALE below).  Output of `python -m tests.loss_ref`.
FLOORS = {
    "random": {"l1": 1.55e-07, "ssim": 1.32e-07, "depth": 5.57e-07, "sky": 1.16e-07, "g_image": 1.06e-06, "g_depth": 1.27e-06, "g_weight": 7.30e-08},
    "equal": {"l1": 5.96e-08, "ssim": 5.96e-08, "depth": 5.38e-06, "sky": 9.81e-08, "g_image": 5.88e-07, "g_depth": 2.72e-06, "g_weight": 7.30e-08},
    "blocks": {"l1": 1.08e-07, "ssim": 2.00e-06, "depth": 6.18e-07, "sky": 7.76e-08, "g_image": 1.75e-04, "g_depth": 1.14e-06, "g_weight": 7.30e-08},
    "pixel": {"l1": 5.96e-08, "ssim": 1.50e-07, "depth": 1.56e-06, "sky": 1.57e-07, "g_image": 4.75e-07, "g_depth": 1.44e-06, "g_weight": 9.05e-08},
    "wide": {"l1": 8.77e-08, "ssim": 9.55e-08, "depth": 3.20e-07, "sky": 1.91e-07, "g_image": 4.81e-07, "g_depth": 9.10e-07, "g_weight": 7.30e-08},
}


def grad_scale(ref, name):
    """What a gradient's error is a fraction of: the largest entry of the reference, as in tests/test_loss_gpu.py.  dL/dimage of an image that
    EQUALS its target is 0 in exact arithmetic (sign(0) = 0 and SSIM at its maximum): what float64 autograd returns there is its own rounding
    residue and no scale, so the scale is never taken below the L1 gradient's 1 / (3 H W), the largest entry of any image that differs from its
    target in one pixel."""
    s = float(np.abs(ref[name]).max())
    if name == "g_image":
        s = max(s, 1.0 / ref["g_image"].size)
    return s


def errors(got, ref):
    """got, ref: dicts as reference() returns -> {output: error}, terms relative (absolute where the reference is 0), gradients by grad_scale.
    The total has total_error / total_allowance."""
    e = {}
    for k in TERMS:
        e[k] = abs(float(got[k]) - ref[k]) / (abs(ref[k]) if ref[k] != 0 else 1.0)
    for k in GRADS:
        s = grad_scale(ref, k)
        e[k] = float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max()) / s if s > 0 else float(np.abs(got[k]).max())
    return e


def oracle_fp32(case, **lam):
    """oracle.loss_oracle.loss_tail in float32 on the CPU, in the layout of reference()."""
    from oracle import loss_oracle as lo
    H, W = case["H"], case["W"]
    lam = {**LAMBDAS, **lam}
    image = torch.from_numpy(case["image"]).requires_grad_(True)
    depth, weight = torch.from_numpy(case["depth"])[None].requires_grad_(True), torch.from_numpy(case["weight"])[None].requires_grad_(True)
    mask = None if case["mask"] is None else torch.from_numpy(case["mask"])[None]
    valid = decisions(case, case["max_depth"])["valid"]
    with_depth = bool(valid.any())                             # the oracle's mean over no pixel is NaN; the contract says 0
    total, terms = lo.loss_tail(image, torch.from_numpy(case["gt"]), depth if with_depth else None, torch.from_numpy(case["gt_depth"])[None], mask,
                                weight, torch.from_numpy(case["sky_mask"] != 0)[None], **lam)
    total.backward()
    out = {k: float(terms[k].detach()) if k in terms else 0.0 for k in TERMS}
    out["total"] = float(total.detach())
    g = lambda x, shape: np.zeros(shape, F32) if x.grad is None else x.grad.numpy().reshape(shape)
    out["g_image"], out["g_depth"], out["g_weight"] = g(image, (3, H, W)), g(depth, (H, W)), g(weight, (H, W))
    return out


def measure_floors():
    """-> {family: {output: floor}} (single-threaded: a float32 sum's rounding depends on how it is split); "total share" is the oracle's worst
    error of the total as a share of total_allowance under the CURRENT table."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        floors = {}
        for family in FAMILIES:
            worst = {k: HALF_ULP for k in TERMS + GRADS}
            share = 0.0
            for case in family_cases(family):
                got, ref = oracle_fp32(case), reference(case, **LAMBDAS, max_depth=case["max_depth"])
                e = errors(got, ref)
                worst = {k: max(worst[k], e[k]) for k in worst}
                if family in FLOORS:
                    share = max(share, total_error(got, ref) / total_allowance(family, ref))
            floors[family] = {**worst, "total share": share}
        return floors
    finally:
        torch.set_num_threads(threads)


def total_allowance(family, ref):
    """The total is formed from the four terms -- l1 + lambda_dssim (1 - ssim) + lambda_depth depth + lambda_sky sky, four float32 roundings --, so
    its error is theirs: the ABSOLUTE bound is the sum of what the terms are allowed, weighted as the total weights them, and four half-ulps of the
    largest summand; never more than 1e-5 of that summand (test_loss_gpu.py: 1e-5 relative)."""
    ld, lp, ls = ref["lambdas"]
    derived = sum(abs(lam) * allowance(family, k) * abs(ref[k]) for k, lam in zip(TERMS, (1.0, ld, lp, ls)))
    return min(derived + 4 * HALF_ULP * ref["total_scale"], 1e-5 * ref["total_scale"])


def total_error(got, ref):
    return abs(float(got["total"]) - ref["total"])


def allowance(family, output):
    """What the kernel may differ by: 4 x the float32 floor -- its separable window and block-wise sums round differently from the outer-product
    convolution, in the same order of error -- and never more than tests/test_loss_gpu.py grants."""
    return min(4.0 * FLOORS[family][output], 1e-4 if output in GRADS else 1e-5)


if __name__ == "__main__":
    print("FLOORS = {")
    for family, row in measure_floors().items():
        print(f'    "{family}": {{' + ", ".join(f'"{k}": {v:.2e}' for k, v in row.items() if k in TERMS + GRADS) + "},")
    print("}")
