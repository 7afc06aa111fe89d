"""Cases, reference and tolerances of the sky camera-ray tests (SkyCubeMap / composite_s3g: rays built from the camera, 2-D backward tiles).
Not a test: tests/test_sky_cpu.py measures the tolerances and proves that the cases reach their branches, tests/test_sky_gpu.py compares the
HIP path with `reference(case, torch.float64)`.  Both build identical inputs from the case id: everything here is on the CPU.

Reference: oracle/sky_oracle.py (rays, sky_s3g, blend_s3g) in float64 with torch autograd, fed the float32 inputs the kernel gets.

Discontinuities.  The clamp's pass mask 0 <= s <= 1 is a step: a float32 and a float64 evaluation can disagree at a pixel whose unclamped
colour is within rounding of 0 or 1, and then a whole upstream gradient goes to the texels or does not.  `build` marks every sampled pixel whose
unclamped float64 colour has a channel within MARK_BAND of 0 or of 1 and zeroes both upstream gradients there; forward comparisons skip those
pixels.  At most MARK_SHARE of a case's pixels may be marked (test_sky_cpu asserts it).  The sampling mask (1 - acc) > 1e-3 is a step too: no
`acc` lies within ACC_GAP of the threshold.
"""
import functools
import types

import torch

from oracle import sky_oracle as so

UP = (0.1, 0.2, 1.0)
T = (0.3, -1.5, 0.2)
MARK_BAND = 1e-4
MARK_SHARE = 0.005
ACC_GAP = 5e-4
QUANTITIES = ("sky", "out", "d_cube", "d_render", "d_weight")

# id -> H, W, focal, res, fwd.  The smallest shapes at which each branch of k_sky_backward is reached (test_sky_cpu asserts that they are):
#   corner-min  three faces in view, corner taps (3-tap renormalisation), edge taps re-indexed onto the next face
#   corner-64   tiles that straddle a cube edge: window on one face, other lanes' taps on another
#   corner-mag  many pixels per texel: heavy same-cell LDS accumulation, window origin off the face at the corner
#   face-mag    one face, all taps in the window
#   minified    a tile spans more than 24 texels: the out-of-window global atomic carries most of the gradient
#   odd-neg     odd resolution, negative faces
#   row         height == 1 with a camera (1-D indexing together with pixel_ray)
#   two-rows    the smallest 2-D image, ragged tile in both directions
CASES = {
    "corner-min": (45, 70, 40.0, 8, (1.0, 1.0, 1.0)),
    "corner-64": (45, 70, 48.0, 64, (1.0, 1.0, 1.0)),        # (focal 48: at 40 no pixel centre falls into the half-texel corner cell of a 64^2 face)
    "corner-mag": (37, 53, 400.0, 64, (1.0, 1.0, 1.0)),
    "face-mag": (37, 53, 400.0, 256, (1.0, 0.02, 0.01)),
    "minified": (33, 50, 12.0, 128, (1.0, 1.0, 1.0)),
    "odd-neg": (33, 50, 12.0, 5, (-1.0, 1.0, -1.0)),
    "row": (1, 300, 40.0, 16, (1.0, 1.0, 1.0)),
    "two-rows": (2, 37, 40.0, 16, (1.0, 1.0, 1.0)),
}
# the further tests, all on the corner-64 camera: a given jitter draw; camera.sky_mask under is_train (70 x 40 so that rows >= 50 exist);
# SkyCubeMap.forward(cam, acc=acc) without the blend
VARIANTS = {
    "jitter": (45, 70) + CASES["corner-64"][2:],
    "sky-mask": (70, 40) + CASES["corner-64"][2:],
    "no-blend": (45, 70) + CASES["corner-64"][2:],
}
SEED = 200                                 # (two-rows has 74 pixels, of which MARK_SHARE allows none: this draw marks none there)
ZERO_CHANNEL_CASE = "corner-min"          # channel 1 of both upstream gradients is exactly zero there (the gs[c] == 0 skip)

# Largest |float32 oracle - float64 oracle| per quantity on these very inputs, over both backgrounds, marked pixels excluded: what float32 costs the
# reference's own formulas.  test_sky_cpu.test_float32_cost_stays_within_table re-measures it (measured <= entry, and >= entry / 4 so that an entry
# cannot sit loosely above what it stands for).  The GPU bar is BAR_FACTOR x the entry, absolute: the kernel is a float32 evaluation in another
# operation order, with fma contraction and float atomics the CPU float32 run does not have.  No entry comes from the kernel's output.
# Against the older bars of test_sky_gpu.py (colours 2e-5; dL/dcube 1e-4 of its largest entry, here 6 ... 28, so 6e-4 ... 3e-3): every dL/dcube
# bar here is tighter (at most 9.6e-4 where the largest entry is 15).  The colour bars of the res >= 64 cases are looser, up to 9.6e-5: a
# direction carries ~1e-7 of float32 error, u * res multiplies it by res (64 ... 256), and neighbouring texels here differ by up to 1.6 (values in
# [-0.3, 1.3]) where the older test's differ by at most 1.  dL/dweight = sum_c g_c (render_c - sky_c) inherits that error times |g| up to ~9.
BAR_FACTOR = 4.0
TABLE = {
    "corner-min": {"sky": 1.8e-6, "out": 1.6e-6, "d_cube": 2.2e-5, "d_render": 2.4e-7, "d_weight": 5.3e-6},
    "corner-64": {"sky": 1.5e-5, "out": 1.1e-5, "d_cube": 9.9e-5, "d_render": 2.4e-7, "d_weight": 6.1e-5},
    "corner-mag": {"sky": 1.7e-5, "out": 1.4e-5, "d_cube": 2.1e-4, "d_render": 2.3e-7, "d_weight": 7.7e-5},
    "face-mag": {"sky": 2.2e-5, "out": 1.8e-5, "d_cube": 2.4e-4, "d_render": 2.4e-7, "d_weight": 1.1e-4},
    "minified": {"sky": 2.2e-5, "out": 2.0e-5, "d_cube": 1.3e-4, "d_render": 2.4e-7, "d_weight": 1.2e-4},
    "odd-neg": {"sky": 1.4e-6, "out": 8.7e-7, "d_cube": 1.8e-5, "d_render": 2.4e-7, "d_weight": 6.2e-6},
    "row": {"sky": 3.0e-6, "out": 2.9e-6, "d_cube": 3.2e-5, "d_render": 2.3e-7, "d_weight": 7.8e-6},
    "two-rows": {"sky": 2.4e-6, "out": 1.5e-6, "d_cube": 1.4e-5, "d_render": 1.5e-7, "d_weight": 5.7e-6},
    "jitter": {"sky": 1.9e-5, "out": 1.1e-5, "d_cube": 8.1e-5, "d_render": 2.4e-7, "d_weight": 1.3e-4},
    "sky-mask": {"sky": 1.6e-5, "out": 1.6e-5, "d_cube": 9.2e-5, "d_render": 2.4e-7, "d_weight": 5.0e-5},
    "no-blend": {"sky": 1.4e-5, "d_cube": 6.8e-5},
}


def bar(case_id, quantity):
    return BAR_FACTOR * TABLE[case_id][quantity]


def camera(H, W, focal, fwd):
    """(K [3,3], w2c [4,4]) float32: looks along `fwd` with UP up (x right, y down, z forward), translation T, principal point off centre."""
    f = torch.tensor(fwd, dtype=torch.float64)
    f = f / f.norm()
    right = torch.linalg.cross(f, torch.tensor(UP, dtype=torch.float64))
    right = right / right.norm()
    down = torch.linalg.cross(f, right)
    w2c = torch.eye(4, dtype=torch.float64)
    w2c[:3, :3] = torch.stack([right, down, f])
    w2c[:3, 3] = torch.tensor(T, dtype=torch.float64)
    K = torch.tensor([[focal, 0.0, W / 2 + 0.3], [0.0, focal, H / 2 - 0.2], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return K.float(), w2c.float()


def _forced_mask(sky_mask):
    m = sky_mask[0].bool().clone()
    m[:50, :] = True
    return m


@functools.lru_cache(maxsize=None)
def build(case_id, white):
    """The inputs of one case, float32 on the CPU and never modified afterwards: camera (K, w2c), cube, acc [1,H,W], render [3,H,W], jitter
    ([H,W,2] or None), sky_mask ([1,H,W] bool or None), upstream gradients g_out / g_sky [3,H,W] (zero at marked pixels), marked [H,W]."""
    H, W, focal, res, fwd = CASES[case_id] if case_id in CASES else VARIANTS[case_id]
    gen = torch.Generator().manual_seed(SEED + 2 * (list(CASES) + list(VARIANTS)).index(case_id) + int(white))
    K, w2c = camera(H, W, focal, fwd)
    cube = torch.rand(6, res, res, 3, generator=gen) * 1.6 - 0.3               # the clamp and its pass mask act
    acc = torch.rand(1, H, W, generator=gen)
    acc[(acc - (1 - 1e-3)).abs() <= ACC_GAP] = 0.998                               # no value near the sampling threshold
    acc[:, :, :5] = 1.0                                                        # not sampled: a tile's leader is not lane 0
    if H >= 16 and W >= 32:
        acc[:, :16, 16:32] = 1.0                                               # a whole tile contributes nothing: the early return
    render = torch.rand(3, H, W, generator=gen)
    jitter = torch.rand(H, W, 2, generator=gen) if case_id in ("jitter", "sky-mask") else None
    sky_mask = (torch.rand(1, H, W, generator=gen) < 0.5) if case_id == "sky-mask" else None
    g_out, g_sky = torch.randn(3, H, W, generator=gen), torch.randn(3, H, W, generator=gen)
    if case_id == ZERO_CHANNEL_CASE:
        g_out[1] = 0.0
        g_sky[1] = 0.0
    sampled = _forced_mask(sky_mask) if sky_mask is not None else (1 - acc[0].double()) > 1e-3
    dirs = so.rays(H, W, K, w2c[:3, :3], w2c[:3, 3], jitter, dtype=torch.float64)
    col = so.cube_lookup(cube.double(), dirs)                                  # unclamped
    marked = sampled & ((col.abs() < MARK_BAND) | ((col - 1).abs() < MARK_BAND)).any(-1)
    g_out[:, marked] = 0.0
    g_sky[:, marked] = 0.0
    return types.SimpleNamespace(id=case_id, H=H, W=W, res=res, white=bool(white), fill=1.0 if white else 0.0, K=K, w2c=w2c, cube=cube, acc=acc,
                                 render=render, jitter=jitter, sky_mask=sky_mask, g_out=g_out, g_sky=g_sky, marked=marked, sampled=sampled,
                                 blend=case_id != "no-blend")


def loss(out, sky, g_out, g_sky):
    """The scalar both sides differentiate; the factor is a non-unit upstream gradient.  out None: the sky colour alone."""
    s = (sky * g_sky).sum()
    if out is not None:
        s = s + (out * g_out).sum()
    return 2.0 * s


@functools.lru_cache(maxsize=None)
def reference(case_id, white, dtype=torch.float64):
    """The oracle's own functions in `dtype` with torch autograd -> dict of QUANTITIES (CPU tensors of `dtype`; the blend's are absent without it)."""
    c = build(case_id, white)
    cube = c.cube.to(dtype, copy=True).requires_grad_(True)
    render = c.render.to(dtype, copy=True).requires_grad_(True)
    weight = c.acc.to(dtype, copy=True).requires_grad_(True)
    dirs = so.rays(c.H, c.W, c.K, c.w2c[:3, :3], c.w2c[:3, 3], c.jitter, dtype=dtype)
    if c.sky_mask is not None:                       # rows < 50 forced on, threshold 0.5, the fill elsewhere, the blend in torch
        sky = so.sky_s3g(cube, dirs, (1 - _forced_mask(c.sky_mask).to(dtype))[None], fill=c.fill, threshold=0.5)
    else:
        sky = so.sky_s3g(cube, dirs, weight.detach(), fill=c.fill)
    out = so.blend_s3g(render, weight, sky) if c.blend else None
    loss(out, sky, c.g_out.to(dtype), c.g_sky.to(dtype)).backward()
    r = {"sky": sky.detach(), "d_cube": cube.grad}
    if c.blend:
        r.update(out=out.detach(), d_render=render.grad, d_weight=weight.grad)
    return r


def max_diff(got, ref, case, quantity):
    """Largest |got - ref| of one quantity (tensors on the CPU); the forward images without the marked pixels."""
    d = (got.double() - ref.double()).abs()
    if quantity in ("sky", "out"):
        d = d[:, ~case.marked]
    return float(d.max())
