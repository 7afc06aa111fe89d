"""-m gpu: the hot loops of the two render kernels at the shapes where their batch forms, liveness tests and ring reads can go wrong.

K7's 64-lane pixel loop (render_backward_body) walks the live pixel pairs of a batch from a ballot of n_contrib against the batch's shallowest
entry, takes the two n_contrib of a pair from the plane that holds them beside Q, gives lanes without an entry the largest survivor number and
forms its pixel centres from integer sums; K6's drain (k_render_forward_q) reads every array of its LDS ring per entry.  Nothing of that may
change a result: the forward images bit for bit, the gradients within tests/helpers.py's bars.  One 27 x 37 image (6 tiles; neither side a multiple of 8, the width odd: the pixel pair (36, 37) and the
quadrants at x >= 32 and y >= 24 straddle the image edge, so some lanes are outside), every Gaussian anisotropic and rotated (B != 0) and placed by hand:

  quadrant (tile, q)      Gaussians               what it covers
  (0, 0) (0, 3)           65, 64 faint            a full 64-lane batch plus a one-entry deepest batch (half-wave form); exactly one full batch
  (1, 0) (1, 3)           33, 32 faint            a partial 64-lane batch; the largest half-wave batch
  (3, 0)                  1 faint                 the smallest batch
  (2, 0)                  40 faint                the right edge: footprints cross x = 36 | 37, lanes outside the image
  (5, 2)                  10 faint                the corner: right and bottom edge
  (4, 0)                  50 near-opaque          pixels terminate inside the list (n_contrib below the survivor count, the stop test)

"Faint" (opacity 0.05 .. 0.12) keeps every pixel unsaturated, so every survivor up to the deepest contributes and the backward walks all of them; every
footprint stays at least 3 px inside its quadrant, so each quadrant's corner pixels are reached by nothing (n_contrib == 0) and no other quadrant sees
its Gaussians.  The premises are proved from the oracle's own output on the CPU.  Cases: the normal image on, off, and one extra colour set, so every
ring array and every instantiation's layout is read."""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_oracle as co
from tests.helpers import (IMAGE_TOL, assert_grad_close, compare_backward, compare_forward, make_case, run_hip, run_oracle, run_oracle_extra_sets)

H, W = 27, 37
# (tile, quadrant, Gaussians, opacity range, exact): `exact` -- the premise pins the number of entries the backward walks to the count
GROUPS = [(0, 0, 65, (0.05, 0.12), True), (0, 3, 64, (0.05, 0.12), True), (1, 0, 33, (0.05, 0.12), True), (1, 3, 32, (0.05, 0.12), True),
          (3, 0, 1, (0.05, 0.12), True), (2, 0, 40, (0.05, 0.12), False), (5, 2, 10, (0.05, 0.12), False), (4, 0, 50, (0.85, 0.95), False)]
N = sum(g[2] for g in GROUPS)
GX = (W + 15) // 16


def _origin(tile, q):
    return (tile % GX) * 16 + (q & 1) * 8, (tile // GX) * 16 + (q >> 1) * 8


def _scene():
    case = make_case(n=N, H=H, W=W, seed=41, normal_loss=True)
    rng = np.random.default_rng(4100)
    cam = case["cam"]
    V, c = cam.world_view_transform.float(), cam.camera_center.float()
    px, py, op = np.zeros(N), np.zeros(N), np.zeros(N)
    at = 0
    for tile, q, k, (lo, hi), _ in GROUPS:
        x0, y0 = _origin(tile, q)
        # centres 3 .. 5 px inside the quadrant; at the image edges as far inside as the image goes (the footprints then cross the edge)
        px[at:at + k] = np.minimum(x0 + rng.uniform(3.0, 5.0, k), W - 1.0 - rng.uniform(0.0, 1.5, k))
        py[at:at + k] = np.minimum(y0 + rng.uniform(3.0, 5.0, k), H - 1.0 - rng.uniform(0.0, 1.5, k))
        op[at:at + k] = rng.uniform(lo, hi, k)
        at += k
    z = rng.permutation(np.linspace(2.0, 6.0, N))                  # distinct depths, every group spread over the whole range
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    px, py, z = t(px), t(py), t(z)
    x = z * cam.tanfovx * ((2 * px + 1) / W - 1)
    y = z * cam.tanfovy * ((2 * py + 1) / H - 1)
    case["means3D"] = c[None] + z[:, None] * V[:3, 2][None] + x[:, None] * V[:3, 0][None] + y[:, None] * V[:3, 1][None]
    # 0.35 .. 0.7 px per axis under the case's random rotations: anisotropic, rotated, and never wider than 0.7 px in any direction
    case["scales"] = t(rng.uniform(0.35, 0.7, (N, 3))) * (z * 2 * cam.tanfovx / W)[:, None]
    case["opacities"] = t(op)[:, None]
    return case


def _variant(case, variant, seed=7):
    """-> (case, extra colour sets, their image gradients)"""
    if variant == "no-normal":
        case = dict(case, flags=case["flags"] & ~co.F_NORMAL, dL_dnormal=None)
    if variant == "extra1":
        g = torch.Generator().manual_seed(seed)
        return case, [torch.rand(case["N"], 3, generator=g)], [torch.randn(3, H, W, generator=g).numpy()]
    return case, [], []


@functools.lru_cache(maxsize=None)
def _reference(variant):
    """The oracle's result of a variant, computed once and shared (never modified)."""
    case, feats, dX = _variant(_scene(), variant)
    orc = run_oracle_extra_sets(case, feats, dX) if feats else run_oracle(case, backward=True)
    return case, feats, dX, orc


def _quadrant_walk(orc, tile, q):
    """From the oracle's projection and sorted list alone, in float64: for the pixels of quadrant q of a tile that lie inside the image ->
    (entries of the tile's list that pass the skip tests at some pixel, those that do so at a pixel that has not terminated yet, whether the deepest
    of the former is among the latter, pixels nothing reaches, pixels that terminate inside the list)."""
    pre, b = orc["pre"], orc["bin"]
    s, e = (int(v) for v in b["ranges"][tile])
    ids = b["ids"][s:e].astype(np.int64)
    xy = pre["means2D"][ids].astype(np.float64)
    con = pre["conic_opacity"][ids].astype(np.float64)
    x0, y0 = _origin(tile, q)
    pxs, pys = x0 + np.arange(8), y0 + np.arange(8)
    inside = (pys[:, None] < H) & (pxs[None, :] < W)
    dx = xy[None, None, :, 0] - pxs[None, :, None]
    dy = xy[None, None, :, 1] - pys[:, None, None]
    power = -0.5 * (con[:, 0] * dx * dx + con[:, 2] * dy * dy) - con[:, 1] * dx * dy
    alpha = np.minimum(0.99, con[:, 3] * np.exp(np.minimum(power, 0.0)))
    reach = (power <= 0) & (alpha >= 1.0 / 255.0) & inside[:, :, None]
    T = np.cumprod(1.0 - np.where(reach, alpha, 0.0), axis=2)
    hit = reach & (T < 1e-4)
    stop = np.where(hit.any(2), hit.argmax(2), e - s)
    used = reach & (np.arange(e - s)[None, None, :] < stop[:, :, None])
    reaching, contributing = reach.any((0, 1)), used.any((0, 1))
    deepest_used = bool(reaching.any() and contributing[np.flatnonzero(reaching)[-1]])
    return int(reaching.sum()), int(contributing.sum()), deepest_used, int((inside & ~reach.any(2)).sum()), int((hit.any(2)).sum())


def test_the_scene_takes_every_batch_form():
    """CPU only (the oracle): the premise of the GPU cases below."""
    orc = _reference("normal")[3]
    pre = orc["pre"]
    assert int((pre["radii"] > 0).sum()) == N
    assert float(np.abs(pre["conic_opacity"][:, 1]).min()) > 0.0 and float(np.abs(pre["conic_opacity"][:, 1]).max()) > 0.1      # B != 0: rotated footprints
    for tile, q, k, _, exact in GROUPS:
        reaching, contributing, deepest_used, untouched, terminated = _quadrant_walk(orc, tile, q)
        if exact:
            # exactly k entries reach the quadrant, all of them contribute, no pixel terminates: the backward walks k survivors
            assert (reaching, contributing, deepest_used, terminated) == (k, k, True, 0), (tile, q, reaching, contributing, deepest_used, terminated)
            assert untouched >= 4, f"quadrant ({tile}, {q}): {untouched} pixels with n_contrib == 0"
        else:
            assert reaching >= k and contributing >= 1, (tile, q, reaching, contributing)
    # the edge quadrants hold pixels outside the image and entries that reach their last inside column / row
    assert _origin(2, 0)[0] + 8 > W and _origin(5, 2)[1] + 8 > H and W % 2 == 1 and W % 8 and H % 8
    # the near-opaque pile: pixels terminate before the list ends, others of the same quadrant never do
    _, _, _, untouched, terminated = _quadrant_walk(orc, 4, 0)
    assert terminated >= 4 and untouched >= 4, (terminated, untouched)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["normal", "no-normal", "extra1"])
def test_batch_forms_and_image_edges_against_the_oracle(variant):
    case, feats, dX, orc = _reference(variant)
    hip = run_hip(case, backward=True, colors_extra=feats or None, dL_dextra=dX or None)
    compare_forward(hip, orc, tol=IMAGE_TOL)            # keys, ids, colour, depth, alpha, normal: bit for bit
    checked = compare_backward(hip, orc)
    assert "means3D" in checked and "opacities" in checked and "scales" in checked
    for k, of in enumerate(orc.get("extra", [])):
        nz = int((hip["extra"][k].view(np.uint32) != of["img"]["color"].view(np.uint32)).sum())
        assert nz == 0, f"extra image {k}: {nz} values differ from the oracle's"
        assert_grad_close(hip["render_grads"][f"rgb_extra{k}"], of["grads"]["render_grads"]["rgb"], f"render:rgb_extra{k}")
        assert_grad_close(hip["grads"]["colors_extra"][k], of["grads"]["colors"], f"colors_extra[{k}]")
    if variant == "no-normal":
        assert not hip["normal"].any()
