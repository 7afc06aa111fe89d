"""-m gpu: K6 leaves a round's drain as soon as nothing can change any more, and queues nothing for 4x4 sub-blocks whose pixels are all done.

k_render_forward_q ends the drain loop of a scan -> cull -> drain round when no lane is both live and in a row (= sub-block) that still holds an
entry, and appends an entry only to the byte lists of sub-blocks with a live pixel.  Neither may change an output: images bit for bit, and -- through
the survivor numbering, n_contrib and quad_need that the backward walks -- the gradients.  The scenes are built so that both paths are taken, and each
proves that from the oracle's own output, on the CPU (a scene that does not is a broken test):

  stack  32 x 32, 4 tiles.  180 faint and then 250 near-opaque Gaussians, each wider than a tile, in front of 1570 small ones: every pixel terminates a few
         entries into the opaque ones, i.e. past the 128 entries of the first round and hundreds of entries before its tile's list ends.
  pile   48 x 32, 6 tiles.  800 small opaque Gaussians piled on ONE 4x4 sub-block of tile 0's first quadrant, faint ones on the other three, then 40
         that close the whole quadrant, small ones everywhere: the sub-block is done hundreds of entries before its quadrant, and after that more
         entries reach it than any other sub-block (its list would have been the longest of every later round).  The last tile is the control:
         quadrants in which no pixel terminates at all.

Cases: the normal image on (k_render_forward_q<true, 0>), off (<false, 0>) and one extra colour set (<true, 1>), each with the default list and with
keep_all_pairs.  Bars: tests/helpers.py's, unchanged (compare_forward: keys / ids / images bit-exact; compare_backward: render backward, projection
backward on the kernel's own render gradients, end to end)."""
import functools

import numpy as np
import pytest
import torch

from oracle import cpu_oracle as co
from tests.helpers import (IMAGE_TOL, assert_grad_close, compare_backward, compare_forward, make_case, run_hip, run_oracle, run_oracle_extra_sets)

N = 2000


def _place(case, idx, px, py, z, sigma_px, opacity):
    """Put the Gaussians `idx` at pixel (px, py) and view depth z, isotropic, `sigma_px` pixels wide on screen."""
    cam = case["cam"]
    V, c = cam.world_view_transform.float(), cam.camera_center.float()
    f = lambda a: torch.as_tensor(np.broadcast_to(np.asarray(a, np.float32), (len(idx),)).copy())
    px, py, z, sigma_px, opacity = f(px), f(py), f(z), f(sigma_px), f(opacity)
    x = z * cam.tanfovx * ((2 * px + 1) / case["W"] - 1)
    y = z * cam.tanfovy * ((2 * py + 1) / case["H"] - 1)
    case["means3D"][idx] = c[None] + z[:, None] * V[:3, 2][None] + x[:, None] * V[:3, 0][None] + y[:, None] * V[:3, 1][None]
    case["scales"][idx] = (sigma_px * z * 2 * cam.tanfovx / case["W"])[:, None].expand(-1, 3)
    case["opacities"][idx] = opacity[:, None]


def _scene(name):
    rng = np.random.default_rng(2024)
    u = lambda lo, hi, k: rng.uniform(lo, hi, k)
    if name == "stack":
        case = make_case(n=N, H=32, W=32, seed=31)
        _place(case, np.arange(0, 180), u(0, 32, 180), u(0, 32, 180), np.linspace(2.0, 3.0, 180), 12.0, u(0.02, 0.04, 180))
        _place(case, np.arange(180, 430), u(0, 32, 250), u(0, 32, 250), np.linspace(3.0, 5.0, 250), 10.0, u(0.9, 0.99, 250))
        k = N - 430
        _place(case, np.arange(430, N), u(-2, 34, k), u(-2, 34, k), u(5.0, 9.0, k), u(0.7, 1.5, k), u(0.05, 0.5, k))
    else:
        case = make_case(n=N, H=32, W=48, seed=32)
        _place(case, np.arange(0, 800), u(0, 3, 800), u(0, 3, 800), np.linspace(2.0, 6.0, 800), 0.5, u(0.85, 0.95, 800))
        _place(case, np.arange(800, 950), u(0, 8, 150), u(0, 8, 150), u(2.0, 6.0, 150), 2.0, u(0.01, 0.02, 150))
        _place(case, np.arange(950, 990), u(2.5, 4.5, 40), u(2.5, 4.5, 40), np.linspace(6.5, 7.0, 40), 4.0, 0.95)
        k = N - 990
        _place(case, np.arange(990, N), u(-2, 50, k), u(-2, 34, k), u(2.0, 9.0, k), u(0.7, 1.5, k), u(0.05, 0.3, k))
    return case


def _variant(case, variant, seed=5):
    """-> (case, extra colour sets, their image gradients)"""
    if variant == "no-normal":
        case = dict(case, flags=case["flags"] & ~co.F_NORMAL)
    if variant == "extra1":
        g = torch.Generator().manual_seed(seed)
        return case, [torch.rand(case["N"], 3, generator=g)], [torch.randn(3, case["H"], case["W"], generator=g).numpy()]
    return case, [], []


@functools.lru_cache(maxsize=None)
def _reference(scene, variant):
    """The oracle's result of a (scene, variant), computed once and shared by the pair modes (never modified)."""
    case, feats, dX = _variant(_scene(scene), variant)
    orc = run_oracle_extra_sets(case, feats, dX) if feats else run_oracle(case, backward=True)
    return case, feats, dX, orc


def _termination(orc, tile):
    """From the oracle's projection and sorted list alone: (L, stop[16, 16], reach[16, 16, L]) of a tile -- the length of its list, per pixel the position
    in it of the entry at which the pixel terminates (T (1 - alpha) < 1e-4; L where it never does), and whether entry k passes the skip tests at the pixel
    (power <= 0, alpha >= 1/255).  float64 re-evaluation of the compositing rule: a position can be off by one against the fp32 oracle, which the
    premises below leave room for."""
    pre, b, S = orc["pre"], orc["bin"], orc["S"]
    gx = (S.W + 15) // 16
    s, e = (int(v) for v in b["ranges"][tile])
    ids = b["ids"][s:e].astype(np.int64)
    xy = pre["means2D"][ids].astype(np.float64)
    con = pre["conic_opacity"][ids].astype(np.float64)
    px = (tile % gx) * 16 + np.arange(16, dtype=np.float64)
    py = (tile // gx) * 16 + np.arange(16, dtype=np.float64)
    dx = xy[None, None, :, 0] - px[None, :, None]
    dy = xy[None, None, :, 1] - py[:, None, None]
    power = -0.5 * (con[:, 0] * dx * dx + con[:, 2] * dy * dy) - con[:, 1] * dx * dy
    alpha = np.minimum(0.99, con[:, 3] * np.exp(np.minimum(power, 0.0)))
    reach = (power <= 0) & (alpha >= 1.0 / 255.0)
    T = np.cumprod(1.0 - np.where(reach, alpha, 0.0), axis=2)
    hit = reach & (T < 1e-4)
    stop = np.where(hit.any(2), hit.argmax(2), e - s)
    return e - s, stop, reach


def _quadrant(a, q):
    return a[(q >> 1) * 8:(q >> 1) * 8 + 8, (q & 1) * 8:(q & 1) * 8 + 8]


def _subblock(a, r):
    return a[(r >> 1) * 4:(r >> 1) * 4 + 4, (r & 1) * 4:(r & 1) * 4 + 4]


def _premise_stack(orc):
    """Every quadrant of every tile saturates: past the first round's 128 entries (mid-drain of a later round), long before its list ends."""
    for tile in range(4):
        L, stop, _ = _termination(orc, tile)
        for q in range(4):
            end = int(_quadrant(stop, q).max())
            assert 128 < end < L - 64, f"tile {tile} quadrant {q}: its last pixel terminates at entry {end} of {L}"


def _premise_pile(orc):
    """Tile 0, quadrant 0: sub-block 0 is done at least 256 entries (two rounds and more) before the quadrant, the quadrant before the list ends, and of
    the entries between the two more reach sub-block 0 than any other sub-block.  Last tile: quadrants in which no pixel ever terminates."""
    L, stop, reach = _termination(orc, 0)
    qs, qr = _quadrant(stop, 0), _quadrant(reach, 0)
    sub_end, quad_end = int(_subblock(qs, 0).max()), int(qs.max())
    assert sub_end + 256 <= quad_end < L - 64, f"sub-block done at entry {sub_end}, quadrant at {quad_end}, list of {L}"
    later = [int(_subblock(qr, r)[:, :, sub_end + 1:quad_end].any((0, 1)).sum()) for r in range(4)]
    assert later[0] > 1.5 * max(later[1:]), f"entries that reach each sub-block after sub-block 0 is done: {later}"
    L, stop, reach = _termination(orc, 5)
    alive = [q for q in range(4) if int(_quadrant(stop, q).min()) == L]
    assert L > 128 and alive, f"control tile: list of {L}, quadrants without a terminated pixel: {alive}"


@pytest.mark.parametrize("scene", ["stack", "pile"])
def test_the_scenes_take_the_new_paths(scene):
    """CPU only (the oracle): the premise of every GPU case below."""
    orc = _reference(scene, "normal")[3]
    (_premise_stack if scene == "stack" else _premise_pile)(orc)
    assert N == orc["pre"]["radii"].shape[0] and int((orc["pre"]["radii"] > 0).sum()) > 0.9 * N


@pytest.mark.gpu
@pytest.mark.parametrize("keep_all_pairs", [False, True], ids=["default-list", "keep-all-pairs"])
@pytest.mark.parametrize("scene,variant", [("stack", "normal"), ("pile", "normal"), ("pile", "no-normal"), ("stack", "extra1")])
def test_saturating_scenes_against_the_oracle(scene, variant, keep_all_pairs):
    case, feats, dX, orc = _reference(scene, variant)
    (_premise_stack if scene == "stack" else _premise_pile)(orc)
    hip = run_hip(case, backward=True, keep_all_pairs=keep_all_pairs, colors_extra=feats or None, dL_dextra=dX or None)
    compare_forward(hip, orc, tol=IMAGE_TOL)            # colour, depth, alpha, normal: bit for bit
    checked = compare_backward(hip, orc)
    assert "means3D" in checked and "opacities" in checked
    for k, of in enumerate(orc.get("extra", [])):
        nz = int((hip["extra"][k].view(np.uint32) != of["img"]["color"].view(np.uint32)).sum())
        assert nz == 0, f"extra image {k}: {nz} values differ from the oracle's"
        assert_grad_close(hip["render_grads"][f"rgb_extra{k}"], of["grads"]["render_grads"]["rgb"], f"render:rgb_extra{k}")
        assert_grad_close(hip["grads"]["colors_extra"][k], of["grads"]["colors"], f"colors_extra[{k}]")
    if variant == "no-normal":
        assert not hip["normal"].any()
