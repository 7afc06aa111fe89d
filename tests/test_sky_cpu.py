"""CPU: the sky oracle against the golden vectors captured from the reference's SkyCubeMap / EnvLight / render() blend
(tests/gen_golden.py, nvdiffrast's dr.texture replaced by the oracle lookup), and the size-independent properties of the
cube lookup itself (the part of the path whose parity is unpinned: nvdiffrast is absent from the reference tree)."""
import os

import numpy as np
import pytest
import torch

from oracle import sky_oracle as so

G = os.path.join(os.path.dirname(__file__), "golden")


def _t(a):
    return torch.from_numpy(np.asarray(a))


def test_rays_mask_clamp_layout_blend_match_reference():
    g = np.load(os.path.join(G, "s3g_sky.npz"))
    H, W = int(g["H"]), int(g["W"])
    w2c = _t(g["world_view_transform"]).T
    rays = so.rays(H, W, _t(g["K"]), w2c[:3, :3], w2c[:3, 3])
    np.testing.assert_allclose(rays.numpy(), g["rays"], atol=2e-6)
    for tag, fill in (("white", 1.0), ("black", 0.0)):
        np.testing.assert_allclose(_t(g[f"{tag}_dirs_all"]).numpy(), g["rays"], atol=0)      # what the reference handed to dr.texture
        cube, acc = _t(g[f"{tag}_cube"]), _t(g[f"{tag}_acc"])
        np.testing.assert_allclose(so.sky_s3g(cube, rays).numpy(), g[f"{tag}_sky_all"], atol=1e-5)
        sky = so.sky_s3g(cube, rays, acc, fill=fill)
        np.testing.assert_allclose(sky.numpy(), g[f"{tag}_sky_masked"], atol=1e-5)
        assert int(((1 - acc[0]) > 1e-3).sum()) == int(g[f"{tag}_n_masked_dirs"])
        assert np.all(sky.numpy()[:, :10] == fill)                                           # fully covered rows are not sampled
        np.testing.assert_allclose(so.blend_s3g(_t(g[f"{tag}_render"]), acc, sky).numpy(), g[f"{tag}_blended"], atol=1e-5)
        assert g[f"{tag}_sky_all"].min() >= 0 and g[f"{tag}_sky_all"].max() <= 1


def test_envlight_matches_reference():
    g = np.load(os.path.join(G, "or_envlight.npz"))
    d = _t(g["viewdirs"]).reshape(-1, 3) @ _t(g["to_opengl"]).T
    np.testing.assert_allclose(d.numpy(), g["lookup_dirs"], atol=1e-7)
    light = so.cube_lookup(_t(g["base"]), d).reshape(g["light"].shape)
    np.testing.assert_allclose(light.numpy(), g["light"], atol=1e-6)
    np.testing.assert_allclose(so.blend_add(_t(g["rgb"]), _t(g["opacity"]), light).numpy(), g["blended"], atol=1e-6)


def test_cube_lookup_properties():
    torch.manual_seed(0)
    res = 16
    cube = torch.rand(6, res, res, 3)
    d = torch.randn(50000, 3)
    # constant texture -> constant colour (weights sum to one everywhere, corners included)
    np.testing.assert_allclose(so.cube_lookup(torch.full((6, res, res, 3), 0.37), d).numpy(), 0.37, atol=1e-6)
    # the six axes hit the centre of faces +x,-x,+y,-y,+z,-z
    for f, ax in enumerate([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]):
        v = so.cube_lookup(cube, torch.tensor([ax], dtype=torch.float32))[0]
        np.testing.assert_allclose(v.numpy(), cube[f, res // 2 - 1:res // 2 + 1, res // 2 - 1:res // 2 + 1].mean((0, 1)).numpy(), atol=1e-6)
    # OpenGL orientation: on +z, u grows with x and v grows with -y
    face, u, v = so.index_cube(torch.tensor([[0.5, 0.0, 1.0], [0.0, 0.5, 1.0]]))
    assert face.tolist() == [4, 4] and u[0] > 0.5 and abs(v[0] - 0.5) < 1e-6 and v[1] < 0.5
    # scale invariance
    np.testing.assert_allclose(so.cube_lookup(cube, d * 7.5).numpy(), so.cube_lookup(cube, d).numpy(), atol=1e-5)
    # seamless: moving a direction by 1e-5 never changes the colour by more than the texture gradient allows,
    # in particular not across the 12 edges (a seam would jump by O(1))
    out = so.cube_lookup(cube, d)
    d2 = d / d.norm(dim=1, keepdim=True)
    step = 1e-4 * torch.randn_like(d2)
    jump = (so.cube_lookup(cube, d2 + step) - out).abs().max().item()
    assert jump < 0.02, jump
    # directions ON edges and corners are finite and inside the range of the texture
    e = torch.tensor([[1.0, 1.0, 0.3], [1.0, -1.0, -0.2], [-1.0, 0.4, 1.0], [1.0, 1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, -1.0, 1.0]])
    v = so.cube_lookup(cube, e)
    assert torch.isfinite(v).all() and v.min() >= cube.min() and v.max() <= cube.max()
    idx, w = so.cube_taps(e, res)
    np.testing.assert_allclose(w.sum(1).numpy(), 1.0, atol=1e-6)
    assert (w[3:] == 0).sum() >= 3            # each corner direction drops its fourth tap


# ---- the camera-ray cases of tests/sky_cases.py: what float32 costs the oracle itself (the GPU test's tolerances), and proof that the cases
# ---- reach the branches of k_sky_backward they are there for.  Nothing below touches the kernel.
from tests import sky_cases as sc  # noqa: E402

ALL_IDS = list(sc.CASES) + list(sc.VARIANTS)


@pytest.mark.parametrize("case_id", ALL_IDS)
def test_float32_cost_stays_within_table(case_id):
    """The oracle in float32 against the oracle in float64 on the same inputs: the largest difference of every compared quantity is what
    sky_cases.TABLE says (never above; not below a quarter of it either, so the table cannot drift loose).  Marked pixels stay rare."""
    worst = {}
    for white in (True, False):
        c = sc.build(case_id, white)
        assert int(c.marked.sum()) <= sc.MARK_SHARE * c.H * c.W, (case_id, white, int(c.marked.sum()))
        r32, r64 = sc.reference(case_id, white, torch.float32), sc.reference(case_id, white, torch.float64)
        assert set(r64) == set(sc.TABLE[case_id])
        for q in r64:
            assert r32[q].dtype == torch.float32 and r64[q].dtype == torch.float64
            worst[q] = max(worst.get(q, 0.0), sc.max_diff(r32[q], r64[q], c, q))
    print(case_id, {q: f"{v:.2e}" for q, v in worst.items()})
    for q, v in worst.items():
        assert sc.TABLE[case_id][q] / 4 <= v <= sc.TABLE[case_id][q], (case_id, q, v, sc.TABLE[case_id][q])


@pytest.mark.parametrize("case_id", ALL_IDS)
def test_case_inputs_are_as_specified(case_id):
    for white in (True, False):
        c = sc.build(case_id, white)
        a = c.acc[0]
        assert (a[:, :5] == 1.0).all() and ((a - (1 - 1e-3)).abs() > sc.ACC_GAP).all()
        assert c.cube.min() < -0.25 and c.cube.max() > 1.25
        assert ((c.g_out[1] == 0).all() and (c.g_sky[1] == 0).all()) == (case_id == sc.ZERO_CHANNEL_CASE)
        assert (c.g_out[:, c.marked] == 0).all() and (c.g_sky[:, c.marked] == 0).all()
        if c.H >= 16 and c.W >= 32:
            assert (a[:16, 16:32] == 1.0).all()
        r = sc.reference(case_id, white)
        assert (r["sky"][:, ~c.sampled] == c.fill).all() and 0 < int(c.sampled.sum()) < c.H * c.W
        clamped = (r["sky"][:, c.sampled] == 0).sum() + (r["sky"][:, c.sampled] == 1).sum()
        assert clamped > 0                                                  # the clamp acts
    if case_id == "sky-mask":
        assert c.H > 50 and not c.sampled[50:].all() and c.sampled[:50].all() and not c.sky_mask[0, :50].all()


def _taps(c):
    """float64 reference taps of the sampled pixels: (pixel y, x), own face, tap texels [n,4], weights [n,4], and the gradient that reaches the
    lookup per channel [n,3] (zero where the clamp does not pass)."""
    w2c = c.w2c
    dirs = so.rays(c.H, c.W, c.K, w2c[:3, :3], w2c[:3, 3], c.jitter, dtype=torch.float64)[c.sampled]
    idx, w = so.cube_taps(dirs, c.res)
    col = (c.cube.double().reshape(-1, 3)[idx] * w[..., None]).sum(1)
    gs = 2.0 * (c.g_sky.double() + c.g_out.double() * (1 - c.acc.double()))[:, c.sampled].T
    gs = gs * ((col >= 0) & (col <= 1))
    yx = torch.nonzero(c.sampled)
    return yx, so.index_cube(dirs)[0], idx, w, gs


def _window_stats(c):
    """The window rule of k_sky_backward restated: per 16 x 16 pixel tile the leader is the first pixel in row-major tile order that is sampled and
    has a non-zero gradient; the window is SKY_WIN = 24 texels square on the face of the leader's tap 0 with origin (u0 - 12, v0 - 12).
    -> (tap weight outside the windows, tap weight in all, number of tiles whose window leaves the face, tiles without a leader)."""
    yx, _, idx, w, gs = _taps(c)
    live = (gs != 0).any(1)
    r2 = c.res * c.res
    outside = total = 0.0
    off_face = 0
    tiles = [(ty, tx) for ty in range((c.H + 15) // 16) for tx in range((c.W + 15) // 16)]
    for ty, tx in tiles:
        sel = live & (yx[:, 0] // 16 == ty) & (yx[:, 1] // 16 == tx)
        if not sel.any():
            continue
        lane = (yx[:, 0] % 16) * 16 + yx[:, 1] % 16
        leader = torch.nonzero(sel)[lane[sel].argmin()].item()
        t0 = int(idx[leader, 0])
        of, ou, ov = t0 // r2, t0 % r2 % c.res - 12, t0 % r2 // c.res - 12
        off_face += int(ou < 0 or ov < 0 or ou + 24 > c.res or ov + 24 > c.res)
        f, u, v = idx[sel] // r2, idx[sel] % r2 % c.res, idx[sel] % r2 // c.res
        in_win = (f == of) & (u >= ou) & (u < ou + 24) & (v >= ov) & (v < ov + 24)
        total += float(w[sel].sum())
        outside += float(w[sel][~in_win].sum())
    empty = sum(1 for ty, tx in tiles if not (live & (yx[:, 0] // 16 == ty) & (yx[:, 1] // 16 == tx)).any())
    return outside, total, off_face, empty


@pytest.mark.parametrize("white", [True, False])
def test_cases_reach_their_branches(white):
    stats = {}
    for case_id in sc.CASES:
        c = sc.build(case_id, white)
        yx, own, idx, w, gs = _taps(c)
        faces = set((idx[w > 0] // (c.res * c.res)).tolist())
        corner = int((w == 0).any(1).sum())
        other = int(((idx // (c.res * c.res) != own[:, None]) & (w > 0)).sum())
        stats[case_id] = (faces, corner, other)
        print(case_id, stats[case_id])
        if case_id.startswith("corner"):
            assert len(faces) >= 3 and corner > 0 and other > 0, (case_id, stats[case_id])
    assert stats["face-mag"][0] == {0} and stats["face-mag"][2] == 0
    assert stats["odd-neg"][0] & {1, 3, 5}
    out, tot, _, empty = _window_stats(sc.build("minified", white))
    assert out > 0.5 * tot, (out, tot)
    assert empty == 1                                                            # the tile of acc == 1: the early return
    out, tot, off, _ = _window_stats(sc.build("face-mag", white))
    assert out == 0 and off == 0 and tot > 0
    out, tot, off, empty = _window_stats(sc.build("corner-mag", white))
    assert off > 0 and empty == 1 and 0 < out < tot
    out, tot, off, empty = _window_stats(sc.build("corner-64", white))
    assert 0 < out < tot and empty == 1                                          # taps on the window's face and on another, from the same tiles
    # a leader that is not lane 0: no tile in the first column of tiles can start at its first pixel (columns 0-4 are not sampled)
    for case_id in sc.CASES:
        assert not sc.build(case_id, white).sampled[:, :5].any()
