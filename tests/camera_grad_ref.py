"""The reference of the camera-gradient tests (tests/test_camera_grad_{cpu,gpu}.py): the fp64 autograd restatement of the hot path
(oracle/torch_ref.py, itself pinned by tests/test_oracle_cpu.py) with the camera -- viewmatrix, projmatrix, campos -- as fp64 LEAVES.

  * `camera35`: dL/d(V[16], P[16], campos[3]) in the layout of EmdSettings, (a) from given per-Gaussian gradients of the projection's
    outputs (the render backward's accumulator rows: the projection part alone), (b) through `tr.composite` from the image gradients.
  * `jacobians`: d(projection outputs of ONE visible Gaussian)/d(camera), [visible, 9, 35].  From them come the TERMS of the sum the
    kernel forms and the condition-aware bound of tests/helpers.py's pose bar:  |got - ref| <= GRAD_RTOL |ref| + POSE_TERM_RTOL sum_i sum_path |term_i,path| + 1e-12.
    The four paths count separately, so that cancellation BETWEEN them is covered: pixel mean (through P), covariance (the conic through
    M = J W, i.e. the view matrix as `project` reads it for W), camera-space mean (the conic through J's dependence on t = (m, 1) V, and
    the view depth), colour (through campos).  The middle two both run through V and do cancel: with a camera whose z axis is a world
    axis and whose centre has coordinate 0 along it (scenes.small_camera at yaw 0) a change of V[0] or V[1] moves M and t so that the
    conic of an unclamped Gaussian stays put EXACTLY -- the kernel adds J00 dM0 and m dt, two fp32 terms whose sum is zero.  To tell the
    two apart without restating `project`, the view matrix handed to it is a `SplitView`: `hom @ V` reads one leaf, `V[:3, :3]` the other.
"""
import numpy as np
import torch

from oracle import cpu_oracle as co
from oracle import torch_ref as tr
from tests.helpers import GRAD_RTOL, POSE_TERM_RTOL, make_case, place_in_depth_band, run_oracle

N_CASE = dict(n=600, H=32, W=48)      # 600 = 2 * 256 + 88: three workgroups, a ragged last one
# seed 0 of the static case: the reference shows visible Gaussians whose view-space x/z or y/z is clamped (asserted in nonvacuous())
CASES = {
    "static-sh": dict(seed=0),
    # (yawed: at yaw 0 the camera's z axis is a world axis, dL/dV[0] and dL/dV[1] of unclamped Gaussians vanish identically (module
    #  docstring) and this seed has no clamped one -- kept as it is in the static case, where four clamped Gaussians leave a residue)
    "motion-residual": dict(seed=1, motion=True, residual=True, yaw=0.15),
    "cov-colors": dict(seed=2, cov_precomp=True, colors_precomp=True),
    "sh-deg0": dict(seed=10, sh_degree=0),
    "near-0.05": dict(seed=8, near_plane=0.05, band=(0.05, 0.2)),
    # (yawed by 3 degrees for the same reason: the three clamped Gaussians of this seed are clamped in y/z only, which leaves dL/dV[0] an
    #  identically vanishing sum -- 1e-17 of its terms in fp64, or an exact 0.0, as the rounding falls, which nonvacuous() does not count as non-zero)
    "raw-params": dict(seed=61, raw=True, yaw=3.0),
}
READ_V = [4 * k + r for k in range(4) for r in range(3)]
READ_P = [16 + 4 * k + j for k in range(4) for j in (0, 1, 3)]
UNREAD = [3, 7, 11, 15, 18, 22, 26, 30]


def build_case(name):
    """-> (case, raw) with raw = None or dict(log_s, raw_q, logit), built as tests/helpers.raw_params_parity's callers build them."""
    kw = dict(N_CASE, **CASES[name])
    band, is_raw = kw.pop("band", None), kw.pop("raw", False)
    case = make_case(**kw)
    if band is not None:
        place_in_depth_band(case, np.arange(3 * case["N"] // 50, 3 * case["N"] // 50 + case["N"] // 5), *band, seed=kw["seed"])
    raw = None
    if is_raw:
        g = torch.Generator().manual_seed(5)
        raw = dict(log_s=torch.log(case["scales"]), raw_q=case["rotations"] * (0.5 + torch.rand(case["N"], 1, generator=g)),
                   logit=torch.logit(case["opacities"].clamp(1e-4, 1 - 1e-4)))
    return case, raw


class SplitView:
    """A view matrix with two leaves of the same value: `hom @ V` (the camera-space mean) reads `Vt`, `V[:3, :3]` (the rotation W of the
    covariance) reads `Vm`.  dL/dV = dL/dVt + dL/dVm."""

    def __init__(self, V):
        self.Vt, self.Vm = V.detach().clone().requires_grad_(True), V.detach().clone().requires_grad_(True)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        return func(*[a.Vt if isinstance(a, SplitView) else a for a in args], **(kwargs or {}))

    def __getitem__(self, idx):
        return self.Vm[idx]


def camera_leaves(S):
    """Replace the camera of a TorchSettings by fresh fp64 leaves; S.leaves = (Vt, Vm, P, campos)."""
    S.view = SplitView(S.view)
    S.proj = S.proj.detach().clone().requires_grad_(True)
    S.campos = S.campos.detach().clone().requires_grad_(True)
    S.leaves = (S.view.Vt, S.view.Vm, S.proj, S.campos)
    return S


def flat51(g):
    """(dVt, dVm, dP, dcampos) -> [51] numpy, None as zeros."""
    z = lambda x, n: torch.zeros(n, dtype=torch.float64) if x is None else x.reshape(-1).to(torch.float64)
    return torch.cat([z(g[0], 16), z(g[1], 16), z(g[2], 16), z(g[3], 3)]).numpy()


def fold35(v51):
    """[..., 51] -> [..., 35]: the two halves of the view matrix added."""
    return np.concatenate([v51[..., 0:16] + v51[..., 16:32], v51[..., 32:51]], -1)


def leaf_grads35(S):
    """The camera gradient a backward() left on the leaves of camera_leaves(S)."""
    return fold35(flat51([x.grad for x in S.leaves]))


class Reference:
    """World-space inputs (fp64, no grad) of the VISIBLE Gaussians of one view + the settings; everything else is derived."""

    def __init__(self, H, W, tanfovx, tanfovy, bg, view, proj, campos, sh_degree, scale_modifier, near_plane, radii, ids, ranges,
                 means, opac, shs=None, colors=None, scales=None, rots=None, cov=None, clamp01=False):
        self.mk = lambda: tr.TorchSettings(H, W, tanfovx, tanfovy, bg, view, proj, sh_degree, campos, scale_modifier, near_plane)
        self.N = means.shape[0]
        self.vis = np.asarray(radii) > 0
        self.idx = torch.as_tensor(np.nonzero(self.vis)[0])
        self.ids, self.ranges = ids, ranges
        sel = lambda t: None if t is None else t.detach()[self.idx]
        self.means, self.opac_all = sel(means), opac.detach().reshape(-1)
        self.shs, self.colors, self.scales, self.rots, self.cov, self.clamp01 = sel(shs), sel(colors), sel(scales), sel(rots), sel(cov), clamp01
        self._jac = None

    @classmethod
    def from_case(cls, case, orc):
        """`orc` = run_oracle(case): the visibility and the tile lists."""
        t = lambda a: None if a is None else torch.as_tensor(np.asarray(a, np.float64))
        scales, rots, opac = case["scales"], case["rotations"], case["opacities"]
        means, rots, opac = t(case["means3D"]), t(rots), t(opac).reshape(-1)
        if case["flags"] & co.F_MOTION:
            aid = torch.as_tensor(case["actor_ids"].numpy().astype(np.int64))
            means, rots, opac = tr.motion_transform(means, rots, opac, aid, t(case["actor_pose"]), t(case["residual_dx"]), t(case["residual_dq"]))
        cam = case["cam"]
        return cls(case["H"], case["W"], cam.tanfovx, cam.tanfovy, case["bg"].numpy(), cam.world_view_transform.numpy(),
                   cam.full_proj_transform.numpy(), cam.camera_center.numpy(), case["sh_degree"], case.get("scale_modifier", 1.0),
                   case.get("near_plane", 0.2), orc["pre"]["radii"], orc["bin"]["ids"], orc["bin"]["ranges"], means, opac, t(case["shs"]),
                   t(case["colors_precomp"]), t(scales), rots, t(case["cov3D_precomp"]), bool(case["flags"] & co.F_CLAMP01))

    def settings(self, cam=None):
        """TorchSettings with fresh camera leaves, or with the given (view, proj, campos) tensors (non-leaves of a longer chain)."""
        S = self.mk()
        if cam is None:
            return camera_leaves(S)
        S.view, S.proj, S.campos = cam
        return S

    def project(self, S, sl=slice(None)):
        """The projection's outputs of the visible Gaussians `sl`: (m2d [n,2], tz [n], conic [n,3], rgb [n,3])."""
        g = lambda t: None if t is None else t[sl]
        return tr.project(S, self.means[sl], g(self.shs), g(self.colors), None, g(self.scales), g(self.rots), g(self.cov), clamp01=self.clamp01)

    def rows(self, g):
        """[visible, 9] from a dict of per-Gaussian [N, .] arrays (mean2D, depth, conic, rgb), fp64."""
        a = lambda k, w: torch.as_tensor(np.asarray(g[k], np.float64).reshape(self.N, w))[self.idx]
        return torch.cat([a("mean2D", 2), a("depth", 1), a("conic", 3), a("rgb", 3)], 1)

    def camera35_from_rows(self, rows, S=None):
        """Full autograd of sum(outputs * rows) w.r.t. the camera leaves: the projection backward alone."""
        S = self.settings() if S is None else S
        out = torch.cat([o.reshape(len(self.idx), -1) for o in self.project(S)], 1)
        return fold35(flat51(torch.autograd.grad((out * rows).sum(), S.leaves, allow_unused=True)))

    def images(self, S):
        """Through the compositing: (color, depth, alpha images, the projection's outputs [visible, 9] with retained grad)."""
        m2d, tz, conic, rgb = self.project(S)
        out9 = torch.cat([m2d, tz[:, None], conic, rgb], 1)
        out9.retain_grad()
        full = torch.zeros(self.N, 9, dtype=torch.float64).index_copy(0, self.idx, out9)
        img = tr.composite(S, self.ids, self.ranges, full[:, 0:2], full[:, 2], full[:, 3:6], self.opac_all, full[:, 6:9])
        return img, out9

    def jacobian_of(self, i):
        """[9, 51] of visible Gaussian i alone: its projection outputs backpropagated one by one to fresh camera leaves."""
        S = self.settings()
        o = torch.cat([x.reshape(-1) for x in self.project(S, slice(i, i + 1))])
        J = np.zeros((9, 51))
        for j in range(9):
            if o[j].requires_grad:           # (a precomputed colour does not depend on the camera)
                J[j] = flat51(torch.autograd.grad(o[j], S.leaves, retain_graph=True, allow_unused=True))
        return J

    def jacobians(self):
        """[visible, 9, 51], d(output j of visible Gaussian i)/d(Vt, Vm, P, campos).  One Gaussian at a time costs 9 backward passes per
        Gaussian (10 s per case); the same numbers come out of 51 batched passes: G(w) = d/d camera of sum_ij w_ij out_ij is linear in the
        weights w, and dG_e/dw_ij IS that Jacobian entry.  A sample of Gaussians is redone one at a time (jacobian_of) and must agree."""
        if self._jac is None:
            S = self.settings()
            out = torch.cat([o.reshape(len(self.idx), -1) for o in self.project(S)], 1)
            w = torch.ones_like(out).requires_grad_(True)
            G = torch.autograd.grad((out * w).sum(), S.leaves, create_graph=True, allow_unused=True)
            G = [None if g is None else g.reshape(-1) for g in G]
            J = np.zeros((len(self.idx), 9, 51))
            for e in range(51):
                g = G[min(e // 16, 3)]
                ge = None if g is None else g[e - 16 * min(e // 16, 3)]
                if ge is not None and ge.requires_grad:
                    J[:, :, e] = torch.autograd.grad(ge, w, retain_graph=True)[0].numpy()
            for i in np.random.default_rng(0).choice(len(self.idx), size=min(6, len(self.idx)), replace=False):
                one = self.jacobian_of(int(i))
                assert np.abs(one - J[i]).max() <= 1e-10 * max(np.abs(one).max(), 1e-300), int(i)
            self._jac = J
        return self._jac

    def terms(self, rows):
        """[visible, 4 paths, 35]: what every visible Gaussian adds to the 35 sums along every path."""
        T = self.jacobians() * rows.numpy()[:, :, None]                       # [visible, 9, 51]
        only = lambda a, lo, hi: np.concatenate([np.zeros_like(a[..., :lo]), a[..., lo:hi], np.zeros_like(a[..., hi:])], -1)
        pix, sh = T[:, 0:2].sum(1), T[:, 6:9].sum(1)
        cov = only(T[:, 3:6].sum(1), 16, 32)                                  # the conic through Vm
        mean = T[:, 3:6].sum(1) - cov + T[:, 2]                               # the conic through Vt (nothing else reaches it), and the depth
        return fold35(np.stack([pix, cov, mean, sh], 1))


def term_bound(terms):
    return POSE_TERM_RTOL * np.abs(terms).sum((0, 1))


def bound35(ref, terms, extra=0.0):
    return GRAD_RTOL * np.abs(ref) + term_bound(terms) + extra + 1e-12


def check_decomposition(terms, full):
    """The terms add up to the full-autograd camera gradient (1e-9 relative): the decomposition the bound is built on is the sum itself."""
    s = terms.sum((0, 1))
    scale = max(float(np.abs(full).max()), 1e-300)
    assert float(np.abs(s - full).max()) <= 1e-9 * scale, (float(np.abs(s - full).max()), scale)


# "Non-zero in the reference" means a sum that does not vanish identically.  One that does (module docstring) comes out of fp64 autograd as
# 0.0 or as a residue of some n * 2^-53 ~ 1e-13 of the magnitudes of its terms, whichever way the rounding falls -- nothing a test may
# depend on, and nothing that exercises the kernel.  An entry counts only four decades above that residue.
NONZERO_OF_TERMS = 1e-9


def nonvacuous(name, ref, cam35, terms, case=None, min_visible=100):
    """The CPU-side asserts every case makes before the GPU runs: enough visible Gaussians, every read entry of V and P (and campos for SH
    colours) moves the loss (above NONZERO_OF_TERMS of the magnitudes of its `terms`), the near band of `near-0.05` is populated."""
    nv = int(ref.vis.sum())
    assert nv >= min_visible, (name, nv)
    moves = np.abs(cam35) > NONZERO_OF_TERMS * np.abs(terms).sum((0, 1))
    assert moves[READ_V].all() and moves[READ_P].all(), (name, cam35, np.abs(terms).sum((0, 1)))
    assert (cam35[UNREAD] == 0).all()
    if ref.shs is not None and ref.mk().sh_degree > 0:        # (a degree-0 colour has no direction: its campos gradient is exactly zero)
        assert moves[32:35].all(), (name, cam35[32:35])
    else:
        assert (cam35[32:35] == 0).all()
    if case is not None and case.get("near_plane", 0.2) < 0.2:
        tz = ref.project(ref.mk())[1].numpy()
        assert int(((tz > case["near_plane"]) & (tz < 0.2)).sum()) >= 10, name


def clamped_count(ref):
    """Visible Gaussians whose view-space x/z or y/z lies outside 1.3 tan(fov / 2) (the clx / cly branches of the kernel)."""
    S = ref.mk()
    hom = torch.cat([ref.means, torch.ones(len(ref.idx), 1, dtype=torch.float64)], 1) @ S.view
    return int(((hom[:, 0] / hom[:, 2]).abs() > 1.3 * S.tanfovx).sum() + ((hom[:, 1] / hom[:, 2]).abs() > 1.3 * S.tanfovy).sum())


# ---- the gsplat camera (emd_amd.gsplat_api._device_camera) restated in fp64 ------------------------------------------------------------

def device_camera_ref(vm, K, width, height, znear=0.01, zfar=100.0):
    """(wvt, full, campos) of one gsplat camera from its world-to-camera matrix `vm` [4,4] and intrinsics `K` [3,3], differentiable fp64:
    wvt = vm^T; full = wvt P^T with the pinhole projection of emd_amd.camera.projection_from_K; campos = -R^T t."""
    vm, K = vm.to(torch.float64), K.to(torch.float64)
    P = torch.zeros(4, 4, dtype=torch.float64)
    P[0, 0], P[1, 1] = 2.0 * K[0, 0] / width, 2.0 * K[1, 1] / height
    P[0, 2], P[1, 2] = (2.0 * K[0, 2] - width) / width, (2.0 * K[1, 2] - height) / height
    P[3, 2], P[2, 2], P[2, 3] = 1.0, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    wvt = vm.t()
    return wvt, wvt @ P.t(), -(vm[:3, :3].t() @ vm[:3, 3])


def se3_exp(delta):
    """[6] = (translation part, rotation vector) -> the 4x4 rigid transform exp of the twist."""
    v, w = delta[:3], delta[3:]
    z = torch.zeros((), dtype=delta.dtype)
    A = torch.stack([torch.stack([z, -w[2], w[1], v[0]]), torch.stack([w[2], z, -w[0], v[1]]), torch.stack([-w[1], w[0], z, v[2]]),
                     torch.zeros(4, dtype=delta.dtype)])
    return torch.linalg.matrix_exp(A)
