"""The SH colour beside the rasterizer (`emd_sh_forward` / `emd_sh_backward`, `emd_sh_grad_from_factors` and the callers that reach them:
`gsplat_api.spherical_harmonics`, `nodes._colors`, `model.pre_compute_colors`, `dp.sh_grad_from_factors`) restated in plain torch, fp64 on the
CPU, with the inputs the CPU and the GPU tests share.

`sh_colour` is `oracle/torch_ref.eval_sh` (the reference's polynomial, pinned by tests/golden/s3g_sh.npz) on the normalised directions;
autograd supplies every gradient.  `dense_from_factors` is the sum over views that `dp.sh_grad_from_factors` documents, with the world means
of `torch_ref.motion_transform`.  Nothing here shares code with the kernels.  Every function takes a `dtype`: float64 is the reference, float32
the same formula at the kernels' precision -- tests/test_sh_paths_cpu.py holds it against the fp64 result under the project's criterion
(`criterion` below is tests/skinning_ref.criterion, imported), which is the evidence that the bar comes from the formula
and the number format and not from a kernel.

Inputs are fp32 tensors built from fixed seeds (the reference upcasts the same values the kernels read) and are cached together with their
references: treat both as read-only."""
import functools

import torch
import torch.nn.functional as F

from oracle import torch_ref as tr
from tests.skinning_ref import criterion  # noqa: F401  (the bar of every comparison: imported, never restated)

F64 = torch.float64

# ---- a/b/c: the stand-alone forward and backward -------------------------------------------------------------------------------------
SH_DEG_ROWS = ((0, 1), (0, 16), (1, 4), (1, 16), (2, 9), (2, 16), (3, 16))                 # (degree, coefficient rows M)
SH_COUNTS = (1, 255, 256, 257, 1000)                                                      # one lane; a block less one, exact, plus one; four blocks
SH_CASES = tuple((deg, M, N) for deg, M in SH_DEG_ROWS for N in SH_COUNTS)
DIR_NORM = (0.5, 20.0)

# ---- e: the dense gradient from per-view factors -------------------------------------------------------------------------------------
FACTOR_COUNTS = (1, 127, 128, 129, 255, 256, 257, 700)                                    # the seams of the two 128-row halves of a 256-lane block
FACTOR_FORMS = ("static", "shared", "per_view", "residual")
FACTOR_SWEEP = tuple(dict.fromkeys([(2, 2, N) for N in FACTOR_COUNTS] + [(deg, V, 257) for deg in range(4) for V in (1, 2, 3)]))
FACTOR_FORM_CASES = tuple((deg, 3, 700, form, scale) for deg in (1, 3) for form in FACTOR_FORMS for scale in (1.0, 1.0 / 3.0))
FACTOR_ACTORS = 5
CAMERA_DISTANCE = 2.0                                                                     # every camera centre is at least this far from every world mean

# ---- f: the callers ------------------------------------------------------------------------------------------------------------------
NODE_CASES = ((3, 0), (3, 1000), (3, 2000), (3, 3000), (1, 5000), (2, 5000))             # (sh_degree, step): n = 0, 1, 2, 3 of 16 rows; 4 and 9 rows
NODE_POINTS, NODE_ACTORS, NODE_INTERVAL = 300, 2, 1000
PRECOMPUTE_DEGREES = (0, 1, 2, 3)
CLAMP_MARGIN = 1e-5


def sh_colour(deg, coeffs, dirs, dtype=F64):
    """eval_sh(deg, coeffs^T, dirs / |dirs|): coeffs [..., M, 3], dirs [..., 3] (any length but zero) -> [..., 3]."""
    coeffs, dirs = coeffs.to(dtype), dirs.to(dtype)
    return tr.eval_sh(deg, coeffs.transpose(-1, -2), dirs / dirs.norm(dim=-1, keepdim=True))


def sh_grads(deg, coeffs, dirs, g, dtype=F64, post=None):
    """Colour (after `post`, e.g. the callers' + 0.5 and clamp), the value in front of `post`, and dL/dcoeffs, dL/ddirs for L = sum(colour * g).
    Autograd returns None for the directions at degree 0 (the colour does not depend on them): zeros then."""
    c = coeffs.detach().to(dtype).clone().requires_grad_(True)
    d = dirs.detach().to(dtype).clone().requires_grad_(True)
    pre = sh_colour(deg, c, d, dtype)
    out = pre if post is None else post(pre)
    gc, gd = torch.autograd.grad((out * g.to(dtype)).sum(), (c, d), allow_unused=True)
    return dict(colour=out.detach(), pre=pre.detach(), d_coeffs=torch.zeros_like(c) if gc is None else gc,
                d_dirs=torch.zeros_like(d) if gd is None else gd)


def world_means(means, ids=None, pose=None, rdx=None, dtype=F64):
    """torch_ref.motion_transform on the means alone: residual added to every point, the pose of its actor applied where ids >= 0."""
    means = means.to(dtype)
    if ids is None and rdx is None:
        return means
    if ids is None:
        ids, pose = torch.full((means.shape[0],), -1, dtype=torch.int64), torch.zeros(1, 12)
    return tr.motion_transform(means, None, None, ids, pose.to(dtype), None if rdx is None else rdx.to(dtype))[0]


def dense_from_factors(deg, means, campos, factors, ids=None, pose=None, rdx=None, scale=1.0, rows=16, dtype=F64):
    """scale * sum_v d/dshs [ (sh_colour(deg, shs, mean_v - campos_v) * g_v).sum() ]  -> [N, rows, 3].  pose [A,12]: every view shares it;
    [V,A,12]: one table per view.  The colour is linear in shs, so the value at which autograd differentiates does not matter."""
    N, V = means.shape[0], campos.shape[0]
    shs = torch.zeros(N, rows, 3, dtype=dtype, requires_grad=True)
    total = 0
    for v in range(V):
        wm = world_means(means, ids, pose if (pose is None or pose.dim() == 2) else pose[v], rdx, dtype)
        total = total + (sh_colour(deg, shs, wm - campos[v].to(dtype), dtype) * factors[v].to(dtype)).sum()
    return scale * torch.autograd.grad(total, shs)[0]


def _gen(seed):
    g = torch.Generator().manual_seed(seed)
    return (lambda *s: torch.rand(*s, generator=g, dtype=F64)), (lambda *s: torch.randn(*s, generator=g, dtype=F64)), g


def _pose_tables(r, n, tables, actors):
    """[tables, actors, 12]: unit q_mean, translation in [-1, 1]^3, valid = 1, unit q_rot (include/emd_raster.h: EMD_ACTOR_STRIDE)."""
    return torch.cat([F.normalize(n(tables, actors, 4), dim=-1), 2.0 * r(tables, actors, 3) - 1.0, torch.ones(tables, actors, 1, dtype=F64),
                      F.normalize(n(tables, actors, 4), dim=-1)], -1)


@functools.lru_cache(maxsize=None)
def sh_case(deg, M, N):
    """dirs [N,3] with |dirs| in [0.5, 20], coeffs [N,M,3], the upstream colour gradient g [N,3]."""
    r, n, _ = _gen(7000 + 1000 * deg + 37 * M + N)
    dirs = F.normalize(n(N, 3), dim=-1) * (0.51 + 19.4 * r(N, 1))
    return dict(deg=deg, M=M, N=N, K=(deg + 1) ** 2, dirs=dirs.float(), coeffs=n(N, M, 3).float(), g=n(N, 3).float())


@functools.lru_cache(maxsize=None)
def sh_reference(deg, M, N, dtype=F64):
    c = sh_case(deg, M, N)
    return sh_grads(deg, c["coeffs"], c["dirs"], c["g"], dtype)


@functools.lru_cache(maxsize=None)
def factor_case(deg, V, N, form="shared"):
    """Means in a unit box, camera centres on the sphere of radius 6 (world means stay within 3 of the origin), factor rows [V,N,3] with a third
    of the (view, Gaussian) pairs exactly zero; Gaussian 0 is invisible in view 0 and visible in view 1, the last Gaussian invisible everywhere.
    static: no motion block; shared: one pose table, a third of the ids -1; per_view: one table per view; residual: shared plus residual_dx."""
    r, n, g = _gen(9000 + 1000 * deg + 100 * V + N + 17 * FACTOR_FORMS.index(form))
    case = dict(deg=deg, V=V, N=N, form=form, K=(deg + 1) ** 2, means=(r(N, 3) - 0.5).float(), ids=None, pose=None, rdx=None)
    if form != "static":
        ids = torch.randint(0, FACTOR_ACTORS, (N,), generator=g)
        ids[torch.randperm(N, generator=g)[:(N + 1) // 3]] = -1
        pose = _pose_tables(r, n, V if form == "per_view" else 1, FACTOR_ACTORS)
        case.update(ids=ids, pose=(pose if form == "per_view" else pose[0]).float().contiguous())
    if form == "residual":
        case["rdx"] = (0.05 * n(N, 3)).float()
    case["campos"] = (6.0 * F.normalize(n(V, 3), dim=-1)).float()
    factors = n(V, N, 3)
    zero = torch.zeros(V * N, dtype=torch.bool)
    zero[torch.randperm(V * N, generator=g)[:(V * N) // 3]] = True
    zero = zero.reshape(V, N)
    if N >= 2:
        zero[:, N - 1] = True
    if V >= 2:
        zero[0, 0], zero[1, 0] = True, False
    factors[zero] = 0.0
    case.update(factors=factors.float(), zero=zero)
    return case


@functools.lru_cache(maxsize=None)
def factor_reference(deg, V, N, form="shared", scale=1.0, dtype=F64):
    c = factor_case(deg, V, N, form)
    return dense_from_factors(deg, c["means"], c["campos"], c["factors"], c["ids"], c["pose"], c["rdx"], scale, 16, dtype)


@functools.lru_cache(maxsize=None)
def node_case(sh_degree, step):
    """The arguments of nodes.rigid_gaussians: 300 points, a third of them bound to two actors, (sh_degree + 1)^2 coefficient rows, and an upstream
    gradient for every entry of the returned dictionary."""
    r, n, g = _gen(11000 + 100 * sh_degree + step // 1000)
    N = NODE_POINTS
    ids = torch.full((N,), -1, dtype=torch.int64)
    ids[torch.randperm(N, generator=g)[:N // 3]] = torch.randint(0, NODE_ACTORS, (N // 3,), generator=g)
    f = lambda t: t.float().contiguous()
    return dict(sh_degree=sh_degree, step=step, n=min(step // NODE_INTERVAL, sh_degree), means=f(0.5 * n(N, 3)), quats=f(n(N, 4)),
                opacity_logits=f(n(N, 1)), log_scales=f(0.3 * n(N, 3) - 1.0), features_dc=f(n(N, 3)), features_rest=f(n(N, (sh_degree + 1) ** 2 - 1, 3)),
                point_ids=ids, actor_pose=f(_pose_tables(r, n, 1, NODE_ACTORS)[0]), camera_center=f(6.0 * F.normalize(n(3), dim=-1)),
                g_means=f(n(N, 3)), g_opacities=f(n(N, 1)), g_rgbs=f(n(N, 3)), g_scales=f(n(N, 3)), g_quats=f(n(N, 4)))


@functools.lru_cache(maxsize=None)
def node_reference(sh_degree, step, dtype=F64):
    """_rgbs = clamp(sh_colour(n, cat(features_dc, features_rest), world_means.detach() - camera_center) + 0.5, 0, 1) and its gradients."""
    c = node_case(sh_degree, step)
    wm = world_means(c["means"], c["point_ids"], c["actor_pose"], None, dtype).detach()
    colors = torch.cat((c["features_dc"][:, None, :], c["features_rest"]), dim=1)
    out = sh_grads(c["n"], colors, wm - c["camera_center"].to(dtype), c["g_rgbs"], dtype, post=lambda x: torch.clamp(x + 0.5, 0.0, 1.0))
    out.update(d_features_dc=out["d_coeffs"][:, 0], d_features_rest=out["d_coeffs"][:, 1:], world_means=wm)
    return out


@functools.lru_cache(maxsize=None)
def precompute_case(deg):
    """The arguments of model.pre_compute_colors: 16 coefficient rows, means in a unit box, the camera 3 from the origin."""
    r, n, _ = _gen(13000 + deg)
    N = NODE_POINTS
    return dict(deg=deg, K=(deg + 1) ** 2, shs=n(N, 16, 3).float(), xyz=(r(N, 3) - 0.5).float(), camera_center=(3.0 * F.normalize(n(3), dim=-1)).float(),
                g=n(N, 3).float())


@functools.lru_cache(maxsize=None)
def precompute_reference(deg, dtype=F64):
    """clamp_min(sh_colour(deg, shs, xyz - camera_center) + 0.5, 0); dL/dxyz = dL/ddirs."""
    c = precompute_case(deg)
    dirs = c["xyz"].to(dtype) - c["camera_center"].to(dtype).reshape(1, 3)
    return sh_grads(deg, c["shs"], dirs, c["g"], dtype, post=lambda x: torch.clamp_min(x + 0.5, 0.0))
