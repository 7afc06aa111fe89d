"""The contract of emd_amd.smpl in plain torch, fp64 on the CPU: the 24-joint kinematic chain and linear-blend skinning exactly as
include/emd_raster.h states them, restated from OmniRe's SMPLTemplate.forward (human_body.py:158-181) and
SMPLNodes.transform_means_and_quats (smpl.py:438-532) with pytorch3d's matrix_to_quaternion.  The reference's own files are not available
to record a golden from, so this restatement IS the pinned contract; it follows the formulation of the reference --
a Python loop over the joints of 4x4 products, an [N,24] x [N,24,16] blend, a bmm, four quaternion candidates, a quaternion product -- and
shares no code with the kernels.  The functions follow their inputs' dtype and device (profiles/skinning_microbench.py times them in fp32 on
the GPU as the yardstick).  `make_case` builds the inputs the CPU and the GPU tests share."""
import math

import torch

SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)
PATH_PARENTS = tuple(j - 1 for j in range(24))
STAR_PARENTS = (-1,) + (0,) * 23
J = 24


def quat_to_R(q):
    """Rotation of q / |q|, q = (w, x, y, z): [..., 3, 3]."""
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(*q.shape[:-1], 3, 3)


def _to44(R, t):
    top = torch.cat([R, t[..., None]], -1)
    bottom = torch.zeros(*R.shape[:-2], 1, 4, dtype=R.dtype, device=R.device)
    bottom[..., 0, 3] = 1
    return torch.cat([top, bottom], -2)


def joint_chain(theta, joints, parents=SMPL_PARENTS, canon_inv=None):
    """A [P,24,12] (row-major 3x4)."""
    R = quat_to_R(theta)                                                    # [P,24,3,3]
    G = [None] * J
    for j in range(J):
        if parents[j] < 0:
            G[j] = _to44(R[:, j], joints[:, j])
        else:
            G[j] = G[parents[j]] @ _to44(R[:, j], joints[:, j] - joints[:, parents[j]])
    G = torch.stack(G, 1)                                                   # [P,24,4,4]
    eye = torch.eye(3, dtype=theta.dtype, device=theta.device).expand(*joints.shape[:2], 3, 3)
    A = G @ _to44(eye, -joints)                                             # [G.R | G.t - G.R joints]
    if canon_inv is not None:
        C = canon_inv.reshape(*canon_inv.shape[:2], 3, 4)
        A = A @ _to44(C[..., :3], C[..., 3])
    return A[..., :3, :].reshape(*A.shape[:2], 12)


def _sqrt_positive_part(x):
    pos = x > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, x, torch.ones_like(x))), torch.zeros_like(x))


def matrix_to_quaternion(M):
    """pytorch3d's matrix_to_quaternion (real part first, not normalised, no sign standardisation) -> (quaternion [...,4], q_abs [...,4])."""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = M.reshape(*M.shape[:-2], 9).unbind(-1)
    q_abs = _sqrt_positive_part(torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1))
    cand = torch.stack([torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], -1),
                        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], -1),
                        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], -1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], -1)], -2)
    cand = cand / (2.0 * q_abs[..., None].clamp_min(0.1))
    best = q_abs.argmax(-1)                                                 # the first of equal maxima
    return torch.gather(cand, -2, best[..., None, None].expand(*best.shape, 1, 4)).squeeze(-2), q_abs


def quat_mult(a, b):
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def quat_act(q):
    return torch.nn.functional.normalize(q, dim=-1)


def skin(means, quats, opacities, ids, weights, A, trans, valid=None):
    """-> world_means, world_quats, opacities_out, q_abs [N,4] (of the bound points; zeros elsewhere)."""
    ids = ids.long()
    bound = ids >= 0
    p = ids.clamp_min(0)
    A44 = _to44(A.reshape(*A.shape[:2], 3, 4)[..., :3], A.reshape(*A.shape[:2], 3, 4)[..., 3])          # [P,24,4,4]
    T = (weights[:, :, None] * A44[p].reshape(-1, J, 16)).sum(1).reshape(-1, 4, 4)                    # [N,24] x [N,24,16]
    hom = torch.cat([means, torch.ones_like(means[:, :1])], -1)
    wm = torch.bmm(T, hom[:, :, None])[:, :3, 0] + trans[p]
    qm, q_abs = matrix_to_quaternion(T[:, :3, :3])
    wq = quat_act(quat_mult(qm, quat_act(quats)))
    v = torch.ones(A.shape[0], dtype=means.dtype, device=means.device) if valid is None else valid.to(means.dtype)
    wo = opacities * v[p]
    b = bound[:, None]
    return torch.where(b, wm, means), torch.where(b, wq, quats), torch.where(bound, wo, opacities), q_abs * b


def criterion(got, ref, what, rows=None):
    """element-wise |got - ref| <= 1e-4 |ref| + 1e-6 max |ref| and relative L2 <= 1e-5 (rows: the rows compared)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    scale = float(ref.abs().max())
    err = (got - ref).abs()
    worst = float((err / (1e-4 * ref.abs() + 1e-6 * scale + 1e-300)).max()) if ref.numel() else 0.0
    l2 = float((got - ref).norm() / ref.norm().clamp_min(1e-300)) if ref.numel() else 0.0
    print(f"{what}: worst element at {worst:.3f} of its bound, relative L2 {l2:.2e}")
    assert worst <= 1.0, (what, worst)
    assert l2 <= 1e-5, (what, l2)


COUNTS = (1, 70, 300, 0, 129)            # less than a wave, more than a wave, more than one chunk, an empty instance, one past a wave multiple
INVALID = 1
TIE_GAP = 1e-3


def make_case(parents=SMPL_PARENTS, canon=False, shuffled=False, seed=11):
    """fp32 CPU tensors of one test case.  The sorted and the shuffled layout hold the SAME bound points (the shuffled one adds 17 unbound rows);
    `perm` maps a row of the shuffled layout to its row in the sorted one (-1: unbound)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    P, N = len(COUNTS), sum(COUNTS)
    axis = torch.nn.functional.normalize(n(P, J, 3), dim=-1)
    ang = r(P, J, 1) * math.pi
    theta = torch.cat([torch.cos(ang / 2), torch.sin(ang / 2) * axis], -1) * (0.5 + r(P, J, 1))
    joints, trans = 0.3 * n(P, J, 3), 5.0 * n(P, 3)
    cq, ct = n(P, J, 4), 0.2 * n(P, J, 3)
    canon_inv = torch.cat([quat_to_R(cq), ct[..., None]], -1).reshape(P, J, 12)
    ids = torch.repeat_interleave(torch.arange(P), torch.tensor(COUNTS))
    w = r(N, J) ** 4
    d = dict(means=0.5 * n(N, 3), quats=n(N, 4), opacities=r(N), weights=w / w.sum(-1, keepdim=True), ids=ids,
             g_wm=n(N, 3), g_wq=n(N, 4), g_wo=n(N))
    perm = torch.arange(N)
    if shuffled:
        U = 17
        slot = torch.randperm(N + U, generator=g)
        perm = torch.full((N + U,), -1, dtype=torch.long)
        perm[slot[:N]] = torch.arange(N)
        extra = dict(means=n(U, 3), quats=n(U, 4), opacities=r(U), weights=torch.zeros(U, J, dtype=torch.float64), ids=torch.full((U,), -1),
                     g_wm=n(U, 3), g_wq=n(U, 4), g_wo=n(U))
        for k in d:
            full = torch.cat([d[k], extra[k]])
            out = torch.empty_like(full)
            out[slot] = full
            d[k] = out
    valid = torch.ones(P, dtype=torch.bool)
    valid[INVALID] = False
    f = lambda t: t.float().contiguous()
    case = {k: (v.to(torch.int64) if k == "ids" else f(v)) for k, v in d.items()}
    case.update(theta=f(theta), joints=f(joints), trans=f(trans), valid=valid, canon_inv=f(canon_inv) if canon else None,
                parents=tuple(parents), perm=perm, P=P)
    return case


def reference(case):
    """fp64 values and gradients of a case under the contract.  Points whose two largest q_abs differ by less than TIE_GAP sit on a branch
    boundary of matrix_to_quaternion: `tie` marks them, and their upstream quaternion gradient is taken as zero (returned as g_wq)."""
    D = lambda t: None if t is None else t.double()
    leaf = lambda t: t.double().clone().requires_grad_(True)
    theta, means, quats, opac, weights, trans = (leaf(case[k]) for k in ("theta", "means", "quats", "opacities", "weights", "trans"))
    A = joint_chain(theta, D(case["joints"]), case["parents"], D(case["canon_inv"]))
    A.retain_grad()
    wm, wq, wo, q_abs = skin(means, quats, opac, case["ids"], weights, A, trans, case["valid"])
    top = q_abs.detach().sort(-1, descending=True).values
    bound = case["ids"] >= 0
    tie = bound & ((top[:, 0] - top[:, 1]) < TIE_GAP)
    g_wq = torch.where(tie[:, None], torch.zeros_like(case["g_wq"]), case["g_wq"])
    ((wm * D(case["g_wm"])).sum() + (wq * D(g_wq)).sum() + (wo * D(case["g_wo"])).sum()).backward()
    branch = q_abs.detach().argmax(-1)[bound & ~tie]
    return dict(A=A.detach(), wm=wm.detach(), wq=wq.detach(), wo=wo.detach(), tie=tie, g_wq=g_wq, branch_counts=torch.bincount(branch, minlength=4),
                d_theta=theta.grad, d_means=means.grad, d_quats=quats.grad, d_opacities=opac.grad, d_weights=weights.grad, d_trans=trans.grad,
                d_A=A.grad)
