"""Linear-blend skinning of SMPL pedestrian nodes, host side: the 24-joint kinematic chain and the per-point
blend / transform / quaternion composition through the HIP kernels of csrc/skinning.hip, two launches each way, no float atomics.

Mirrors (behaviour restated as the formulas of include/emd_raster.h, pinned by tests/skinning_ref.py; not copied):
  SMPLTemplate.forward                     OmniRe/models/human_body.py:158-181   -> joint_transforms
  SMPLNodes.transform_means_and_quats      OmniRe/models/nodes/smpl.py:438-532   -> skin_gaussians
What stays in torch with the caller: loading the SMPL template, betas -> rest joints, the skinning weights of a point (kNN to template
vertices or a voxel grid), the pose-refinement schedule, and the test-time pose interpolation on `theta` / `trans` (`motion.interpolate_quats`),
the same split as between `build_actor_pose` and `actor_pose_table`.

Every gradient is a fixed function of the call's inputs: bit-identical from run to run, across streams and under hipGraph replay.  There is no
`deterministic=` switch because there is no other mode."""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L

SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)
J = L.SKIN_JOINTS

_parents_cache = {}
_CHECKER = " (the checker's restatement is tests/skinning_ref.py)"       # behind the operator's name in a refusal of CPU tensors


def _parents_dev(parents, device):
    """The parent table as a device int32[24], built once per (table, device)."""
    tab = tuple(int(x) for x in (parents.tolist() if isinstance(parents, torch.Tensor) else parents))
    if len(tab) != J or tab[0] != -1 or any(not (0 <= tab[j] < j) for j in range(1, J)):
        raise ValueError(f"parents must list {J} joints with parents[0] = -1 and 0 <= parents[j] < j")
    key = (tab, str(device))
    if key not in _parents_cache:
        _parents_cache[key] = torch.tensor(tab, dtype=torch.int32, device=device)
    return _parents_cache[key]


# What a forward saw of the layout (the SkinLayout may be prepared for another point set before the backward runs)
PointLayout = namedtuple("PointLayout", "ids32 order chunks chunk_start num_chunks num_instances")


class SkinLayout:
    """Where each instance's points are, for the skinning backward: an instance's points are not contiguous after densification (new points
    are appended), and the backward sums over an instance's points in chunks of at most 256.  Built with torch ops once per point set and
    cached on the id tensor's identity, version, pointer and size (as `TrackOffsetHeads._prepare_ids`); one host read per point set (the
    chunk count, with the sortedness flag and the id range check), none per step.  `prepare(point_ids)` returns the `PointLayout`:

      ids32        [N] int32
      order        [N] int32, a STABLE argsort of the ids (all ids < 0 first, as one group), or None when the ids are already sorted
      chunks       [C,3] int32 rows (instance or -1, first position in `order`, count <= 256); ceil(n_p / 256) chunks per instance
      chunk_start  [P+1] int32: instance p owns the chunks [chunk_start[p], chunk_start[p+1])
    """
    CHUNK = L.SKIN_CHUNK

    def __init__(self, num_instances):
        self.num_instances = int(num_instances)
        if self.num_instances <= 0:
            raise ValueError("SkinLayout needs at least one instance")
        self._key = None

    def invalidate(self):
        """Forget the cached layout (call after any change of the point set: densification, pruning).  The cache key also carries the id
        tensor's version counter, so in-place edits are seen without it."""
        self._key = None

    def prepare(self, point_ids):
        ids = point_ids[..., 0] if point_ids.dim() == 2 else point_ids
        key = (id(point_ids), point_ids._version, point_ids.data_ptr(), point_ids.numel(), point_ids.dtype)
        if self._key == key:
            return self._layout
        P, dev, N = self.num_instances, ids.device, ids.numel()
        ids32 = ids.to(torch.int32).contiguous()
        if N == 0:
            self._layout = PointLayout(ids32, None, torch.zeros(0, 3, dtype=torch.int32, device=dev),
                                       torch.zeros(P + 1, dtype=torch.int32, device=dev), 0, P)
            self._key, self._ref = key, point_ids
            return self._layout
        group = ids.long().clamp_min(-1) + 1                                      # 0: unbound, 1 + p: instance p
        counts = torch.zeros(P + 2, dtype=torch.long, device=dev)
        counts.scatter_add_(0, group.clamp_max(P + 1), torch.ones_like(group))    # slot P + 1: ids beyond the table
        is_sorted = (group[1:] >= group[:-1]).all()
        counts = counts[:P + 1]
        nch = (counts + self.CHUNK - 1) // self.CHUNK
        zero = torch.zeros(1, dtype=torch.long, device=dev)
        seg_first = torch.cat([zero, counts.cumsum(0)])                           # [P + 2] first position of a group
        ch_first = torch.cat([zero, nch.cumsum(0)])                               # [P + 2] first chunk of a group
        C_, sorted_, bound = torch.stack([ch_first[-1], is_sorted.long(), seg_first[-1]]).tolist()     # the host read
        if bound != N:
            raise ValueError(f"point_ids hold {N - bound} ids >= num_instances = {P}")
        c = torch.arange(C_, device=dev)
        grp = torch.searchsorted(ch_first[1:], c, right=True)
        local = c - ch_first[grp]
        first = seg_first[grp] + local * self.CHUNK
        count = torch.minimum(counts[grp] - local * self.CHUNK, torch.full_like(local, self.CHUNK))
        chunks = torch.stack([grp - 1, first, count], dim=1).to(torch.int32).contiguous()
        order = None if sorted_ else torch.argsort(group, stable=True).to(torch.int32).contiguous()
        self._layout = PointLayout(ids32, order, chunks, ch_first[1:].to(torch.int32).contiguous(), int(C_), P)
        self._key, self._ref = key, point_ids                                     # (the reference keeps id() from being reused)
        return self._layout


def _chain_args(theta, joints, parents_dev, canon_inv, A):
    a = L.EmdJointChainArgs()
    a.num_instances = theta.shape[0] if theta is not None else A.shape[0]
    a.theta, a.joints, a.parents, a.canon_inv, a.A = L.ptr(theta), L.ptr(joints), L.ptr(parents_dev), L.ptr(canon_inv), L.ptr(A)
    return a


def _chain_forward(theta, joints, parents_dev, canon_inv):
    if theta.dim() != 3 or theta.shape[1:] != (J, 4) or joints.shape != (theta.shape[0], J, 3):
        raise ValueError(f"theta must be [P,{J},4] and joints [P,{J},3]")
    if canon_inv is not None and canon_inv.shape != (theta.shape[0], J, 12):
        raise ValueError(f"canon_inv must be [P,{J},12] (row-major 3x4)")
    A = torch.empty(theta.shape[0], J, 12, device=theta.device, dtype=torch.float32)
    a = _chain_args(theta, joints, parents_dev, canon_inv, A)
    L.launch("emd_joint_chain_forward", C.byref(a))
    return A


def _skin_args(means, quats, opac, weights, A, trans, valid, lay, outs=(None, None, None)):
    N, P = means.shape[0], A.shape[0]
    if quats.shape != (N, 4) or opac.shape != (N,) or weights.shape != (N, J) or lay.ids32.shape != (N,):
        raise ValueError(f"skin_gaussians: means [N,3], quats [N,4], opacities [N], point_ids [N], weights [N,{J}]")
    if A.shape[1:] != (J, 12) or trans.shape != (P, 3) or (valid is not None and valid.shape != (P,)) or lay.num_instances != P:
        raise ValueError(f"skin_gaussians: A [P,{J},12], trans [P,3], valid [P] and a layout of P instances")
    a = L.EmdSkinArgs()
    a.num_points, a.num_instances, a.num_chunks = N, P, lay.num_chunks
    a.means, a.quats, a.opacities, a.ids, a.weights = means.data_ptr(), quats.data_ptr(), opac.data_ptr(), lay.ids32.data_ptr(), weights.data_ptr()
    a.A, a.trans, a.valid, a.order, a.chunks = A.data_ptr(), trans.data_ptr(), L.ptr(valid), L.ptr(lay.order), lay.chunks.data_ptr()
    a.world_means, a.world_quats, a.opacities_out = (L.ptr(o) for o in outs)
    return a


def _skin_forward(means, quats, opac, weights, A, trans, valid, lay):
    outs = (torch.empty_like(means), torch.empty_like(quats), torch.empty_like(opac))
    a = _skin_args(means, quats, opac, weights, A, trans, valid, lay, outs)
    L.launch("emd_skin_forward", C.byref(a))
    return outs


def _skin_backward(means, quats, opac, weights, A, trans, valid, lay, g_wm, g_wq, g_wo, want_weights):
    """-> d_means, d_quats, d_opac, d_weights or None, partials [C, 291] (from torch's allocator: under capture, from the graph's pool)."""
    c = lambda t: t.contiguous().float()
    g_wm, g_wq, g_wo = c(g_wm), c(g_wq), c(g_wo)
    d_means, d_quats, d_opac = torch.empty_like(means), torch.empty_like(quats), torch.empty_like(opac)
    d_w = torch.empty_like(weights) if want_weights else None
    partials = torch.empty(lay.num_chunks, L.SKIN_PARTIAL_FLOATS, device=means.device, dtype=torch.float32)
    a = _skin_args(means, quats, opac, weights, A, trans, valid, lay)
    g = L.EmdSkinGrads()
    g.g_world_means, g.g_world_quats, g.g_opacities_out = g_wm.data_ptr(), g_wq.data_ptr(), g_wo.data_ptr()
    g.d_means, g.d_quats, g.d_opacities, g.d_weights, g.partials = d_means.data_ptr(), d_quats.data_ptr(), d_opac.data_ptr(), L.ptr(d_w), partials.data_ptr()
    L.launch("emd_skin_backward", C.byref(a), C.byref(g))
    return d_means, d_quats, d_opac, d_w, partials


class _JointChain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, joints, parents_dev, canon_inv):
        A = _chain_forward(theta, joints, parents_dev, canon_inv)
        ctx.save_for_backward(theta, joints, parents_dev, canon_inv)
        return A

    @staticmethod
    def backward(ctx, g_A):
        theta, joints, parents_dev, canon_inv = ctx.saved_tensors
        g_A = g_A.contiguous().float()
        d_theta = torch.empty_like(theta)
        a = _chain_args(theta, joints, parents_dev, canon_inv, None)
        L.launch("emd_joint_chain_backward", C.byref(a), g_A.data_ptr(), None, None, None, None, d_theta.data_ptr())
        return d_theta, None, None, None


class _Skin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, opac, weights, A, trans, valid, lay):
        outs = _skin_forward(means, quats, opac, weights, A, trans, valid, lay)
        ctx.save_for_backward(means, quats, opac, weights, A, trans, valid)
        ctx.lay = lay
        return outs

    @staticmethod
    def backward(ctx, g_wm, g_wq, g_wo):
        means, quats, opac, weights, A, trans, valid = ctx.saved_tensors
        lay = ctx.lay
        d_means, d_quats, d_opac, d_w, partials = _skin_backward(means, quats, opac, weights, A, trans, valid, lay, g_wm, g_wq, g_wo,
                                                                 ctx.needs_input_grad[3])
        dA = d_trans = None
        if ctx.needs_input_grad[4] or ctx.needs_input_grad[5]:
            # the per-instance sums: an instance's chunk slabs added in ascending chunk order (the first half of k_joint_chain_backward)
            dA, d_trans = torch.empty_like(A), torch.empty_like(trans)
            a = _chain_args(None, None, None, None, A)
            L.launch("emd_joint_chain_backward", C.byref(a), None, partials.data_ptr(), lay.chunk_start.data_ptr(), dA.data_ptr(),
                     d_trans.data_ptr(), None)
        return d_means, d_quats, d_opac, d_w, dA, d_trans, None, None


class _PosedSkin(torch.autograd.Function):
    """joint_transforms + skin_gaussians as ONE node: two launches forward, and two backward -- k_skin_backward leaves the chunk slabs and
    k_joint_chain_backward adds them, which gives dL/dA and dL/dtrans, and runs the chain in reverse in the same launch."""

    @staticmethod
    def forward(ctx, means, quats, opac, weights, theta, joints, trans, valid, parents_dev, canon_inv, lay):
        A = _chain_forward(theta, joints, parents_dev, canon_inv)
        outs = _skin_forward(means, quats, opac, weights, A, trans, valid, lay)
        ctx.save_for_backward(means, quats, opac, weights, theta, joints, trans, valid, parents_dev, canon_inv, A)
        ctx.lay = lay
        return outs

    @staticmethod
    def backward(ctx, g_wm, g_wq, g_wo):
        means, quats, opac, weights, theta, joints, trans, valid, parents_dev, canon_inv, A = ctx.saved_tensors
        lay = ctx.lay
        d_means, d_quats, d_opac, d_w, partials = _skin_backward(means, quats, opac, weights, A, trans, valid, lay, g_wm, g_wq, g_wo,
                                                                 ctx.needs_input_grad[3])
        d_theta, d_trans = torch.empty_like(theta), torch.empty_like(trans)
        a = _chain_args(theta, joints, parents_dev, canon_inv, None)
        L.launch("emd_joint_chain_backward", C.byref(a), None, partials.data_ptr(), lay.chunk_start.data_ptr(), None, d_trans.data_ptr(),
                 d_theta.data_ptr())
        return d_means, d_quats, d_opac, d_w, d_theta, None, d_trans, None, None, None, None


def _f(t):
    return None if t is None else t.contiguous().float()


def _valid_floats(valid):
    return None if valid is None else valid.reshape(-1).to(torch.float32).contiguous()


def joint_transforms(theta, joints, parents=SMPL_PARENTS, canon_inv=None):
    """A [P,24,12]: the skinning matrices (row-major 3x4) of P posed instances, one HIP launch (and one for the backward).
    theta [P,24,4]: unnormalised joint quaternions (w, x, y, z), row 0 the global orientation (the caller concatenates `instances_quats` and
    `smpl_qauts`); joints [P,24,3]: rest-pose joint positions; canon_inv [P,24,12]: the inverse of the canonical "da-pose" transforms, composed
    on the right.  The gradient goes to theta, through the normalisation; joints and canon_inv are buffers in the reference and get none."""
    L.need_device("joint_transforms" + _CHECKER, theta)
    return _JointChain.apply(_f(theta), _f(joints).detach(), _parents_dev(parents, theta.device), None if canon_inv is None else _f(canon_inv).detach())


def _layout_for(layout, point_ids, num_instances):
    lay = layout if layout is not None else SkinLayout(num_instances)        # no layout kept by the caller: built per call (one host read)
    return lay.prepare(point_ids)


def skin_gaussians(means, quats, opacities, point_ids, weights, A, trans, valid=None, layout=None):
    """world_means, world_quats (already `quat_act`-ed), opacities * valid[instance] -- one HIP launch, differentiable in means, quats, opacities,
    weights, A and trans.  point_ids [N]: the instance of a point, or < 0 (returned as `transform_gaussians` returns a static point);
    weights [N,24]: dense skinning weights; A: `joint_transforms`; layout: a `SkinLayout` the caller keeps between steps (and invalidates when
    the point set changes) -- without one the layout is rebuilt, with its host read, on every call."""
    L.need_device("skin_gaussians" + _CHECKER, means)
    lay = _layout_for(layout, point_ids, A.shape[0])
    return _Skin.apply(_f(means), _f(quats), _f(opacities).reshape(-1), _f(weights), _f(A), _f(trans), _valid_floats(valid), lay)


def posed_skin_gaussians(means, quats, opacities, point_ids, weights, theta, joints, trans, valid=None, parents=SMPL_PARENTS, canon_inv=None,
                         layout=None):
    """`skin_gaussians(..., joint_transforms(theta, joints, parents, canon_inv), ...)` as one autograd node: the same values and, bit for bit,
    the same gradients, with two launches each way (the per-instance sums and the reverse chain share a launch)."""
    L.need_device("posed_skin_gaussians" + _CHECKER, means)
    lay = _layout_for(layout, point_ids, theta.shape[0])
    return _PosedSkin.apply(_f(means), _f(quats), _f(opacities).reshape(-1), _f(weights), _f(theta), _f(joints).detach(), _f(trans),
                            _valid_floats(valid), _parents_dev(parents, theta.device), None if canon_inv is None else _f(canon_inv).detach(), lay)
