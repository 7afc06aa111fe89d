"""Per-class Gaussian dictionaries of the OmniRe flow on the HIP path.

`rigid_gaussians` is RigidNodes.get_gaussians (OmniRe/models/nodes/rigid.py:570-615): world means / quaternions through the
per-actor rigid transform, opacity x validity of (frame, actor), SH colour on DETACHED world view directions clamped to [0, 1],
exp scales -- the dictionary `collect_gaussians` (models/trainers/base.py:342-383) concatenates over classes before the
`rasterization` call.  `deformable_gaussians` is DeformableNodes.get_gaussians (models/nodes/deformable.py:49-114): the learned
residual of `ConditionalDeformNetwork` is added to the (detached) canonical means and to the normalised quaternions first.
`smpl_gaussians` is SMPLNodes.get_gaussians (models/nodes/smpl.py): the per-point blend of 24 joint transforms of `emd_amd.smpl`.
Two HIP launches per class (`emd_motion_forward`, `emd_sh_forward`) instead of the reference's Python loop over actors; the
NaN / Inf guard of the reference (ten `.any()` host syncs per class and step) is one reduction and one sync, and can be
switched off.  (When the caller uses this repository's GaussianRasterizer directly, the same transform and SH evaluation are
fused into its projection kernel and none of this is needed: EMD_FLAG_MOTION.)

`vanilla_gaussians` is VanillaGaussians.get_gaussians (models/gaussians/vanilla.py:378-414), the class without a transform -- the Background,
the large majority of a scene's Gaussians: the three activations and the SH colour in ONE launch each way (`emd_vanilla_forward` /
`emd_vanilla_backward`, csrc/vanilla.hip), with `features_dc` and `features_rest` read where they are (no `torch.cat`).

`RigidNodes` / `DeformableNodes` are the actor classes as stores (models/nodes/rigid.py, deformable.py): `VanillaGaussians` plus the actor tables,
`point_ids`, per-point embeddings, `get_gaussians` through the functions above, and the refinement event with the per-box cull and the rows
grouped by actor (`density.restructure_node_rows`, csrc/densify.hip).  `SMPLNodes` is the pedestrian class as a store
(models/nodes/smpl.py): the pose Parameters, `get_gaussians` through `smpl_gaussians`, the k-NN table inside each instance and the neighbour-std
regulariser `knn_reg` on it (`knn.KnnTable(segment_start=)`, `knn.neighbour_std`, csrc/neighbour_reg.hip)."""
import ctypes as C

import torch
from torch.nn import Parameter

from . import _lib as L
from .gsplat_api import spherical_harmonics
from .motion import transform_gaussians
from .vanilla import VanillaGaussians, _get


def _check_finite(gs, step):
    bad = torch.stack([~torch.isfinite(v).all() for v in gs.values()])
    if bool(bad.any()):                                          # one host sync (the reference: two per entry)
        for (k, v), b in zip(gs.items(), bad.tolist()):
            if b:
                kind = "NaN" if bool(torch.isnan(v).any()) else "Inf"
                raise ValueError(f"{kind} detected in gaussian {k} at step {step}")


def _colors(world_means, features_dc, features_rest, camera_center, sh_degree, step, sh_degree_interval):
    colors = torch.cat((features_dc[:, None, :], features_rest), dim=1)
    if sh_degree > 0:
        viewdirs = world_means.detach() - camera_center                           # (N, 3): no gradient to the means through colour
        viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
        n = min(step // sh_degree_interval, sh_degree)
        return torch.clamp(spherical_harmonics(n, viewdirs, colors) + 0.5, 0.0, 1.0)
    return torch.sigmoid(colors[:, 0, :])


def rigid_gaussians(means, quats, opacity_logits, log_scales, features_dc, features_rest, point_ids, actor_pose, camera_center,
                    sh_degree=3, step=0, sh_degree_interval=1000, check_finite=True, deterministic=False):
    """-> dict(_means, _opacities [N,1], _rgbs, _scales, _quats).  actor_pose: the [A,12] table of motion.build_actor_pose /
    actor_pose_table for the current frame (pose, learned track offsets, validity).  deterministic: as transform_gaussians."""
    ids = point_ids[..., 0] if point_ids.dim() == 2 else point_ids
    world_means, world_quats, opac = transform_gaussians(means, quats, torch.sigmoid(opacity_logits), ids, actor_pose,
                                                         deterministic=deterministic)
    gs = dict(_means=world_means, _opacities=opac.reshape(-1, 1),
              _rgbs=_colors(world_means, features_dc, features_rest, camera_center, sh_degree, step, sh_degree_interval),
              _scales=torch.exp(log_scales), _quats=world_quats)
    if check_finite:
        _check_finite(gs, step)
    return gs


def smpl_gaussians(means, quats, opacity_logits, log_scales, features_dc, features_rest, point_ids, weights, theta, joints, trans, valid,
                   camera_center, canon_inv=None, sh_degree=3, step=0, sh_degree_interval=1000, check_finite=True, layout=None):
    """SMPLNodes.get_gaussians (models/nodes/smpl.py): as rigid_gaussians, with the per-point blend of 24 joint transforms in place of one
    actor pose.  theta [P,24,4]: the frame's joint quaternions, row 0 the global orientation; joints [P,24,3]: rest joints; trans [P,3] and
    valid [P]: the frame's instance translations and validity; weights [N,24]: the points' skinning weights; layout: a `smpl.SkinLayout`
    kept between steps.  Two HIP launches each way for the pose and the skinning (`smpl.posed_skin_gaussians`), then `emd_sh_forward`."""
    from .smpl import posed_skin_gaussians
    world_means, world_quats, opac = posed_skin_gaussians(means, quats, torch.sigmoid(opacity_logits), point_ids, weights, theta, joints, trans,
                                                          valid=valid, canon_inv=canon_inv, layout=layout)
    gs = dict(_means=world_means, _opacities=opac.reshape(-1, 1),
              _rgbs=_colors(world_means, features_dc, features_rest, camera_center, sh_degree, step, sh_degree_interval),
              _scales=torch.exp(log_scales), _quats=world_quats)
    if check_finite:
        _check_finite(gs, step)
    return gs


def deformable_gaussians(network, means, quats, opacity_logits, log_scales, features_dc, features_rest, point_ids, actor_pose,
                         camera_center, instances_size, instances_embedding, t, sh_degree=3, step=0, sh_degree_interval=1000,
                         use_deformation=True, stop_optimizing_canonical_xyz=True, check_finite=True, deterministic=False):
    """DeformableNodes.get_gaussians: delta_xyz on the canonical means (detached when `stop_optimizing_canonical_xyz`), delta_quat on
    the normalised quaternions, delta_scale (when the network has that head) on the activated scales; then as rigid_gaussians
    (`deterministic` included: it covers the motion transform and, through `nonrigid_deformation(..., deterministic=True)`, the gradient of
    `instances_embedding` behind the encoder input; the layers of ConditionalDeformNetwork are covered when `network.fused` is set: they then run on
    the fixed-order kernels of csrc/deform_mlp.hip instead of rocBLAS)."""
    from .deformation import nonrigid_deformation
    ids = point_ids[..., 0] if point_ids.dim() == 2 else point_ids
    dx = dq = ds = None
    if use_deformation:
        dx, dq, ds = nonrigid_deformation(network, means, ids, instances_size, instances_embedding, t, deterministic=deterministic)
    base = means.detach() if (dx is not None and stop_optimizing_canonical_xyz) else means
    # the residuals enter the HIP transform as `residual_dx` / `residual_dq`, added before the rigid motion; the reference adds
    # delta_quat to get_quats = q / |q| (deformable.py:69), so the quaternions are normalised first when a residual is present
    q_in = quats / quats.norm(dim=-1, keepdim=True) if dq is not None else quats
    world_means, world_quats, opac = transform_gaussians(base, q_in, torch.sigmoid(opacity_logits), ids, actor_pose,
                                                         residual_dx=dx, residual_dq=dq, deterministic=deterministic)
    scales = torch.exp(log_scales)
    if ds is not None:
        scales = scales + ds
    gs = dict(_means=world_means, _opacities=opac.reshape(-1, 1),
              _rgbs=_colors(world_means, features_dc, features_rest, camera_center, sh_degree, step, sh_degree_interval),
              _scales=scales, _quats=world_quats)
    if check_finite:
        _check_finite(gs, step)
    return gs


class RigidNodes(VanillaGaussians):
    """OmniRe's RigidNodes (models/nodes/rigid.py) as a store: the parent's six per-point parameters in the ACTOR's frame, `point_ids` [N,1] int64
    (the reference's attribute; `ids32` is the int32 form the kernels read), the per-frame actor poses `instances_quats` [F,A,4] / `instances_trans`
    [F,A,3] (Parameters), `instances_size` [A,3], `instances_fv` [F,A] bool, `cur_frame`, and -- with ctrl `gaussian_embedding_dim` > 0 -- the
    per-point `_embeddings` [N,E] behind the learned track offsets of an attached `motion.TrackOffsetHeads`.

    `refinement_after` and the event's body `_refine` are the parent's (schedule, opacity reset, the rows that travel, their install); the class
    overrides the four hooks of that body -- `_refine_args` (the actor part of an EmdRefineNodesArgs behind the parent's fill), `_refine_attrs`
    (`_embeddings`), `_refine_rows` and `_after_refine` (ids, segment table, track heads).  The driver is `density.restructure_node_rows`: the
    parent's decisions plus ctrl `cull_out_of_bound` (default False: a row, a split sample at its sampled position included, is culled when it leaves its actor's box) and
    ctrl `group_by_actor` (default True: the output rows are grouped by actor, so an actor's points stay contiguous for the whole run and
    `segment_start` [A+1] is their table; the reference appends new rows at the end).  All parameters, `_embeddings` and both Adam moments of each
    travel through the one gather; `point_ids`, `ids32` and `segment_start` come from the event's index stage; an attached `track_heads` adopts the
    new layout without a host read.  The pose-smoothness regulariser of rigid.py:636-706 acts on the [F,A,3] tables of a few dozen actors and is left
    to the trainer's torch code; `after_train` and `compute_reg_loss` are the parent's."""
    # optimiser group (after the class prefix) -> attribute, beside the parent's six.  The reference file is not at hand: the names are kept in this one
    # table (INTEGRATION.md says how to change them).
    NODE_PARAM_GROUPS = {"ins_rotation": "instances_quats", "ins_translation": "instances_trans", "embedding": "_embeddings",
                         "smpl_rotation": "smpl_quats"}          # (the last: SMPLNodes only; a class without the attribute has no such group)

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.point_ids = torch.zeros(1, 1, dtype=torch.int64, device=self.device)
        self.ids32 = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._ids_flat = self.point_ids.reshape(-1)
        self.instances_quats = self.instances_trans = self.instances_size = self.instances_fv = None
        self._embeddings = None
        self.segment_start = None
        self.cur_frame = 0
        self.track_heads = None

    num_actors = property(lambda self: self.instances_size.shape[0])
    num_frames = property(lambda self: self.instances_quats.shape[0])
    embedding_dim = property(lambda self: int(_get(self.ctrl_cfg, "gaussian_embedding_dim", 0) or 0))

    def create_from_tensors(self, means, colors, log_scales, point_ids, instances_quats, instances_trans, instances_size, instances_fv, quats=None,
                            embeddings=None):
        """The parent's `create_from_tensors` on points in the actors' frames, plus the actor tables.  point_ids [N] or [N,1], any integer type;
        embeddings [N,E] (default zeros) when ctrl `gaussian_embedding_dim` = E > 0."""
        super().create_from_tensors(means, colors, log_scales, quats=quats)
        dev, n = self.device, means.shape[0]
        self._set_ids(point_ids.to(dev).reshape(n).to(torch.int32).contiguous(), None)
        self.instances_quats = Parameter(instances_quats.to(dev).float().contiguous())
        self.instances_trans = Parameter(instances_trans.to(dev).float().contiguous())
        self.instances_size = instances_size.to(dev).float().contiguous()
        self.instances_fv = instances_fv.to(dev).bool().contiguous()
        E = self.embedding_dim
        if E > 0:
            self._embeddings = Parameter((torch.zeros(n, E) if embeddings is None else embeddings).to(dev).float().reshape(n, E).contiguous())
        if self.track_heads is not None:
            self.track_heads.invalidate()

    def _set_ids(self, ids32, segment_start):
        self.ids32 = ids32
        self.point_ids = ids32.to(torch.int64)[:, None]
        self._ids_flat = self.point_ids.reshape(-1)                 # ONE object: the key of the track heads' layout cache
        self.segment_start = segment_start

    def attach_track_heads(self, heads):
        self.track_heads = heads
        if heads is not None:
            heads.invalidate()

    def set_cur_frame(self, frame):
        self.cur_frame = frame

    def get_param_groups(self):
        groups = self.get_gaussian_param_groups()
        for short, attr in self.NODE_PARAM_GROUPS.items():
            if getattr(self, attr, None) is not None:
                groups[self.class_prefix + short] = [getattr(self, attr)]
        return groups

    def get_out_of_bound_mask(self):
        """[N] bool: |mean_c| > instances_size[id]_c / 2 for any c (the rows `cull_out_of_bound` removes at the next event)."""
        return (self._means.detach().abs() > self.instances_size[self._ids_flat] / 2).any(dim=-1)

    def _actor_pose(self):
        from .motion import build_actor_pose
        h = self.track_heads
        if h is None:
            return build_actor_pose(self.instances_quats, self.instances_trans, self.instances_fv, self.cur_frame, in_test_set=self.in_test_set)
        if not self.in_test_set:
            return h.pose_table(self.instances_quats, self.instances_trans, self.instances_fv, self.cur_frame, self._embeddings, self._ids_flat, self.step)
        tt, tr = h(self.cur_frame, self.num_frames, self._embeddings, self._ids_flat, self.step)
        return build_actor_pose(self.instances_quats, self.instances_trans, self.instances_fv, self.cur_frame, tt, tr, in_test_set=True)

    def _node_kwargs(self, check_finite):
        c = self.ctrl_cfg
        return dict(sh_degree=self.sh_degree, step=self.step, sh_degree_interval=_get(c, "sh_degree_interval", 1000),
                    check_finite=bool(_get(c, "check_finite", True)) if check_finite is None else check_finite,
                    deterministic=bool(_get(c, "deterministic", False)))

    def get_gaussians(self, cam, check_finite=None):
        """rigid.py:570-615 through `rigid_gaussians`; the frame's pose table is `motion.build_actor_pose`, or `track_heads.pose_table` when a
        `TrackOffsetHeads` is attached."""
        self.filter_mask = torch.ones(self.num_points, dtype=torch.bool, device=self._means.device)
        return rigid_gaussians(self._means, self._quats, self._opacities, self._scales, self._features_dc, self._features_rest, self.point_ids,
                               self._actor_pose(), cam.camtoworlds[..., :3, 3], **self._node_kwargs(check_finite))

    # ---- the refinement event -----------------------------------------------------------------------------------------------------------------
    # (the body is the parent's `_refine`; these four say what an actor class adds)
    def _refine_args(self, do_densify, do_cull):
        c = self.ctrl_cfg
        a, keep = super()._refine_args(do_densify, do_cull, L.EmdRefineNodesArgs())          # (its first fields are EmdRefineArgs's)
        actor = [self._means.detach().contiguous(), self._quats.detach().contiguous(), self.ids32.contiguous(), self.instances_size.contiguous()]
        a.means, a.rotation, a.ids, a.instances_size = (t.data_ptr() for t in actor)
        a.num_actors, a.num_samples = self.num_actors, int(_get(c, "n_split_samples", 2))
        a.cull_out_of_bound, a.group_by_actor = int(bool(_get(c, "cull_out_of_bound", False))), int(bool(_get(c, "group_by_actor", True)))
        a.seed = (self.refine_seed * 0x9E3779B97F4A7C15 + self.refine_events) & 0xFFFFFFFFFFFFFFFF
        return a, keep + actor

    def _refine_attrs(self):
        attrs = super()._refine_attrs()
        if self._embeddings is not None:
            attrs["embedding"] = ("_embeddings", L.DENSIFY_ROLE_COPY)
        return attrs

    def _refine_rows(self, a, keep, jobs, N, samples):
        from .density import restructure_node_rows
        outs, ids_out, seg, (n_keep, n_dup, n_split, n_samp) = restructure_node_rows(a, jobs, N, samples=samples)
        return outs, (n_keep, n_dup, sum(n_samp), n_split), (ids_out, seg)

    def _after_refine(self, layout):
        ids_out, seg = layout
        self._set_ids(ids_out.contiguous(), seg)
        if self.track_heads is not None:
            if seg is not None:
                self.track_heads.adopt_layout(self._ids_flat, self.ids32, seg)
            else:
                self.track_heads.invalidate()


class DeformableNodes(RigidNodes):
    """OmniRe's DeformableNodes (models/nodes/deformable.py): RigidNodes whose canonical points take the learned residual of a
    `deformation.ConditionalDeformNetwork` first.  `set_deformation` supplies the network, the per-actor `instances_embedding` [A,D] and the
    frames' `normalized_timestamps` [F]; ctrl `use_deformation` (default True) and `stop_optimizing_canonical_xyz` (default True) as in the
    reference.  The refinement event is the parent's."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.deform_network = self.instances_embedding = self.normalized_timestamps = None

    def set_deformation(self, network, instances_embedding, normalized_timestamps):
        self.deform_network = network
        self.instances_embedding = instances_embedding if isinstance(instances_embedding, Parameter) else Parameter(instances_embedding.to(self.device).float().contiguous())
        self.normalized_timestamps = normalized_timestamps.to(self.device).float()

    def get_gaussians(self, cam, check_finite=None):
        """deformable.py:49-114 through `deformable_gaussians`, the pose table as in RigidNodes."""
        c = self.ctrl_cfg
        self.filter_mask = torch.ones(self.num_points, dtype=torch.bool, device=self._means.device)
        return deformable_gaussians(self.deform_network, self._means, self._quats, self._opacities, self._scales, self._features_dc, self._features_rest,
                                    self.point_ids, self._actor_pose(), cam.camtoworlds[..., :3, 3], self.instances_size, self.instances_embedding,
                                    self.normalized_timestamps[self.cur_frame].reshape(1), use_deformation=bool(_get(c, "use_deformation", True)),
                                    stop_optimizing_canonical_xyz=bool(_get(c, "stop_optimizing_canonical_xyz", True)), **self._node_kwargs(check_finite))


class SMPLNodes(RigidNodes):
    """OmniRe's SMPLNodes (models/nodes/smpl.py) as a store, the fourth class of `collect_gaussians`: the parent's six per-point parameters in the
    CANONICAL frame of each person, the per-frame pose Parameters `instances_quats` [F,P,4] (global orientation), `smpl_quats` [F,P,23,4] and
    `instances_trans` [F,P,3], and the buffers `joints` [P,24,3] (rest joints), `weights` [N,24] (skinning weights), `instances_fv` [F,P],
    `instances_size` [P,3] and optionally `canon_inv` [P,24,12].  Loading the SMPL template, betas -> joints and the voxel deformer stay with the
    caller: `create_from_tensors` takes their results.

    The rows are grouped by instance for the whole run (sorted once at creation, stable; `segment_start` [P+1] built on the device), because the
    class never changes its point set: `refinement_after` is the k-NN refresh every ctrl `knn_update_interval` (default 100) steps and nothing
    else -- the reading of the reference taken here, which replaces the densification hook by that refresh.  `compute_reg_loss` adds `knn_reg`
    (reg_cfg key `knn_reg` with `lambda_std_q`, `lambda_std_s`, `lambda_std_o`, `lambda_std_shs_dc`, `lambda_std_shs_rest`) to the parent's dict:
    the sum of the five terms of ONE `knn.neighbour_std` node over the table of each point's ctrl `knn_neighbors` - 1 (default 3 - 1) nearest points
    of the same person.  The reference's `x_offset`, voxel-deformer and temporal-smoothness terms are not built."""
    # reg_cfg weight -> (attribute, activation of the values the reference takes the std of).  Which blocks are activated is a reading: change it here.
    KNN_REG_BLOCKS = {"lambda_std_q": ("_quats", "identity"), "lambda_std_s": ("_scales", "exp"), "lambda_std_o": ("_opacities", "sigmoid"),
                      "lambda_std_shs_dc": ("_features_dc", "identity"), "lambda_std_shs_rest": ("_features_rest", "identity")}

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.knn_neighbors < 2:
            raise ValueError(f"SMPLNodes: knn_neighbors counts the point itself and must be at least 2, got {self.knn_neighbors}")
        self.smpl_quats = self.joints = self.weights = self.canon_inv = None
        self.skin_layout = self.knn_table = None

    knn_neighbors = property(lambda self: int(_get(self.ctrl_cfg, "knn_neighbors", 3)))
    knn_update_interval = property(lambda self: int(_get(self.ctrl_cfg, "knn_update_interval", 100)))

    def create_from_tensors(self, means, colors, log_scales, point_ids, instances_quats, smpl_quats, instances_trans, instances_size, instances_fv,
                            joints, weights, quats=None, canon_inv=None):
        """Points in the persons' canonical frames with their instance ids [N] or [N,1] and skinning weights [N,24]; the rows are sorted by
        instance here (stable), ids < 0 -- points bound to nobody -- first, outside every segment."""
        from .smpl import SkinLayout
        dev, n, P = self.device, means.shape[0], instances_size.shape[0]
        ids = point_ids.to(dev).reshape(n).to(torch.int64)
        order = torch.argsort(ids, stable=True)
        row = lambda t: t.to(dev)[order]
        super().create_from_tensors(row(means), row(colors), row(log_scales.reshape(n, -1)), ids[order], instances_quats, instances_trans,
                                    instances_size, instances_fv, quats=None if quats is None else row(quats))
        seg = torch.searchsorted(ids[order].contiguous(), torch.arange(P + 1, device=dev)).to(torch.int32)
        self._set_ids(self.ids32, seg)
        self.smpl_quats = Parameter(smpl_quats.to(dev).float().contiguous())
        self.joints = joints.to(dev).float().contiguous()
        self.weights = row(weights).float().contiguous()
        self.canon_inv = None if canon_inv is None else canon_inv.to(dev).float().contiguous()
        if self.smpl_quats.shape[:2] != self.instances_quats.shape[:2] or self.smpl_quats.shape[2:] != (23, 4):
            raise ValueError(f"SMPLNodes: smpl_quats must be [F,P,23,4] beside instances_quats [F,P,4], got {tuple(self.smpl_quats.shape)}")
        self.skin_layout = SkinLayout(P)                 # one layout for the whole run: the point set never changes
        self.knn_table = None

    def get_gaussians(self, cam, check_finite=None):
        """models/nodes/smpl.py through `smpl_gaussians`: theta = (global orientation, the 23 body joints) of the current frame."""
        f = self.cur_frame
        self.filter_mask = torch.ones(self.num_points, dtype=torch.bool, device=self._means.device)
        kw = self._node_kwargs(check_finite)
        kw.pop("deterministic")                          # (the skinning has no other mode)
        theta = torch.cat((self.instances_quats[f][:, None, :], self.smpl_quats[f]), dim=1)
        return smpl_gaussians(self._means, self._quats, self._opacities, self._scales, self._features_dc, self._features_rest, self._ids_flat,
                              self.weights, theta, self.joints, self.instances_trans[f], self.instances_fv[f], cam.camtoworlds[..., :3, 3],
                              canon_inv=self.canon_inv, layout=self.skin_layout, **kw)

    def update_knn(self):
        """(Re)build the table of each point's `knn_neighbors` - 1 nearest points of the same instance (`knn.KnnTable` over `segment_start`)."""
        from .knn import KnnTable
        k = self.knn_neighbors - 1
        if self.knn_table is None or self.knn_table.k != k:
            self.knn_table = KnnTable(self._means, k=k, segment_start=self.segment_start)
        else:
            self.knn_table.refresh(self._means, segment_start=self.segment_start)
        return self.knn_table

    def postprocess_per_train_step(self, step, optimizer, radii, xys_grad, last_size):
        self.after_train(radii, xys_grad, last_size)
        self.refinement_after(step, optimizer)           # (its own interval: ctrl `refine_interval` plays no part)

    def refinement_after(self, step, optimizer, samples=None):
        """The k-NN refresh at every `knn_update_interval`-th step; the point set, `point_ids` and the optimiser are left as they are."""
        assert step == self.step
        if step % self.knn_update_interval == 0:
            self.update_knn()
        self.xys_grad_norm = self.vis_counts = self.max_2Dsize = None
        return None

    def compute_reg_loss(self):
        """The parent's dict plus `knn_reg` when reg_cfg names it: the sum of the terms of one `neighbour_std` node (a block without rows -- SH
        degree 0 has no `_features_rest` -- is dropped).  The table is built on first use and whenever its point count is stale."""
        from .knn import neighbour_std
        out = super().compute_reg_loss()
        cfg = _get(self.reg_cfg, "knn_reg") if self.reg_cfg else None
        if not cfg:
            return out
        blocks, acts, weights = [], [], []
        for key, (attr, act) in self.KNN_REG_BLOCKS.items():
            x = getattr(self, attr)
            if x.numel() == 0 and self.num_points > 0:
                continue
            blocks.append(x)
            acts.append(act)
            weights.append(float(_get(cfg, key, 0.0) or 0.0))
        if self.knn_table is None or self.knn_table.N != self.num_points:
            self.update_knn()
        out["knn_reg"] = neighbour_std(blocks, self.knn_table, weights, acts).sum()
        return out


class _VanillaGaussians(torch.autograd.Function):
    """One node: (quats, opacity_logits, log_scales, features_dc, features_rest) -> (_opacities [N,1], _scales, _quats, _rgbs).  The means and
    the camera centre enter the colour detached, as in the reference."""

    @staticmethod
    def forward(ctx, means, quats, opacity_logits, log_scales, features_dc, features_rest, camera_center, degree, sh_mode):
        dev, n, M = means.device, means.shape[0], features_rest.shape[1] + 1
        a = L.EmdVanillaArgs()
        a.num_points, a.sh_coeffs, a.degree, a.sh_mode = n, M, int(degree), int(sh_mode)
        a.means, a.log_scales, a.quats, a.opacity_logits = means.data_ptr(), log_scales.data_ptr(), quats.data_ptr(), opacity_logits.data_ptr()
        a.features_dc, a.features_rest, a.camera_center = features_dc.data_ptr(), (features_rest.data_ptr() if M > 1 else None), camera_center.data_ptr()
        new = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        opac, scales, quats_out, rgbs = new(n, 1), new(n, 3), new(n, 4), new(n, 3)
        mask = torch.empty(n, device=dev, dtype=torch.uint8)
        a.opacities, a.scales, a.quats_out, a.rgbs, a.clamp_mask = opac.data_ptr(), scales.data_ptr(), quats_out.data_ptr(), rgbs.data_ptr(), mask.data_ptr()
        L.launch("emd_vanilla_forward", C.byref(a))
        ctx.save_for_backward(means, quats, opacity_logits, log_scales, features_dc, features_rest, camera_center, mask)
        ctx.cfg = (int(degree), int(sh_mode))
        ctx.set_materialize_grads(False)                     # an output nobody used arrives as None and goes in as NULL
        return opac, scales, quats_out, rgbs

    @staticmethod
    def backward(ctx, g_opac, g_scales, g_quats, g_rgbs):
        means, quats, opacity_logits, log_scales, features_dc, features_rest, camera_center, mask = ctx.saved_tensors
        dev, n, M = means.device, means.shape[0], features_rest.shape[1] + 1
        a = L.EmdVanillaArgs()
        a.num_points, a.sh_coeffs, a.degree, a.sh_mode = n, M, ctx.cfg[0], ctx.cfg[1]
        a.means, a.log_scales, a.quats, a.opacity_logits = means.data_ptr(), log_scales.data_ptr(), quats.data_ptr(), opacity_logits.data_ptr()
        a.features_dc, a.features_rest, a.camera_center = features_dc.data_ptr(), (features_rest.data_ptr() if M > 1 else None), camera_center.data_ptr()
        a.clamp_mask = mask.data_ptr()
        # a consumer's torch.cat or slice comes back as a contiguous view at any row offset: the kernel reads g_opac, g_scales and g_rgbs dword by
        # dword (4-byte alignment, which every float view has) and g_quats as float4, whose [N,4] row views stay 16-byte aligned
        ups = [None if g is None else g.contiguous().float() for g in (g_opac, g_scales, g_quats, g_rgbs)]
        if ups[2] is not None and ups[2].data_ptr() % 16:
            ups[2] = ups[2].clone()
        a.g_opacities, a.g_scales, a.g_quats, a.g_rgbs = (L.ptr(g) for g in ups)
        need = ctx.needs_input_grad                           # (means, quats, opacity_logits, log_scales, features_dc, features_rest, ...)
        out = [torch.empty_like(t) if need[k] else None for k, t in ((1, quats), (2, opacity_logits), (3, log_scales), (4, features_dc), (5, features_rest))]
        a.dL_dquats, a.dL_dopacity_logits, a.dL_dlog_scales, a.dL_dfeatures_dc = (L.ptr(t) for t in out[:4])
        a.dL_dfeatures_rest = L.ptr(out[4]) if M > 1 else None
        L.launch("emd_vanilla_backward", C.byref(a))
        return (None, *out, None, None, None)


def vanilla_gaussians(means, quats, opacity_logits, log_scales, features_dc, features_rest, camera_center, sh_degree=3, step=0,
                      sh_degree_interval=1000, check_finite=True):
    """-> dict(_means, _opacities [N,1], _rgbs, _scales, _quats) of a class without a transform.  `_means` is `means` itself.  sh_degree > 0: the
    SH colour of degree n = min(step // sh_degree_interval, sh_degree) on the detached directions means - camera_center, + 0.5, clamped to [0, 1];
    sh_degree == 0: sigmoid(features_dc).  camera_center [3] stays on the device.  With check_finite off the call makes no host synchronisation
    and can be captured into a graph.  The upstream gradients may be views at any row offset (a torch.cat of this dictionary behind other rows)."""
    L.need_device("vanilla_gaussians", means)
    if log_scales.dim() != 2 or log_scales.shape[1] != 3:
        raise NotImplementedError("ball gaussians ([N,1] scales) are not served")
    n = min(step // sh_degree_interval, sh_degree)
    if features_rest.dim() != 3 or (n + 1) ** 2 > features_rest.shape[1] + 1:
        raise ValueError("features_rest holds fewer than (degree + 1)^2 - 1 rows")
    def f(t):
        t = t.contiguous().float()
        return t if t.data_ptr() % 16 == 0 else t.clone()          # (a contiguous slice can start off a 16-byte boundary)
    opac, scales, quats_out, rgbs = _VanillaGaussians.apply(f(means.detach()), f(quats), f(opacity_logits), f(log_scales), f(features_dc),
                                                             f(features_rest), f(camera_center.detach().reshape(3)), n, 1 if sh_degree > 0 else 0)
    gs = dict(_means=means, _opacities=opac, _rgbs=rgbs, _scales=scales, _quats=quats_out)
    if check_finite:
        _check_finite(gs, step)
    return gs
