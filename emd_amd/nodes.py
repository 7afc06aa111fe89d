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
`emd_vanilla_backward`, csrc/vanilla.hip), with `features_dc` and `features_rest` read where they are (no `torch.cat`)."""
import ctypes as C

import torch

from . import _lib as L
from .gsplat_api import spherical_harmonics
from .motion import transform_gaussians


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
    `instances_embedding` behind the encoder input; the layers of ConditionalDeformNetwork run on rocBLAS and are not covered)."""
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
        L.check(L.load().emd_vanilla_forward(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "emd_vanilla_forward")
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
        L.check(L.load().emd_vanilla_backward(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "emd_vanilla_backward")
        return (None, *out, None, None, None)


def vanilla_gaussians(means, quats, opacity_logits, log_scales, features_dc, features_rest, camera_center, sh_degree=3, step=0,
                      sh_degree_interval=1000, check_finite=True):
    """-> dict(_means, _opacities [N,1], _rgbs, _scales, _quats) of a class without a transform.  `_means` is `means` itself.  sh_degree > 0: the
    SH colour of degree n = min(step // sh_degree_interval, sh_degree) on the detached directions means - camera_center, + 0.5, clamped to [0, 1];
    sh_degree == 0: sigmoid(features_dc).  camera_center [3] stays on the device.  With check_finite off the call makes no host synchronisation
    and can be captured into a graph.  The upstream gradients may be views at any row offset (a torch.cat of this dictionary behind other rows)."""
    if means.device.type != "cuda":
        raise L.EmdError("vanilla_gaussians needs tensors on a ROCm device; there is no CPU path")
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
