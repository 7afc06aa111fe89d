"""The image tail of an OmniRe training step on the HIP path (csrc/trainer_loss.hip).

`apply_affine(rgb, affine)` = the per-image affine colour correction of models/trainers/base.py:251-258 with ONE [3,4] matrix per image;
`trainer_losses(...)` = the image losses of compute_losses (base.py:518-620): L1, pytorch_msssim's unpadded SSIM, the occupancy BCE / safe-BCE,
the lidar depth loss, the opacity entropy and kornia's inverse-depth smoothness, with dL/drgb, dL/dopacity and dL/ddepth, in at most five launches.
The formulas are in include/emd_raster.h (EmdTrainerLossArgs).  Everything is channels-last as the trainer's `outputs` dict; no float atomics:
losses and gradients are bit-identical from run to run.  No CPU path."""
import ctypes as C

import torch

from . import _lib as L

LOSS_NAMES = ("rgb_loss", "ssim_loss", "mask_loss", "depth_loss", "opacity_entropy_loss", "inverse_depth_smoothness_loss")
_MASK_TYPES = {"bce": L.TL_MASK_BCE, "safe_bce": L.TL_MASK_SAFE_BCE}
_DEPTH_TYPES = {"l1": L.TL_DEPTH_L1, "l2": L.TL_DEPTH_L2, "smooth_l1": L.TL_DEPTH_SMOOTH_L1}


class _Affine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, affine):
        x = rgb.detach().contiguous().float()
        A = affine.detach().contiguous().float()
        out = torch.empty_like(x)
        L.launch("emd_affine_forward", x.numel() // 3, x.data_ptr(), A.data_ptr(), out.data_ptr())
        ctx.save_for_backward(x, A)
        return out.view(rgb.shape)

    @staticmethod
    def backward(ctx, g):
        x, A = ctx.saved_tensors
        g = g.contiguous().float()
        P = x.numel() // 3
        need_x, need_A = ctx.needs_input_grad
        d_x = torch.empty_like(x) if need_x else None
        d_A = torch.empty(3, 4, device=x.device, dtype=torch.float32) if need_A else None
        # the chunks' partial sums of dL/dA: caller-owned, never cleared (a captured step takes it from the graph's pool)
        ws = torch.empty(max(int(L.load().emd_affine_workspace_size(P)), 8), device=x.device, dtype=torch.uint8) if need_A else None
        L.launch("emd_affine_backward", P, x.data_ptr(), A.data_ptr(), g.data_ptr(), L.ptr(d_x), L.ptr(d_A), L.ptr(ws),
                 0 if ws is None else ws.numel())
        return d_x, d_A


def apply_affine(rgb, affine, pixel_affine=False):
    """rgb [...,3] -> affine[:, :3] @ rgb + affine[:, 3] per pixel, `affine` the [3,4] matrix of the image (the decoder's output for ONE embedding
    row, `img_idx.flatten()[:1]`: see INTEGRATION.md).  Gradients reach both.  A per-pixel [H,W,3,4] matrix is not served."""
    if pixel_affine or affine.dim() != 2:
        raise NotImplementedError("apply_affine takes one [3,4] matrix per image; per-pixel affine (pixel_affine=True, a [H,W,3,4] input) is not built")
    L.need_device("apply_affine", rgb, affine)
    if tuple(affine.shape) != (3, 4) or rgb.dim() < 1 or rgb.shape[-1] != 3 or rgb.numel() == 0:
        raise L.EmdError(f"apply_affine: rgb {tuple(rgb.shape)} / affine {tuple(affine.shape)}, expected [...,3] and [3,4]")
    return _Affine.apply(rgb, affine)


class _TrainerLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, gt_rgb, opacity, sky_mask, depth, lidar_depth, H, W, cfg):
        dev = rgb.device
        f = lambda t: None if t is None else t.detach().contiguous().float()
        x, y, o, s, d, l = f(rgb), f(gt_rgb), f(opacity), f(sky_mask), f(depth), f(lidar_depth)
        a = L.EmdTrainerLossArgs()
        a.height, a.width = H, W
        a.mask_type, a.depth_type, a.normalize, a.inverse = cfg["mask_type"], cfg["depth_type"], cfg["normalize"], cfg["inverse"]
        a.rgb, a.gt_rgb, a.opacity, a.sky_mask, a.depth, a.lidar_depth = x.data_ptr(), y.data_ptr(), L.ptr(o), L.ptr(s), L.ptr(d), L.ptr(l)
        for k in ("w_rgb", "w_ssim", "w_mask", "safe_limit", "w_depth", "upper_bound", "w_entropy", "w_smooth"):
            setattr(a, k, cfg[k])
        losses = torch.empty(7, device=dev, dtype=torch.float32)
        a.losses = losses.data_ptr()
        need = ctx.needs_input_grad
        # a gradient is formed only where a term reaches the input; elsewhere autograd gets None
        on_o = o is not None and ((cfg["w_mask"] != 0.0 and s is not None) or cfg["w_entropy"] != 0.0)
        on_d = d is not None and ((cfg["w_depth"] != 0.0 and l is not None and s is not None) or cfg["w_smooth"] != 0.0)
        g_x = torch.empty_like(x) if need[0] else None
        g_o = torch.empty_like(o) if (need[2] and on_o) else None
        g_d = torch.empty_like(d) if (need[4] and on_d) else None
        a.dL_drgb, a.dL_dopacity, a.dL_ddepth = L.ptr(g_x), L.ptr(g_o), L.ptr(g_d)
        # partial sums and the SSIM derivative maps: caller-owned, never cleared (a captured step takes it from the graph's pool)
        ws = torch.empty(max(int(L.load().emd_trainer_loss_workspace_size(C.byref(a))), 8), device=dev, dtype=torch.uint8)
        L.launch("emd_trainer_loss", C.byref(a), ws.data_ptr(), ws.numel())
        ctx.save_for_backward(g_x, g_o, g_d)
        ctx.shapes = (rgb.shape, None if opacity is None else opacity.shape, None if depth is None else depth.shape)
        ctx.mark_non_differentiable(losses)
        return losses[0].clone(), losses

    @staticmethod
    def backward(ctx, g, _g_terms):
        g_x, g_o, g_d = ctx.saved_tensors
        s = ctx.shapes
        have = [t for t in (g_x, g_o, g_d) if t is not None]
        # the gradients were formed by the forward's launches; the upstream scalar scales them in one multi-tensor launch
        scaled = iter(torch._foreach_mul(have, g) if len(have) > 1 else [t * g for t in have])
        pick = lambda t, shape: None if t is None else next(scaled).view(shape)
        return (pick(g_x, s[0]), None, pick(g_o, s[1]), None, pick(g_d, s[2]), None, None, None, None)


def _image_size(rgb):
    shape = tuple(rgb.shape)
    if len(shape) == 4 and shape[0] == 1:
        shape = shape[1:]
    if len(shape) != 3 or shape[2] != 3:
        raise L.EmdError(f"trainer_losses: rgb is {tuple(rgb.shape)}, expected [H,W,3] or [1,H,W,3]")
    return shape[0], shape[1]


def trainer_losses(rgb, gt_rgb, opacity=None, sky_mask=None, depth=None, lidar_depth=None, *, w_rgb=0.8, w_ssim=0.2, w_mask=0.05, mask_type="bce",
                   safe_limit=0.1, w_depth=0.0, depth_type="l1", normalize=False, inverse=False, upper_bound=80.0, w_entropy=0.0, w_smooth=0.0,
                   depth_error_percentile=None):
    """-> (loss, {"rgb_loss", "ssim_loss", "mask_loss", "depth_loss", "opacity_entropy_loss", "inverse_depth_smoothness_loss"}), each term
    weighted, the loss their sum.  rgb, gt_rgb [H,W,3]; opacity, sky_mask (0 / 1, any dtype), depth, lidar_depth [H,W], [H,W,1] or with a leading
    1.  A term whose weight is 0 or whose input is None is skipped.  The weights are Python numbers: a decay schedule folds into w_depth.
    Gradients reach rgb, opacity and depth."""
    if depth_error_percentile is not None:
        raise NotImplementedError("trainer_losses: depth_error_percentile is not built (the depth loss runs over every hit pixel)")
    if mask_type not in _MASK_TYPES or depth_type not in _DEPTH_TYPES:
        raise L.EmdError(f"trainer_losses: mask_type {mask_type!r} / depth_type {depth_type!r}, expected one of {list(_MASK_TYPES)} / {list(_DEPTH_TYPES)}")
    L.need_device("trainer_losses", rgb, gt_rgb, opacity, sky_mask, depth, lidar_depth)
    H, W = _image_size(rgb)
    if gt_rgb.numel() != 3 * H * W:
        raise L.EmdError(f"trainer_losses: gt_rgb is {tuple(gt_rgb.shape)}, rgb {tuple(rgb.shape)}")
    for name, t in (("opacity", opacity), ("sky_mask", sky_mask), ("depth", depth), ("lidar_depth", lidar_depth)):
        if t is not None and (t.numel() != H * W or tuple(t.shape) not in ((H, W), (H, W, 1), (1, H, W), (1, H, W, 1))):
            raise L.EmdError(f"trainer_losses: {name} is {tuple(t.shape)}, expected [{H},{W}], [{H},{W},1] or either with a leading 1")
    cfg = dict(mask_type=_MASK_TYPES[mask_type], depth_type=_DEPTH_TYPES[depth_type], normalize=int(bool(normalize)), inverse=int(bool(inverse)),
               w_rgb=float(w_rgb), w_ssim=float(w_ssim), w_mask=float(w_mask), safe_limit=float(safe_limit), w_depth=float(w_depth),
               upper_bound=float(upper_bound), w_entropy=float(w_entropy), w_smooth=float(w_smooth))
    total, terms = _TrainerLoss.apply(rgb, gt_rgb, opacity, sky_mask, depth, lidar_depth, H, W, cfg)
    return total, {n: terms[1 + i] for i, n in enumerate(LOSS_NAMES)}
