"""`VanillaGaussians` -- OmniRe's per-class Gaussian store and its density control on the HIP path (the
OmniRe anchor; section 8a row a17).

Mirrors, with the reference's attribute / method names and argument meaning (behaviour restated, not copied):
  parameter layout `_means _scales _quats _opacities _features_dc [N,3] _features_rest [N,K-1,3]`, activations,
  `get_gaussian_param_groups` (class-prefixed group names)            OmniRe/models/gaussians/vanilla.py:29-158,193-204
  `after_train` (running |grad| sums, visibility counts, max screen size)    :163-191
  `postprocess_per_train_step`                                            :150-161
  `refinement_after` = split_gaussians + dup_gaussians + cull_gaussians + opacity reset, and the optimiser surgery
  `dup_in_optim` / `remove_from_optim`                                  :206-376, models/gaussians/basics.py:198-242

WHERE the work runs differs.  The reference grows every parameter and both Adam moments with boolean-mask indexing, `repeat` and `torch.cat`
three times per event (split, duplicate, cull: ~90 launches, a host sync per mask, and the Adam state touched three times); here one event is
`emd_refine_decide` -> prefix sums -> `emd_refine_index` -> ONE `emd_densify_gather` over the six parameters and their twelve moments
(csrc/densify.hip), with a single host read (the new point count).  The reference's semantics that the fused decision reproduces are spelled out
at `EmdRefineArgs` in include/emd_raster.h -- the ones that are easy to get wrong: a split ORIGINAL stays (scale reduced in place), the
duplicate test runs AFTER that reduction (a Gaussian just above the size threshold is split AND duplicated), the cull sees the grown arrays with
`max_2Dsize` 0 on the new rows, and the output order is originals, samples replica 0, replica 1, duplicates.  The split samples are a Philox
draw keyed by (seed, event, source index, replica): every rank of a view-parallel job draws the same samples (`samples=` takes a recorded draw
instead: tests).  There is no CPU path.

The render path and the regularisers of the class (csrc/vanilla.hip):
  `get_gaussians(cam)` (:378-414) is `nodes.vanilla_gaussians`: one launch each way for the activations and the SH colour
  `compute_reg_loss()` is `gaussian_regulation`: sharp-shape, flatten, sparse and max-s-square in two launches forward, one backward.  The trainer
  assigns `cur_radii` per class from `info["radii"]`; where the reference reads `(cur_radii > 0).sum()` on the host and drops `sparse_reg` when
  nothing is visible, the key stays here with value 0 and a zero gradient, and there is no sync.
Not covered: `create_from_pcd` from a point cloud (the caller supplies kNN scales: `create_from_tensors`), the state-dict loaders, ball
Gaussians (`[N,1]` scales: NotImplementedError)."""
import ctypes as C

import torch
from torch.nn import Parameter

from . import _lib as L
from .density import EventRows, restructure_rows

SH_C0 = 0.28209479177387814


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


class _GaussianReg(torch.autograd.Function):
    """One autograd node: `emd_vanilla_reg_forward` (two launches) and `emd_vanilla_reg_backward` (one)."""

    @staticmethod
    def forward(ctx, log_scales, opacity_logits, radii, weights):
        dev, n = log_scales.device, log_scales.shape[0]
        a = L.EmdVanillaRegArgs()
        a.num_points = n
        a.log_scales, a.opacity_logits, a.radii = log_scales.data_ptr(), L.ptr(opacity_logits), L.ptr(radii)
        a.w_sharp, a.max_gauss_ratio, a.w_flatten, a.w_sparse, a.w_max_s_square = weights
        terms = torch.empty(4, device=dev, dtype=torch.float32)
        ws = torch.empty(max(int(L.load().emd_vanilla_reg_workspace_size(n)), 8), device=dev, dtype=torch.uint8)
        a.terms = terms.data_ptr()
        L.launch("emd_vanilla_reg_forward", C.byref(a), ws.data_ptr(), ws.numel())
        ctx.save_for_backward(log_scales, opacity_logits, radii, ws)
        ctx.weights = weights
        return terms

    @staticmethod
    def backward(ctx, g):
        log_scales, opacity_logits, radii, ws = ctx.saved_tensors
        a = L.EmdVanillaRegArgs()
        a.num_points = log_scales.shape[0]
        a.log_scales, a.opacity_logits, a.radii = log_scales.data_ptr(), L.ptr(opacity_logits), L.ptr(radii)
        a.w_sharp, a.max_gauss_ratio, a.w_flatten, a.w_sparse, a.w_max_s_square = ctx.weights
        g = g.contiguous().float()
        d_ls = torch.empty_like(log_scales)
        sparse = ctx.weights[3] != 0.0 and opacity_logits is not None and radii is not None
        d_lo = torch.empty_like(opacity_logits) if (sparse and ctx.needs_input_grad[1]) else None
        a.g, a.dL_dlog_scales, a.dL_dopacity_logits = g.data_ptr(), d_ls.data_ptr(), L.ptr(d_lo)
        L.launch("emd_vanilla_reg_backward", C.byref(a), ws.data_ptr(), ws.numel())
        return d_ls, d_lo, None, None


def gaussian_regulation(log_scales, opacity_logits=None, radii=None, *, w_sharp=0., max_gauss_ratio=10., w_flatten=0., w_sparse=0., w_max_s_square=0.):
    """The regularisers of VanillaGaussians.compute_reg_loss over `log_scales` [N,3], `opacity_logits` [N] or [N,1] and the rasterizer's `radii` [N]
    (> 0: visible) -> terms [4] = sharp_shape, flatten, sparse, max_s_square, each weighted, a differentiable output of one node (the formulas:
    EmdVanillaRegArgs, include/emd_raster.h).  A term whose weight is 0 is skipped (value 0, no gradient), the sparse term also without
    `opacity_logits` or `radii`; `opacity_logits` receives no gradient when there is no sparse term.  The weights are Python numbers.
    Bit-reproducible, forward and backward; no host synchronisation."""
    L.need_device("gaussian_regulation", log_scales)
    if log_scales.dim() != 2 or log_scales.shape[1] != 3:
        raise NotImplementedError("ball gaussians ([N,1] scales) are not served")
    lo = None if opacity_logits is None else opacity_logits.contiguous().float()
    r = None if radii is None else radii.detach().reshape(-1).to(torch.int32).contiguous()
    n = log_scales.shape[0]
    if (lo is not None and lo.numel() != n) or (r is not None and r.numel() != n):
        raise ValueError("opacity_logits / radii do not have one entry per Gaussian")
    weights = (float(w_sharp), float(max_gauss_ratio), float(w_flatten), float(w_sparse), float(w_max_s_square))
    return _GaussianReg.apply(log_scales.contiguous().float(), lo, r, weights)


class VanillaGaussians(torch.nn.Module):
    def __init__(self, class_name, ctrl, reg=None, networks=None, scene_scale=30.0, scene_origin=None, num_train_images=300, device="cuda",
                 refine_seed=0, **kwargs):
        super().__init__()
        self.class_prefix = class_name + "#"
        self.ctrl_cfg, self.reg_cfg, self.networks_cfg = ctrl, reg, networks
        self.scene_scale = scene_scale
        self.scene_origin = torch.zeros(3) if scene_origin is None else scene_origin
        self.num_train_images = num_train_images
        self.step = 0
        self.device = torch.device(device)
        self.in_test_set = False
        self.xys_grad_norm = self.vis_counts = self.max_2Dsize = None
        self.filter_mask = None
        self.cur_radii = None                # this class's rows of info["radii"], assigned by the trainer: the visible set of the sparse regulariser
        self.ball_gaussians = bool(_get(ctrl, "ball_gaussians", False))
        self.refine_seed, self.refine_events = int(refine_seed), 0
        z = lambda *s: torch.zeros(*s, device=self.device)
        self._means, self._scales, self._quats, self._opacities = z(1, 3), z(1, 3), z(1, 4), z(1, 1)
        self._features_dc, self._features_rest = z(1, 3), z(1, (self.sh_degree + 1) ** 2 - 1, 3)

    sh_degree = property(lambda self: _get(self.ctrl_cfg, "sh_degree", 3))
    num_points = property(lambda self: self._means.shape[0])
    get_scaling = property(lambda self: torch.exp(self._scales))
    get_opacity = property(lambda self: torch.sigmoid(self._opacities))
    get_quats = property(lambda self: self.quat_act(self._quats))
    shs_0 = property(lambda self: self._features_dc)
    shs_rest = property(lambda self: self._features_rest)

    @property
    def colors(self):
        return self._features_dc * SH_C0 + 0.5 if self.sh_degree > 0 else torch.sigmoid(self._features_dc)

    def quat_act(self, x):
        return x / x.norm(dim=-1, keepdim=True)

    def create_from_tensors(self, means, colors, log_scales, quats=None):
        """create_from_pcd (vanilla.py:78-106) with the kNN-derived initial log-scales and the random unit quaternions supplied by the caller
        (the reference takes them from sklearn and the global RNG): SH dc = RGB2SH(colors), opacity logit(0.1)."""
        dev, n = self.device, means.shape[0]
        P = lambda t: Parameter(t.to(dev).float().contiguous())
        self._means = P(means)
        self._scales = P(log_scales.reshape(n, -1).expand(n, 3))
        if quats is None:
            quats = torch.zeros(n, 4)
            quats[:, 0] = 1.0
        self._quats = P(quats)
        self._features_dc = P((colors.float() - 0.5) / SH_C0 if self.sh_degree > 0 else torch.logit(colors.float(), eps=1e-10))
        self._features_rest = P(torch.zeros(n, (self.sh_degree + 1) ** 2 - 1, 3))
        self._opacities = P(torch.logit(0.1 * torch.ones(n, 1)))

    def preprocess_per_train_step(self, step):
        self.step = step

    def postprocess_per_train_step(self, step, optimizer, radii, xys_grad, last_size):
        self.after_train(radii, xys_grad, last_size)
        if step % _get(self.ctrl_cfg, "refine_interval") == 0:
            self.refinement_after(step, optimizer)

    def get_gaussian_param_groups(self):
        p = self.class_prefix
        return {p + "xyz": [self._means], p + "sh_dc": [self._features_dc], p + "sh_rest": [self._features_rest], p + "opacity": [self._opacities],
                p + "scaling": [self._scales], p + "rotation": [self._quats]}

    get_param_groups = get_gaussian_param_groups

    # ---- the render path and the regularisers (csrc/vanilla.hip) ----------------------------------------------------------------------------
    def get_gaussians(self, cam, check_finite=None):
        """vanilla.py:378-414: the dictionary `collect_gaussians` concatenates over classes.  `cam.camtoworlds` [..., 4, 4] stays on the device.
        check_finite (default: ctrl key `check_finite`, else True) is the finite check of the node functions, one host sync; with it off the call
        makes no host synchronisation and can be captured into a graph."""
        from .nodes import vanilla_gaussians
        if self.ball_gaussians or self._scales.shape[-1] != 3:
            raise NotImplementedError("ball gaussians ([N,1] scales) are not served")
        self.filter_mask = torch.ones(self.num_points, dtype=torch.bool, device=self._means.device)
        return vanilla_gaussians(self._means, self._quats, self._opacities, self._scales, self._features_dc, self._features_rest,
                                 cam.camtoworlds[..., :3, 3], sh_degree=self.sh_degree, step=self.step,
                                 sh_degree_interval=_get(self.ctrl_cfg, "sh_degree_interval", 1000),
                                 check_finite=bool(_get(self.ctrl_cfg, "check_finite", True)) if check_finite is None else check_finite)

    def compute_reg_loss(self):
        """The reference's dict: `sharp_shape_reg` (when reg_cfg names it and step % step_interval == 0), `flatten`, `sparse_reg` (when reg_cfg names
        it and `cur_radii` is set), `max_s_square` (reg_cfg key `max_s_square_reg`).  Every value is an element of ONE node's output, so the
        trainer's sum over the dict back-propagates through that node once.  Nothing visible: `sparse_reg` stays, with value 0 (no host read)."""
        cfg = self.reg_cfg
        if not cfg:
            return {}
        if self.ball_gaussians or self._scales.shape[-1] != 3:
            raise NotImplementedError("ball gaussians ([N,1] scales) are not served")
        keys, w = {}, dict(w_sharp=0., max_gauss_ratio=10., w_flatten=0., w_sparse=0., w_max_s_square=0.)
        sharp = _get(cfg, "sharp_shape_reg")
        if sharp is not None and self.step % int(_get(sharp, "step_interval", 1)) == 0:
            w["w_sharp"], w["max_gauss_ratio"], keys["sharp_shape_reg"] = float(_get(sharp, "w")), float(_get(sharp, "max_gauss_ratio", 10.)), 0
        flatten = _get(cfg, "flatten")
        if flatten is not None:
            w["w_flatten"], keys["flatten"] = float(_get(flatten, "w")), 1
        sparse = _get(cfg, "sparse_reg")
        if sparse and self.cur_radii is not None:
            w["w_sparse"], keys["sparse_reg"] = float(_get(sparse, "w")), 2
        msq = _get(cfg, "max_s_square_reg")
        if msq is None:
            msq = _get(cfg, "max_s_square")
        if msq is not None:
            w["w_max_s_square"], keys["max_s_square"] = float(_get(msq, "w")), 3
        if not keys:
            return {}
        terms = gaussian_regulation(self._scales, self._opacities if "sparse_reg" in keys else None,
                                    self.cur_radii if "sparse_reg" in keys else None, **w)
        return {k: terms[i] for k, i in keys.items()}

    # ---- a17: the running statistics of the refinement --------------------------------------------------------------------------------------
    def after_train(self, radii, xys_grad, last_size):
        """vanilla.py:163-191 on this class's rows of the rasterizer's outputs: `radii` [n] int, `xys_grad` [n,2] (means2d.grad or .absgrad, already
        scaled to pixels by the trainer, base.py:279-286).  The first call after a refinement starts the sums the way the reference does: the
        norm of EVERY row (visible or not) and a count of ONE everywhere (:175-178); later calls are one launch (no mask indexing, no sync)."""
        with torch.no_grad():
            n = self.num_points
            if self.filter_mask is not None and not bool(self.filter_mask.all()):
                raise NotImplementedError("a partial filter_mask (rows hidden from the rasterizer) is not used by the reference's VanillaGaussians")
            L.need_device("VanillaGaussians.after_train", radii, xys_grad)
            r = radii.reshape(-1).to(torch.int32).contiguous()
            g = xys_grad.reshape(n, -1).float()
            if g.stride(1) != 1:
                g = g.contiguous()
            assert r.numel() == n and g.shape[1] >= 2
            first = self.xys_grad_norm is None
            if first:
                self.xys_grad_norm = g[:, :2].norm(dim=-1) if g.shape[1] > 2 else g.norm(dim=-1)
                self.vis_counts = torch.ones_like(self.xys_grad_norm)
            if self.max_2Dsize is None:
                self.max_2Dsize = torch.zeros(n, device=r.device, dtype=torch.float32)
            L.launch("emd_after_train_stats", n, r.data_ptr(), g.data_ptr(), int(g.stride(0)), None if first else self.xys_grad_norm.data_ptr(),
                     None if first else self.vis_counts.data_ptr(), self.max_2Dsize.data_ptr(), float(last_size))

    # ---- the refinement event ------------------------------------------------------------------------------------------------------------
    def refinement_after(self, step, optimizer, samples=None):
        """vanilla.py:206-297.  `samples` [n_split_samples, n_split, 3]: standard normals to use instead of the Philox draw (tests: the reference's
        recorded `torch.randn((samps * n_splits, 3))`, viewed that way).  Returns {"n_before", "n_after", "split" (sources), "originals_kept",
        "samples_kept", "dups_kept"} (None when the event does nothing: before `warmup_steps`, or inside the guard behind an opacity reset)."""
        assert step == self.step
        c = self.ctrl_cfg
        if self.step <= _get(c, "warmup_steps"):
            return None
        info = None
        with torch.no_grad():
            reset_interval = _get(c, "reset_alpha_interval")
            past_reset = self.step % reset_interval > max(self.num_train_images, _get(c, "refine_interval"))
            do_densification = self.step < _get(c, "stop_split_at") and past_reset
            if do_densification:
                assert self.xys_grad_norm is not None and self.vis_counts is not None and self.max_2Dsize is not None
            if do_densification or past_reset:
                info = self._refine(optimizer, do_densification, past_reset, samples)
            if self.step % reset_interval == _get(c, "refine_interval"):
                # opacity reset (vanilla.py:286-297): logit(min(sigmoid(o), reset_alpha_value)), Adam moments of the opacity group restart at zero
                value = torch.min(self.get_opacity.data, torch.ones_like(self._opacities.data) * _get(c, "reset_alpha_value"))
                self._opacities.data = torch.logit(value)
                for group in optimizer.param_groups:
                    if group["name"] == self.class_prefix + "opacity":
                        st = optimizer.state[group["params"][0]]
                        st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(st["exp_avg"]), torch.zeros_like(st["exp_avg_sq"])
            self.xys_grad_norm = self.vis_counts = self.max_2Dsize = None
        return info

    def _refine(self, optimizer, do_densify, do_cull, samples):
        """The event's body, once for every class: args -> the rows that travel (`density.EventRows`) -> the driver -> install.  A class states what
        differs in `_refine_args`, `_refine_attrs`, `_refine_rows` and `_after_refine`."""
        L.need_device(f"{type(self).__name__}.refinement_after", self._means)
        N, prefix = self.num_points, self.class_prefix
        a, keep = self._refine_args(do_densify, do_cull)
        groups = {grp["name"]: grp for grp in (optimizer.param_groups if optimizer is not None else [])}
        rows = EventRows(optimizer)
        for short, (attr, role) in self._refine_attrs().items():
            rows.add_param(attr, getattr(self, attr), role, groups.get(prefix + short))
        outs, (n_keep, n_dup, n_samp, n_split), layout = self._refine_rows(a, keep, rows.jobs, N, samples)
        info = {"n_before": N, "n_after": n_keep + n_samp + n_dup, "split": n_split, "originals_kept": n_keep, "samples_kept": n_samp, "dups_kept": n_dup}
        if outs is None:
            return info                                             # nothing split, duplicated or culled: every tensor stays as it is
        for attr, param in rows.install(outs).items():
            setattr(self, attr, param)
        self._after_refine(layout)
        if do_densify:
            self.refine_events += 1
        return info

    def _refine_args(self, do_densify, do_cull, a=None):
        """-> (the decision inputs on `a`, default a new EmdRefineArgs; the tensors its pointers need alive, the contiguous log-scales first)"""
        c = self.ctrl_cfg
        a = L.EmdRefineArgs() if a is None else a
        a.num_points, a.do_densify, a.do_cull = self.num_points, int(do_densify), int(do_cull)
        screen_on = self.step < _get(c, "stop_screen_size_at")
        a.use_split_screen, a.cull_big, a.use_cull_screen = int(screen_on), int(self.step > _get(c, "reset_alpha_interval")), int(screen_on)
        keep = [self._scales.detach().contiguous(), self._opacities.detach().reshape(-1).contiguous()]
        a.scaling, a.opacity = keep[0].data_ptr(), keep[1].data_ptr()
        if self.max_2Dsize is not None:
            keep.append(self.max_2Dsize.reshape(-1).float().contiguous())
            a.max_2Dsize = keep[-1].data_ptr()
        if do_densify:
            keep += [self.xys_grad_norm.reshape(-1).float().contiguous(), self.vis_counts.reshape(-1).float().contiguous()]
            a.grad_norm, a.vis_counts = keep[-2].data_ptr(), keep[-1].data_ptr()
        # the host's products, rounded to float once (the reference compares float tensors with Python scalars)
        a.grad_threshold, a.size_threshold = float(_get(c, "densify_grad_thresh")), float(_get(c, "densify_size_thresh") * self.scene_scale)
        a.split_screen, a.cull_alpha = float(_get(c, "split_screen_size")), float(_get(c, "cull_alpha_thresh"))
        a.cull_size, a.cull_screen = float(_get(c, "cull_scale_thresh") * self.scene_scale), float(_get(c, "cull_screen_size"))
        return a, keep

    def _refine_attrs(self):
        """optimiser group (after the class prefix) -> (attribute, role) of every per-point parameter, in the order they travel"""
        return {"xyz": ("_means", L.DENSIFY_ROLE_XYZ), "sh_dc": ("_features_dc", L.DENSIFY_ROLE_COPY), "sh_rest": ("_features_rest", L.DENSIFY_ROLE_COPY),
                "opacity": ("_opacities", L.DENSIFY_ROLE_COPY), "scaling": ("_scales", L.DENSIFY_ROLE_SCALING), "rotation": ("_quats", L.DENSIFY_ROLE_COPY)}

    def _refine_rows(self, a, keep, jobs, N, samples):
        """The driver call -> (outs or None, (originals kept, duplicates kept, samples kept, split sources), what `_after_refine` takes)"""
        ns = int(_get(self.ctrl_cfg, "n_split_samples", 2))
        seed = self.refine_seed * 0x9E3779B97F4A7C15 + self.refine_events
        outs, (n_keep, n_dup, n_samp, n_split) = restructure_rows(L.DENSIFY_MODE_REFINE, a, jobs, N, seed=seed, samples=samples, scaling=keep[0],
                                                                  rotation=self._quats.detach().contiguous(), num_samples=ns)
        return outs, (n_keep, n_dup, ns * n_samp, n_split), None

    def _after_refine(self, layout):
        """Rows moved and the new parameters are installed: what else describes the point set (nothing here)."""
