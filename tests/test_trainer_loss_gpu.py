"""-m gpu: the image tail of an OmniRe step on the device (emd_amd.trainer_loss, csrc/trainer_loss.hip) against the fp64 restatement of
tests/trainer_loss_ref.py under its criterion: the seven scalars and all three gradients on every case, the affine colour correction, bit
reproducibility (eager, a side stream, hipGraph replay), an upstream scalar other than 1, skipped terms, that every gradient element is written,
and the chain composite_add -> apply_affine -> trainer_losses.

The shapes (tests/trainer_loss_ref.py CASES) and what each is for:
  11x11       a single SSIM output per channel; one partly filled chunk
  12x13       the smallest odd W: rows of 39 floats, off 16-byte alignment; every depth option runs here
  tiles       43 x 53: the SSIM map is 33 rows x 129 floats, one above whole 32 x 32 tiles both ways; three chunks of 1024 pixels
  wide        70 x 531: many tiles and chunks
  empty_hits  no lidar return: the depth term is 0 with a zero gradient
  edges       the kinks themselves, term by term"""
import ctypes as C

import pytest
import torch

from emd_amd import _lib as L
from emd_amd import trainer_loss as TL
from tests import trainer_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _leaves(inputs):
    c = {k: v.to(DEV) for k, v in inputs.items()}
    for k in ("x", "o", "d"):
        c[k] = c[k].clone().requires_grad_(True)
    return c


def _call(c, cfg):
    loss, terms = TL.trainer_losses(c["x"], c["y"], c["o"], c["s"], c["d"], c["l"], **cfg)
    assert loss.dim() == 0 and loss.requires_grad and set(terms) == set(R.TERMS) and not any(t.requires_grad for t in terms.values())
    return loss, torch.stack([terms[n] for n in R.TERMS])


def _run(inputs, cfg, leaves=None):
    c = leaves or _leaves(inputs)
    for k in ("x", "o", "d"):
        c[k].grad = None
    loss, terms = _call(c, cfg)
    (R.UPSTREAM * loss + 1).backward()                                  # an upstream scalar other than 1
    return dict(loss=loss.detach(), terms=terms, g_rgb=c["x"].grad, g_opacity=c["o"].grad, g_depth=c["d"].grad)


def _check(name, cfg, what):
    R.criterion(_run(R.case(name), cfg), R.reference(name, cfg, DEV), cfg, f"{name} {what}")


@pytest.mark.parametrize("mask_type", ["bce", "safe_bce"])
@pytest.mark.parametrize("name", R.SMOOTH_CASES)
def test_losses_and_all_gradients_match_the_fp64_reference(name, mask_type):
    _check(name, R.config(mask_type=mask_type), mask_type)
    _check(name, R.config(mask_type=mask_type, w_ssim=0.0), mask_type + " without SSIM")       # the colour gradient under the element-wise rule


@pytest.mark.parametrize("term", list(R.ONLY))
def test_edges_term_by_term(term):
    _check("edges", R.only(term), term + " alone")


@pytest.mark.parametrize("opt", R.DEPTH_OPTIONS, ids=lambda o: f"{o['depth_type']}-n{int(o['normalize'])}-i{int(o['inverse'])}")
def test_every_depth_option(opt):
    _check("12x13", R.config(**opt), "depth option")


def test_empty_hit_set_gives_zero_and_a_zero_depth_gradient():
    c = _leaves(R.case("empty_hits"))
    cfg = R.only("depth")
    got = _run(None, cfg, leaves=c)
    assert float(got["loss"]) == 0.0 and float(got["terms"].abs().max()) == 0.0
    assert got["g_depth"] is not None and float(got["g_depth"].abs().max()) == 0.0


def test_accepted_shapes_are_views():
    c = R.case("12x13")
    cfg = R.config()
    flat = _run(c, cfg)
    shaped = dict(x=c["x"][None], y=c["y"][None], o=c["o"][..., None], s=c["s"][None, ..., None].bool(), d=c["d"][None], l=c["l"][..., None])
    got = _run(shaped, cfg)
    assert got["g_rgb"].shape == (1, 12, 13, 3) and got["g_opacity"].shape == (12, 13, 1) and got["g_depth"].shape == (1, 12, 13)
    assert torch.equal(got["loss"], flat["loss"]) and torch.equal(got["terms"], flat["terms"])
    for k in ("g_rgb", "g_opacity", "g_depth"):
        assert torch.equal(got[k].reshape(flat[k].shape), flat[k])


def test_skipped_terms_leave_their_gradients_zero_or_absent():
    c = R.case("12x13")
    got = _run(c, R.config(w_mask=0.0, w_entropy=0.0, w_depth=0.0, w_smooth=0.0))
    assert got["g_opacity"] is None and got["g_depth"] is None and got["g_rgb"] is not None
    assert [float(got["terms"][i]) for i in (2, 3, 4, 5)] == [0.0] * 4 and float(got["terms"][0]) > 0 and float(got["terms"][1]) > 0
    R.criterion(got, R.reference("12x13", R.config(w_mask=0.0, w_entropy=0.0, w_depth=0.0, w_smooth=0.0), DEV), R.config(), "weights 0")
    # absent inputs: the mask term without a sky mask, the depth term without lidar
    l = _leaves(c)
    loss, terms = TL.trainer_losses(l["x"], l["y"], l["o"], None, l["d"], None, **R.config(w_entropy=0.0, w_smooth=0.0))
    loss.backward()
    assert float(terms["mask_loss"]) == 0.0 and float(terms["depth_loss"]) == 0.0 and l["o"].grad is None and l["d"].grad is None
    # no colour term at all: the colour gradient is written, as zeros
    l = _leaves(c)
    loss, terms = TL.trainer_losses(l["x"], l["y"], l["o"], l["s"], **R.config(w_rgb=0.0, w_ssim=0.0))
    loss.backward()
    assert float(l["x"].grad.abs().max()) == 0.0 and float(l["o"].grad.abs().max()) > 0.0


def _flat(res):
    return [res["loss"].reshape(1), res["terms"], res["g_rgb"], res["g_opacity"], res["g_depth"]]


@pytest.mark.parametrize("name", ["12x13", "tiles"])
def test_bit_reproducible_across_runs_streams_and_graph_replay(name):
    cfg = R.config(mask_type="safe_bce")
    c = _leaves(R.case(name))
    first = [t.clone() for t in _flat(_run(None, cfg, leaves=c))]
    second = [t.clone() for t in _flat(_run(None, cfg, leaves=c))]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = [t.clone() for t in _flat(_run(None, cfg, leaves=c))]
    torch.cuda.current_stream().wait_stream(side)
    side.synchronize()
    for i, (a, b, d) in enumerate(zip(first, second, third)):
        assert torch.equal(a, b) and torch.equal(a, d), i

    A = (torch.eye(3, 4) + 0.05).to(DEV).requires_grad_(True)

    def step():
        loss, terms = _call(dict(c, x=TL.apply_affine(c["x"], A)), cfg)
        grads = torch.autograd.grad(R.UPSTREAM * loss + 1, [c["x"], c["o"], c["d"], A])
        return [loss.detach().reshape(1), terms] + list(grads)
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for replay in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(eager, captured)):
            assert torch.equal(a, b), (replay, i)


@pytest.mark.parametrize("name", ["11x11", "12x13", "tiles", "edges"])
def test_every_gradient_element_is_written_and_nothing_beside_it(name):
    """The C entry point on NaN-filled gradient buffers with guard bands: no NaN survives inside, nothing outside is touched."""
    c = {k: v.to(DEV).contiguous() for k, v in R.case(name).items()}
    H, W = c["d"].shape
    guard = 64
    bufs = {k: torch.full((n + 2 * guard,), float("nan"), device=DEV) for k, n in (("rgb", 3 * H * W), ("o", H * W), ("d", H * W), ("losses", 7))}
    a = L.EmdTrainerLossArgs()
    a.height, a.width = H, W
    a.rgb, a.gt_rgb, a.opacity, a.sky_mask, a.depth, a.lidar_depth = (c[k].data_ptr() for k in "xyosdl")
    a.w_rgb, a.w_ssim, a.w_mask, a.safe_limit, a.w_depth, a.upper_bound, a.w_entropy, a.w_smooth = 0.8, 0.2, 0.05, 0.1, 0.1, 80.0, 0.03, 0.02
    a.losses, a.dL_drgb, a.dL_dopacity, a.dL_ddepth = (bufs[k].data_ptr() + 4 * guard for k in ("losses", "rgb", "o", "d"))
    lib = L.load()
    need = int(lib.emd_trainer_loss_workspace_size(C.byref(a)))
    ws = torch.full((need // 4 + 2 * guard,), float("nan"), device=DEV)
    L.check(lib.emd_trainer_loss(C.byref(a), ws.data_ptr() + 4 * guard, need, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "emd_trainer_loss")
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool(torch.isfinite(t[guard:-guard]).all()), k
        assert bool(torch.isnan(t[:guard]).all()) and bool(torch.isnan(t[-guard:]).all()), k
    assert bool(torch.isnan(ws[:guard]).all()) and bool(torch.isnan(ws[guard + need // 4:]).all())


# ---- the affine colour correction ------------------------------------------------------------------------

def _affine(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.eye(3, 4) + 0.1 * torch.randn(3, 4, generator=g)


def _elementwise(got, ref, what):
    got, ref = got.double().cpu(), ref.double().cpu()
    err, tol = (got - ref).abs(), 1e-4 * ref.abs() + 1e-6 * ref.abs().max()
    print(f"{what} {tuple(ref.shape)}: worst element {float((err / tol).max()):.3f} of its tolerance")
    assert bool((err <= tol).all()), what


@pytest.mark.parametrize("name", list(R.CASES))
def test_affine_forward_and_both_gradients_match_fp64(name):
    c = R.case(name)
    g_out = torch.randn(c["x"].shape, generator=torch.Generator().manual_seed(11))
    x, A = c["x"].to(DEV).requires_grad_(True), _affine(7).to(DEV).requires_grad_(True)
    out = TL.apply_affine(x, A)
    out.backward(g_out.to(DEV))
    x64, A64 = c["x"].double().requires_grad_(True), _affine(7).double().requires_grad_(True)
    ref = x64 @ A64[:, :3].T + A64[:, 3]
    ref.backward(g_out.double())
    assert out.shape == x.shape and x.grad.shape == x.shape and A.grad.shape == (3, 4)
    _elementwise(out.detach(), ref.detach(), name + " affine forward")
    _elementwise(x.grad, x64.grad, name + " affine dL/drgb")
    _elementwise(A.grad, A64.grad, name + " affine dL/dA")


def test_identity_affine_reproduces_the_input_bit_for_bit():
    x = R.case("wide")["x"].to(DEV)
    assert torch.equal(TL.apply_affine(x, torch.eye(3, 4, device=DEV)), x)
    assert torch.equal(TL.apply_affine(x[None], torch.eye(3, 4, device=DEV)), x[None])


def test_affine_gradients_are_bit_reproducible_and_only_what_is_needed_is_formed():
    c = R.case("tiles")
    g_out = torch.randn(c["x"].shape, generator=torch.Generator().manual_seed(12)).to(DEV)
    runs = []
    for _ in range(2):
        x, A = c["x"].to(DEV).requires_grad_(True), _affine(8).to(DEV).requires_grad_(True)
        TL.apply_affine(x, A).backward(g_out)
        runs.append((x.grad, A.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    x, A = c["x"].to(DEV), _affine(8).to(DEV).requires_grad_(True)                          # a leaf image: dL/dA alone
    TL.apply_affine(x, A).backward(g_out)
    assert torch.equal(A.grad, runs[0][1])


# ---- the chain -------------------------------------------------------------------------------------------

def test_chain_composite_affine_losses_backward_against_fp64_torch():
    """composite_add -> apply_affine -> trainer_losses -> backward at 43 x 75 against the same chain in fp64 torch, the sky colour taken from the
    op's own output.  Everything upstream of the corrected image receives the SSIM gradient, so dL/drgb_gaussians, dL/dopacity and dL/dA are
    held to the SSIM rule (1e-4 of the largest entry); dL/ddepth to the element-wise rule; the scalars to 1e-6."""
    from emd_amd.sky import EnvLight, composite_add
    H, W = 43, 75
    g = torch.Generator().manual_seed(21)
    base = R.make_inputs(H, W, seed=22)
    dirs = torch.nn.functional.normalize(torch.randn(H, W, 3, generator=g), dim=-1)
    env = EnvLight(resolution=8, device=DEV)
    env.base.data = (0.2 + 0.6 * torch.rand(6, 8, 8, 3, generator=g)).to(DEV)
    rgb_g = (0.6 * torch.rand(H, W, 3, generator=g) * base["o"][..., None])
    A0 = _affine(9)
    cfg = R.config(mask_type="safe_bce", w_depth=0.1, depth_type="smooth_l1")
    lv = dict(rgb=rgb_g.to(DEV).requires_grad_(True), o=base["o"][..., None].to(DEV).requires_grad_(True), d=base["d"].to(DEV).requires_grad_(True),
              A=A0.to(DEV).requires_grad_(True))

    def device_chain(y):
        rgb, sky = composite_add(env, {"viewdirs": dirs.to(DEV)}, lv["rgb"], lv["o"])
        corrected = TL.apply_affine(rgb, lv["A"])
        if y is None:
            return corrected.detach(), sky.detach()
        loss, terms = TL.trainer_losses(corrected, y, lv["o"], base["s"].to(DEV), lv["d"], base["l"].to(DEV), **cfg)
        return loss, torch.stack([terms[n] for n in R.TERMS])
    corrected, sky = device_chain(None)
    # the ground truth at least 2e-3 from the op's own corrected image: no |x - y| sits at its kink
    sign = 1 - 2 * (torch.rand(H, W, 3, generator=g) < 0.5).float()
    y = corrected + ((0.002 + 0.2 * torch.rand(H, W, 3, generator=g)) * sign).to(DEV)
    loss, terms = device_chain(y)
    (R.UPSTREAM * loss + 1).backward()

    r = dict(rgb=rgb_g.double().to(DEV).requires_grad_(True), o=base["o"][..., None].double().to(DEV).requires_grad_(True),
             d=base["d"].double().to(DEV).requires_grad_(True), A=A0.double().to(DEV).requires_grad_(True))
    rgb64 = r["rgb"] + sky.double() * (1 - r["o"])
    cor64 = rgb64 @ r["A"][:, :3].T + r["A"][:, 3]
    assert float((cor64.detach() - corrected.double()).abs().max()) < 1e-5
    rloss, rterms = R.losses(cor64, y.double(), r["o"][..., 0], base["s"].double().to(DEV), r["d"], base["l"].double().to(DEV), cfg)
    (R.UPSTREAM * rloss + 1).backward()
    for k, a, b in [("loss", loss.detach(), rloss.detach())] + [(n, terms[i], rterms[i].detach()) for i, n in enumerate(R.TERMS)]:
        print(f"chain {k}: got {float(a):.9e} ref {float(b):.9e} |err| {abs(float(a) - float(b)):.3e}")
        assert abs(float(a) - float(b)) <= 1e-6, k
    for k in ("rgb", "o", "A"):
        err, top = float((lv[k].grad.double() - r[k].grad).abs().max()), float(r[k].grad.abs().max())
        print(f"chain dL/d{k}: worst error {err:.3e}, tolerance {1e-4 * top:.3e}")
        assert err <= 1e-4 * top, k
    _elementwise(lv["d"].grad, r["d"].grad, "chain dL/ddepth")
