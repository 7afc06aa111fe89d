"""-m gpu: the per-class dictionary and the regularisers of VanillaGaussians on the device (emd_amd.nodes.vanilla_gaussians,
emd_amd.vanilla.gaussian_regulation, csrc/vanilla.hip) against the fp64 restatement of tests/vanilla_ref.py under the criterion of DESIGN.md
section 5 (relative 1e-5 on the loss terms): values and every gradient, the bits of the existing ops, the +0 rows, the tie rules and the clip of
the sparse term, bit-reproducibility (eager, a side stream, hipGraph replay), that every output element is written and nothing beside it, skipped
terms and absent upstream gradients, and the class methods.

The shapes (tests/vanilla_ref.py) and what each is for:
  dictionary   every (active degree, coefficient rows) of sh_ref.SH_DEG_ROWS -- the degree uses all rows of a record (dwordx4 loads) or the first
               few (dword loads, +0 rows behind them) -- and dc mode; N = 1, 255, 256, 257 (the seams of a 256-lane block and of its two
               128-record halves' last float4), 1000 (four blocks)
  regularisers N one below, at and one above EMD_VANILLA_REG_CHUNK, three chunks and a part, and 300 000: more chunks (293) than the finalize
               workgroup has lanes (256); ties: equal columns in every position; edges: logits inside and outside the clip, nothing / one row visible"""
import ctypes as C
import types

import pytest
import torch

from emd_amd import _lib as L
from emd_amd import nodes, vanilla
from emd_amd.gsplat_api import spherical_harmonics
from tests import vanilla_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEAVES = ("quats", "opacity_logits", "log_scales", "features_dc", "features_rest")
UPS = dict(_opacities="g_opacities", _scales="g_scales", _quats="g_quats", _rgbs="g_rgbs")
IDS = lambda c: "-".join(map(str, c))


def _leaves(c):
    return {k: c[k].to(DEV).requires_grad_(True) for k in LEAVES}


def _consts(c):
    """The tensors without a gradient on the device: the means, the camera centre, the upstream gradients."""
    return {k: c[k].to(DEV) for k in ("means", "camera_center") + tuple(UPS.values())}


def _run(c, leaves=None, used=R.OUTPUTS, check_finite=True, consts=None):
    """-> the dictionary and {d_<leaf>: gradient} of L = sum over `used` of (output * upstream)."""
    leaves, k = leaves or _leaves(c), consts or _consts(c)
    gs = nodes.vanilla_gaussians(k["means"], leaves["quats"], leaves["opacity_logits"], leaves["log_scales"], leaves["features_dc"],
                                 leaves["features_rest"], k["camera_center"], sh_degree=c["sh_degree"], step=c["step"],
                                 sh_degree_interval=R.INTERVAL, check_finite=check_finite)
    assert gs["_means"] is k["means"] and set(gs) == {"_means", "_opacities", "_rgbs", "_scales", "_quats"}
    loss = sum((gs[o] * k[UPS[o]]).sum() for o in used)
    grads = torch.autograd.grad(loss, [leaves[n] for n in LEAVES], allow_unused=True)
    # detached: a result that kept its grad_fn would keep this call's autograd graph alive, and with it the leaves' AccumulateGrad nodes, bound to
    # the stream of THIS call; a later capture on another stream would then have to wait on that stream (the default one: not capturable)
    return {o: v.detach() for o, v in gs.items()}, {"d_" + n: g for n, g in zip(LEAVES, grads)}


# ---- the dictionary --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DICT_CASES, ids=IDS)
def test_dictionary_and_all_five_gradients_match_the_fp64_reference(case):
    c, ref = R.dict_case(*case), R.dict_reference(*case)
    leaves = _leaves(c)
    gs, grads = _run(c, leaves)
    N, K = c["N"], c["K"]
    assert gs["_opacities"].shape == (N, 1)
    for k in R.OUTPUTS:
        R.compare(gs[k], ref[k], f"{case} {k}")
    for k in R.GRADS:
        assert grads[k] is not None and grads[k].shape == ref[k].shape, k
        assert bool(torch.isfinite(grads[k]).all())
        R.compare(grads[k], ref[k], f"{case} {k}")
    unused = grads["d_features_rest"][:, K - 1:] if c["sh_mode"] else grads["d_features_rest"]
    assert not bool((unused != 0).any()) and not bool(torch.signbit(unused).any())          # exactly +0

    # the bits of the existing ops
    ls, rq, lo = leaves["log_scales"].detach(), leaves["quats"].detach(), leaves["opacity_logits"].detach()
    s, q, o = torch.empty_like(ls), torch.empty_like(rq), torch.empty_like(lo)
    L.check(L.load().emd_activations_forward(N, ls.data_ptr(), s.data_ptr(), rq.data_ptr(), q.data_ptr(), lo.data_ptr(), o.data_ptr(), L.stream()),
            "emd_activations_forward")
    assert torch.equal(gs["_scales"], s) and torch.equal(gs["_quats"], q) and torch.equal(gs["_opacities"], o)
    if c["sh_mode"]:
        coeffs = torch.cat((leaves["features_dc"].detach()[:, None, :], leaves["features_rest"].detach()), dim=1)
        want = torch.clamp(spherical_harmonics(c["n"], c["means"].to(DEV) - c["camera_center"].to(DEV), coeffs) + 0.5, 0.0, 1.0)
        assert torch.equal(gs["_rgbs"], want)


@pytest.mark.parametrize("case", [(3, 1000, 16, 257), (0, 0, 4, 257)], ids=IDS)
def test_an_output_nobody_uses_counts_as_a_zero_upstream_gradient(case):
    c, ref = R.dict_case(*case), R.dict_reference(*case)
    _, grads = _run(c, used=("_scales",))
    R.compare(grads["d_log_scales"], ref["d_log_scales"], f"{case} scales alone")
    for k in ("d_quats", "d_opacity_logits", "d_features_dc", "d_features_rest"):
        assert grads[k].shape == ref[k].shape and not bool((grads[k] != 0).any()), k
    _, grads = _run(c, used=("_rgbs", "_quats"))
    for k in ("d_features_dc", "d_features_rest", "d_quats"):
        R.compare(grads[k], ref[k], f"{case} colour and quaternions alone: {k}")
    assert not bool((grads["d_log_scales"] != 0).any()) and not bool((grads["d_opacity_logits"] != 0).any())


@pytest.mark.parametrize("case,ahead", [((3, 3000, 16, 257), 5), ((3, 2000, 16, 255), 1), ((0, 0, 4, 256), 3)], ids=lambda v: IDS(v) if isinstance(v, tuple) else str(v))
def test_gradients_arrive_through_a_concatenation_behind_other_rows(case, ahead):
    """The trainer's collect_gaussians: torch.cat of the classes' dictionaries.  The gradient of a later operand is a view of the whole gradient at
    a row offset; with `ahead` rows in front (no multiple of 4) those of [N,1] and [N,3] outputs start off a 16-byte boundary."""
    c, ref = R.dict_case(*case), R.dict_reference(*case)
    leaves, k = _leaves(c), _consts(c)
    _, direct = _run(c, leaves, consts=k)
    gs = nodes.vanilla_gaussians(k["means"], leaves["quats"], leaves["opacity_logits"], leaves["log_scales"], leaves["features_dc"],
                                 leaves["features_rest"], k["camera_center"], sh_degree=c["sh_degree"], step=c["step"], sh_degree_interval=R.INTERVAL)
    seen, loss = {}, 0.0
    for o in R.OUTPUTS:
        other = torch.ones(ahead, gs[o].shape[1], device=DEV, requires_grad=True)
        whole = torch.cat((other, gs[o]))
        gs[o].register_hook(lambda g, o=o: seen.__setitem__(o, (g.is_contiguous(), g.data_ptr() % 16)))
        loss = loss + (whole * torch.cat((torch.zeros_like(other), k[UPS[o]]))).sum()
    grads = torch.autograd.grad(loss, [leaves[n] for n in LEAVES])
    # what the test is about: the upstream gradients of the [N,1] and [N,3] outputs came in off a 16-byte boundary
    assert all(seen[o][0] for o in R.OUTPUTS) and all(seen[o][1] != 0 for o in ("_opacities", "_scales", "_rgbs")), seen
    for n, g in zip(LEAVES, grads):
        R.compare(g, ref["d_" + n], f"{case} behind {ahead} rows: d_{n}")
        assert torch.equal(g, direct["d_" + n]), n                                         # the same bits as with whole upstream tensors


def _flat(gs, grads):
    return [gs[k] for k in R.OUTPUTS] + [grads[k] for k in R.GRADS]


@pytest.mark.parametrize("case", [(3, 3000, 16, 1000), (3, 1000, 16, 257), (0, 0, 4, 255)], ids=IDS)
def test_dictionary_is_bit_reproducible_across_runs_streams_and_graph_replay(case):
    c = R.dict_case(*case)
    leaves, consts = _leaves(c), _consts(c)
    first = [t.clone() for t in _flat(*_run(c, leaves, consts=consts))]
    second = _flat(*_run(c, leaves, consts=consts))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = [t.clone() for t in _flat(*_run(c, leaves, consts=consts))]
    torch.cuda.current_stream().wait_stream(side)
    side.synchronize()
    for i, (a, b, d) in enumerate(zip(first, second, third)):
        assert torch.equal(a, b) and torch.equal(a, d), i
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _flat(*_run(c, leaves, check_finite=False, consts=consts))          # (the finite check reads the device: one sync)
    for replay in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(first, captured)):
            assert torch.equal(a, b), (replay, i)


GUARD = 64            # floats: 256 bytes, so every carved tensor stays 16-byte aligned


def _carve(sizes):
    """One NaN-filled buffer with a guard band in front of, between and behind tensors of `sizes` floats -> buffer, offsets."""
    offs, off = [], GUARD
    for n in sizes:
        offs.append(off)
        off += (n + 3) // 4 * 4 + GUARD
    return torch.full((off,), float("nan"), device=DEV), offs


def _guards_untouched(buf, offs, sizes):
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    for o, n in zip(offs, sizes):
        keep[o:o + n] = False
    return bool(torch.isnan(buf[keep]).all())


@pytest.mark.parametrize("case", [(3, 3000, 16, 257), (3, 1000, 16, 257), (2, 5000, 9, 1), (3, 0, 16, 255), (0, 0, 4, 256)], ids=IDS)
def test_every_output_element_is_written_and_nothing_beside_it(case):
    """The C entry points on NaN-filled buffers with guard bands: no NaN survives in an output, every guard stays NaN, the values are the node's."""
    c = R.dict_case(*case)
    N, M = c["N"], c["M"]
    gs, grads = _run(c)
    dev = {k: c[k].to(DEV) for k in ("means", "quats", "opacity_logits", "log_scales", "features_dc", "features_rest", "camera_center") + tuple(UPS.values())}
    out_sizes = [N, 3 * N, 4 * N, 3 * N]
    grad_sizes = [4 * N, N, 3 * N, 3 * N, 3 * (M - 1) * N]
    obuf, ooff = _carve(out_sizes)
    gbuf, goff = _carve(grad_sizes)
    mask = torch.full((N + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    a = L.EmdVanillaArgs()
    a.num_points, a.sh_coeffs, a.degree, a.sh_mode = N, M, c["n"], int(c["sh_mode"])
    a.means, a.log_scales, a.quats, a.opacity_logits = (dev[k].data_ptr() for k in ("means", "log_scales", "quats", "opacity_logits"))
    a.features_dc, a.features_rest, a.camera_center = dev["features_dc"].data_ptr(), (dev["features_rest"].data_ptr() if M > 1 else None), dev["camera_center"].data_ptr()
    a.opacities, a.scales, a.quats_out, a.rgbs = (obuf.data_ptr() + 4 * o for o in ooff)
    a.clamp_mask = mask.data_ptr() + GUARD
    a.g_opacities, a.g_scales, a.g_quats, a.g_rgbs = (dev[k].data_ptr() for k in ("g_opacities", "g_scales", "g_quats", "g_rgbs"))
    ptrs = [gbuf.data_ptr() + 4 * o for o in goff]
    a.dL_dquats, a.dL_dopacity_logits, a.dL_dlog_scales, a.dL_dfeatures_dc = ptrs[:4]
    a.dL_dfeatures_rest = ptrs[4] if M > 1 else None
    lib = L.load()
    L.check(lib.emd_vanilla_forward(C.byref(a), L.stream()), "emd_vanilla_forward")
    L.check(lib.emd_vanilla_backward(C.byref(a), L.stream()), "emd_vanilla_backward")
    torch.cuda.synchronize()
    assert _guards_untouched(obuf, ooff, out_sizes) and _guards_untouched(gbuf, goff, grad_sizes)
    assert bool((mask[:GUARD] == 0xAB).all()) and bool((mask[GUARD + N:] == 0xAB).all()) and bool((mask[GUARD:GUARD + N] <= 7).all())
    for k, o, n in zip(R.OUTPUTS, ooff, out_sizes):
        assert torch.equal(obuf[o:o + n], gs[k].reshape(-1)), k
    for k, o, n in zip(R.GRADS, goff, grad_sizes):
        assert torch.equal(gbuf[o:o + n], grads[k].reshape(-1)), k


# ---- the regularisers ------------------------------------------------------------------------------------------------------------------
def _reg_leaves(c):
    return c["log_scales"].to(DEV).requires_grad_(True), c["opacity_logits"].to(DEV).requires_grad_(True), c["radii"].to(DEV)


def _reg(c, w, leaves=None, upstream=R.UPSTREAM, use_logits=True, use_radii=True):
    l, a, r = leaves or _reg_leaves(c)
    terms = vanilla.gaussian_regulation(l, a if use_logits else None, r if use_radii else None, **w)
    assert terms.shape == (4,) and terms.requires_grad
    gl, ga = torch.autograd.grad((terms * torch.tensor(upstream, device=DEV)).sum(), (l, a), allow_unused=True)
    return dict(terms=terms.detach(), d_log_scales=gl, d_opacity_logits=ga)


@pytest.mark.parametrize("wname", list(R.WEIGHT_SETS))
@pytest.mark.parametrize("name", R.REG_CASES)
def test_terms_and_gradients_match_the_fp64_reference(name, wname):
    c, w, ref = R.reg_case(name), R.weights(wname), R.reg_reference(name, wname)
    got = _reg(c, w)
    R.scalar_criterion(got["terms"], ref["terms"], f"{name} {wname}")
    assert bool(torch.isfinite(got["d_log_scales"]).all())
    R.compare(got["d_log_scales"], ref["d_log_scales"], f"{name} {wname} d_log_scales")
    if w["w_sparse"] != 0:
        assert bool(torch.isfinite(got["d_opacity_logits"]).all())
        R.compare(got["d_opacity_logits"], ref["d_opacity_logits"], f"{name} {wname} d_opacity_logits")
    else:
        assert got["d_opacity_logits"] is None and float(ref["d_opacity_logits"].abs().max()) == 0.0      # absent without a sparse term
    if name == "edges_none":
        assert float(got["terms"][2]) == 0.0                                            # nothing visible: the term is 0, the key stays


def test_skipped_terms_are_zero_and_take_nothing_from_their_upstream_scalar():
    c, w = R.reg_case("ties"), R.weights("all")
    nan_up = (R.UPSTREAM[0], R.UPSTREAM[1], float("nan"), R.UPSTREAM[3])
    for kw in (dict(use_radii=False), dict(use_logits=False)):
        ref = R.regulation(c, w, **kw)
        got = _reg(c, w, upstream=nan_up, **kw)                                          # the sparse term is skipped: its NaN upstream reaches nothing
        assert float(got["terms"][2]) == 0.0 and got["d_opacity_logits"] is None
        R.scalar_criterion(got["terms"], ref["terms"], f"sparse skipped {kw}")
        R.compare(got["d_log_scales"], ref["d_log_scales"], f"sparse skipped {kw} d_log_scales")
    got = _reg(c, R.weights("sparse"), upstream=(float("nan"), float("nan"), 1.0, float("nan")))
    assert not bool((got["d_log_scales"] != 0).any()) and bool(torch.isfinite(got["d_opacity_logits"]).all())
    assert not bool((got["terms"][[0, 1, 3]] != 0).any())


@pytest.mark.parametrize("name", [f"n{3 * R.CHUNK + 17}", "n300000", "ties"])
def test_regularisers_are_bit_reproducible_across_runs_streams_and_graph_replay(name):
    c, w = R.reg_case(name), R.weights("all")
    leaves = _reg_leaves(c)
    flat = lambda d: [d["terms"], d["d_log_scales"], d["d_opacity_logits"]]
    first = [t.clone() for t in flat(_reg(c, w, leaves))]
    second = flat(_reg(c, w, leaves))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = [t.clone() for t in flat(_reg(c, w, leaves))]
    torch.cuda.current_stream().wait_stream(side)
    side.synchronize()
    for i, (a, b, d) in enumerate(zip(first, second, third)):
        assert torch.equal(a, b) and torch.equal(a, d), i
    up = torch.tensor(R.UPSTREAM, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        terms = vanilla.gaussian_regulation(leaves[0], leaves[1], leaves[2], **w)
        captured = [terms.detach()] + list(torch.autograd.grad((terms * up).sum(), leaves[:2]))
    for replay in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(first, captured)):
            assert torch.equal(a, b), (replay, i)


@pytest.mark.parametrize("name", [f"n{R.CHUNK - 1}", f"n{R.CHUNK + 1}", "edges_one"])
def test_regulariser_outputs_and_workspace_are_written_and_nothing_beside_them(name):
    """The C entry points: NaN-filled outputs and a workspace full of 0xFF bytes (it is never cleared) between guard bands."""
    c, w = R.reg_case(name), R.weights("all")
    N = c["N"]
    l, lo, r = (t.detach() for t in _reg_leaves(c))
    node = _reg(c, w)
    lib = L.load()
    nbytes = int(lib.emd_vanilla_reg_workspace_size(N))
    assert nbytes % 8 == 0 and nbytes > 0
    sizes = [4, 3 * N, N]
    buf, offs = _carve(sizes)
    ws = torch.full((nbytes + 512,), 0xFF, dtype=torch.uint8, device=DEV)
    up = torch.tensor(R.UPSTREAM, device=DEV)
    a = L.EmdVanillaRegArgs()
    a.num_points, a.log_scales, a.opacity_logits, a.radii = N, l.data_ptr(), lo.data_ptr(), r.data_ptr()
    a.w_sharp, a.max_gauss_ratio, a.w_flatten, a.w_sparse, a.w_max_s_square = w["w_sharp"], w["max_gauss_ratio"], w["w_flatten"], w["w_sparse"], w["w_max_s_square"]
    a.terms, a.dL_dlog_scales, a.dL_dopacity_logits = (buf.data_ptr() + 4 * o for o in offs)
    a.g = up.data_ptr()
    L.check(lib.emd_vanilla_reg_forward(C.byref(a), ws.data_ptr() + 256, nbytes, L.stream()), "emd_vanilla_reg_forward")
    L.check(lib.emd_vanilla_reg_backward(C.byref(a), ws.data_ptr() + 256, nbytes, L.stream()), "emd_vanilla_reg_backward")
    torch.cuda.synchronize()
    assert _guards_untouched(buf, offs, sizes)
    assert bool((ws[:256] == 0xFF).all()) and bool((ws[256 + nbytes:] == 0xFF).all())
    for k, o, n in zip(("terms", "d_log_scales", "d_opacity_logits"), offs, sizes):
        assert torch.equal(buf[o:o + n], node[k].reshape(-1)), k


# ---- the class -------------------------------------------------------------------------------------------------------------------------
def _model(step, step_interval):
    g = torch.Generator().manual_seed(31)
    N = 300
    ctrl = dict(sh_degree=3, sh_degree_interval=R.INTERVAL, refine_interval=100)
    reg = dict(sharp_shape_reg=dict(w=0.7, step_interval=step_interval, max_gauss_ratio=10.0), flatten=dict(w=0.3), sparse_reg=dict(w=0.05),
               max_s_square_reg=dict(w=1.3))
    node = vanilla.VanillaGaussians("Background", ctrl, reg=reg, device=DEV)
    node.create_from_tensors(0.5 * torch.randn(N, 3, generator=g), torch.rand(N, 3, generator=g), 0.9 * torch.randn(N, 1, generator=g) - 1.0)
    with torch.no_grad():                    # the first half keeps its three equal scales (the ties), the second half spreads them
        node._scales[N // 2:] += 0.9 * torch.randn(N - N // 2, 3, generator=g).to(DEV)
        node._features_rest.copy_(torch.randn(N, 15, 3, generator=g).to(DEV))
        node._quats.copy_(torch.randn(N, 4, generator=g).to(DEV))
        node._opacities.copy_(3.0 * torch.randn(N, 1, generator=g).to(DEV))
    node.preprocess_per_train_step(step)
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([4.0, -3.0, 3.5])
    return node, types.SimpleNamespace(camtoworlds=c2w.to(DEV)), g


@pytest.mark.parametrize("step,step_interval", [(0, 10), (1000, 10), (3000, 10), (1000, 7), (3000, 7)])
def test_class_methods_match_the_reference_functions(step, step_interval):
    node, cam, g = _model(step, step_interval)
    N = node.num_points
    cpu = lambda t: t.detach().cpu()
    case = dict(sh_mode=True, n=min(step // R.INTERVAL, 3), means=cpu(node._means), quats=cpu(node._quats), opacity_logits=cpu(node._opacities),
                log_scales=cpu(node._scales), features_dc=cpu(node._features_dc), features_rest=cpu(node._features_rest),
                camera_center=cpu(cam.camtoworlds[:3, 3]), g_opacities=torch.randn(N, 1, generator=g), g_scales=torch.randn(N, 3, generator=g),
                g_quats=torch.randn(N, 4, generator=g), g_rgbs=torch.randn(N, 3, generator=g))
    ref = R.dictionary(case)
    gs = node.get_gaussians(cam)
    assert gs["_means"] is node._means
    assert node.filter_mask.dtype == torch.bool and node.filter_mask.shape == (N,) and bool(node.filter_mask.all())
    for k in R.OUTPUTS:
        R.compare(gs[k], ref[k], f"step {step} {k}")
    sum((gs[k] * case[UPS[k]].to(DEV)).sum() for k in R.OUTPUTS).backward()
    for k, p in (("d_quats", node._quats), ("d_opacity_logits", node._opacities), ("d_log_scales", node._scales), ("d_features_dc", node._features_dc),
                 ("d_features_rest", node._features_rest)):
        R.compare(p.grad, ref[k], f"step {step} {k}")
        p.grad = None
    assert node._means.grad is None
    # after_train accepts the all-ones filter_mask
    radii = (torch.randint(1, 40, (N,), generator=g) * (torch.rand(N, generator=g) < 0.6)).to(torch.int32)
    node.after_train(radii.to(DEV), torch.randn(N, 2, generator=g).to(DEV), 800.0)
    assert node.xys_grad_norm.shape == (N,)

    # compute_reg_loss: the reference's keys, each an element of one node's output
    sharp_on = step % step_interval == 0
    w = dict(w_sharp=0.7 if sharp_on else 0.0, max_gauss_ratio=10.0, w_flatten=0.3, w_sparse=0.05, w_max_s_square=1.3)
    rc = dict(log_scales=cpu(node._scales), opacity_logits=cpu(node._opacities), radii=radii)
    assert node.cur_radii is None
    losses = node.compute_reg_loss()
    assert list(losses) == (["sharp_shape_reg"] if sharp_on else []) + ["flatten", "max_s_square"]       # no radii yet: no sparse_reg
    node.cur_radii = radii.to(DEV)
    losses = node.compute_reg_loss()
    assert list(losses) == (["sharp_shape_reg"] if sharp_on else []) + ["flatten", "sparse_reg", "max_s_square"]
    one = (1.0, 1.0, 1.0, 1.0)
    ref = R.regulation(rc, w, upstream=one)
    got = torch.stack([losses.get(k, torch.zeros((), device=DEV)) for k in ("sharp_shape_reg", "flatten", "sparse_reg", "max_s_square")])
    R.scalar_criterion(got, ref["terms"], f"step {step} / {step_interval} compute_reg_loss")
    sum(losses.values()).backward()
    R.compare(node._scales.grad, ref["d_log_scales"], f"step {step} / {step_interval} d_log_scales")
    R.compare(node._opacities.grad, ref["d_opacity_logits"], f"step {step} / {step_interval} d_opacity_logits")
    # nothing visible: the key stays, the value is 0
    node.cur_radii = torch.zeros(N, dtype=torch.int32, device=DEV)
    assert float(node.compute_reg_loss()["sparse_reg"].detach()) == 0.0


@pytest.mark.parametrize("how", ["keyword", "ctrl"])
def test_get_gaussians_without_the_finite_check_makes_no_sync_and_is_captured(how):
    """The finite check reads the device (a capture refuses that); the keyword and the ctrl key `check_finite` both switch it off."""
    node, cam, _ = _model(3000, 10)
    with torch.no_grad():
        eager = node.get_gaussians(cam)
    kw = {}
    if how == "keyword":
        kw["check_finite"] = False
    else:
        node.ctrl_cfg["check_finite"] = False
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        captured = node.get_gaussians(cam, **kw)
    for k in R.OUTPUTS:
        captured[k].fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for k in R.OUTPUTS:
        assert torch.equal(captured[k], eager[k]), k
