"""-m gpu: emd_image_loss (csrc/loss.hip) called by name through ctypes against tests/loss_ref.py, the float64 restatement of the reference's loss
tail (pinned by tests/test_loss_ref_cpu.py), at the shapes its structure suggests -- smaller than the 11-tap window, on the seams of the 32 x 32
tile and of the four rows a thread owns, on both sides of the 256-pixel point-wise block, with more blocks than the 64 atomic slots -- and with
pixels placed exactly ON every gate (loss_ref.DEPTH_ROWS / WEIGHT_ROWS, image == gt).

Allowances: loss_ref.allowance(family, output) = 4 x the float32 floor of the reference's own formulation, never more than test_loss_gpu.py's
1e-4 of the largest entry / 1e-5 relative; the total, which the kernel forms from the four terms, is held to what their allowances add up to
(loss_ref.total_allowance); where the reference's value is exact (+0, or sign / (3 H W)) the comparison is by bit pattern.

Every buffer handed to the call, input or output, is followed by a guard of 4 096 bytes of 0xFF, outputs and the workspace -- exactly
emd_image_loss_workspace(H, W) bytes -- are pre-filled with 0xFF (as a float: a NaN that no arithmetic produces): each call checks that inputs and
guards are unchanged, that every element of a requested output was written and that an output passed as NULL was not touched."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 4096
UNWRITTEN = -1                     # 0xFFFFFFFF as int32
WORST = {}                         # output -> worst error as a share of its allowance, over the parity tests (printed at the end of the module)


def _lib():
    from emd_amd import _lib as L
    return L, L.load()


class Buffers:
    def __init__(self):
        self.items = []

    def put(self, array):
        raw = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).ravel().copy()).to(DEV)
        t = torch.full((raw.numel() + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        t[:raw.numel()] = raw
        self.items.append((t, raw.numel(), raw))
        return t

    def out(self, nbytes):
        t = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.items.append((t, nbytes, None))
        return t

    def check(self):
        torch.cuda.synchronize()
        for t, nbytes, content in self.items:
            assert bool((t[nbytes:] == 0xFF).all()), "the call wrote behind a buffer"
            assert content is None or torch.equal(t[:nbytes], content), "the call changed an input"


def _words(t, n):
    return t[:4 * n].view(torch.int32).cpu().numpy()


def call(case, want=(True, True, True), use_depth=True, use_sky=True, stream=None, workspace=None, short=0, edit=None, **lam):
    """One emd_image_loss call on guarded buffers -> (return code, dict of float32: the five terms and the requested gradients).  `edit(args)`
    changes the arguments last; `short` bytes are held back from the workspace size handed over."""
    L, lib = _lib()
    H, W = case["H"], case["W"]
    lam = {**R.LAMBDAS, **lam}
    b = Buffers()
    a = L.EmdLossArgs()
    a.height, a.width = H, W
    a.image, a.gt = b.put(case["image"]).data_ptr(), b.put(case["gt"]).data_ptr()
    if use_depth:
        a.depth, a.gt_depth = b.put(case["depth"]).data_ptr(), b.put(case["gt_depth"]).data_ptr()
        if case["mask"] is not None:
            a.mask = b.put(case["mask"]).data_ptr()
    if use_sky:
        a.weight, a.sky_mask = b.put(case["weight"]).data_ptr(), b.put(case["sky_mask"]).data_ptr()
    a.lambda_dssim, a.lambda_depth, a.lambda_sky, a.max_depth = lam["lambda_dssim"], lam["lambda_depth"], lam["lambda_sky"], case["max_depth"]
    losses = b.out(20)
    a.losses = losses.data_ptr()
    sizes = {"g_image": 3 * H * W, "g_depth": H * W, "g_weight": H * W}
    outs = {k: b.out(4 * n) for k, n in sizes.items()}
    for (k, t), wanted, field in zip(outs.items(), want, ("dL_dimage", "dL_ddepth", "dL_dweight")):
        if wanted:
            setattr(a, field, t.data_ptr())
    nbytes = lib.emd_image_loss_workspace(H, W)
    assert nbytes >= 4 * 9 * H * W
    ws = workspace if workspace is not None else b.out(nbytes)
    if workspace is not None:
        b.items.append((ws, nbytes, None))
    ws_ptr, args = ws.data_ptr(), C.byref(a)
    if edit is not None:
        args, ws_ptr = edit(a, args, ws_ptr)
    rc = lib.emd_image_loss(args, ws_ptr, nbytes - short, C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream))
    b.check()
    got = {"rc": rc, "workspace": ws}
    words = _words(losses, 5)
    if rc != L.EMD_OK:
        assert (words == UNWRITTEN).all() and all((_words(t, sizes[k]) == UNWRITTEN).all() for k, t in outs.items()), "a refused call wrote an output"
        return got
    assert (words != UNWRITTEN).all(), "a loss term was not written"
    got.update(zip(R.LOSSES, words.view(np.float32).tolist()))
    for (k, t), wanted in zip(outs.items(), want):
        words = _words(t, sizes[k])
        if wanted:
            assert (words != UNWRITTEN).all(), f"{k}: {(words == UNWRITTEN).sum()} of {words.size} elements were not written"
            got[k] = words.view(np.float32).reshape((3, H, W) if k == "g_image" else (H, W))
        else:
            assert (words == UNWRITTEN).all(), f"{k} was passed as NULL and was written"
    return got


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def compare(got, ref, family, tag, record=False):
    """Terms and the gradients that were requested against the reference at the family's allowance (every figure is printed before it is judged)."""
    bad = []
    judged = {k: (e, R.allowance(family, k)) for k, e in R.errors({k: got.get(k, ref[k]) for k in R.TERMS + R.GRADS}, ref).items() if k in got}
    judged["total"] = (R.total_error(got, ref), R.total_allowance(family, ref))
    for k, (e, allow) in judged.items():
        print(f"{tag} {family} {k}: error {e:.3g}, allowance {allow:.3g}")
        if record:
            WORST[k] = max(WORST.get(k, 0.0), e / allow)
        if not e <= allow:
            bad.append((k, e, allow))
    assert not bad, (tag, family, bad)


def check_placed(case, got, ref, lam):
    """On the gates: +0 by bit pattern where the reference's gradient is 0; elsewhere not 0 and, element by element, within 1e-6 relative (the
    point-wise gradients are products and quotients of at most eight float32 roundings of 2^-24 each, on operands placed clear of cancellation)."""
    if not case["placed"]:
        return
    for key, rows in (("g_depth", [r[0] for r in R.DEPTH_ROWS]), ("g_weight", [r[0] for r in R.WEIGHT_ROWS])):
        if key not in got:
            continue
        for name in rows:
            for at in case["placed"][name]:
                g, r = got[key].flat[at], ref[key].flat[at]
                if r == 0:
                    assert bits(g) == 0, (key, name, g)
                else:
                    assert g != 0 and abs(g / r - 1) <= 1e-6, (key, name, g, r)


def check_l1_gradient_exact(case, got):
    """lambda_dssim == 0: dL/dimage is sign(image - gt) / (3 H W), the one quotient the reference forms, bit for bit; +0 where image == gt."""
    n = np.float32(1) / np.float32(3 * case["H"] * case["W"])
    want = (np.sign(case["image"] - case["gt"]) * n).astype(np.float32) + np.float32(0)          # (-0 + 0 = +0)
    np.testing.assert_array_equal(bits(got["g_image"]), bits(want))
    for at in case["placed"].get("image == gt", []):
        assert (bits(got["g_image"]).reshape(3, -1)[:, at] == 0).all()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst error as a share of its allowance:", ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))


# ---- parity --------------------------------------------------------------------------------------------------------------------------------------
OTHERS = ("equal", "blocks", "pixel", "wide")
PARITY = [(group, shape, OTHERS[i % 4] if group != "slots" else "pixel") for group, shapes in R.SHAPES.items() for i, shape in enumerate(shapes)]


@pytest.mark.parametrize("group,shape,other", PARITY, ids=[f"{s[0]}x{s[1]}-{o}" for _g, s, o in PARITY])
def test_parity_with_the_float64_reference(group, shape, other):
    """The shape with the random family and with one of the other four (each group of shapes sees as many of them as it has shapes); the mask
    kinds (none, binary, {0, 0.5, 1, 2}) and sky counts (none, one, many) in turn, as loss_ref.family_cases deals them."""
    for family in ("random", other):
        cases = R.family_cases(family, [shape])
        if group == "slots":
            cases = cases[-1:]                                  # the single pixel in the last corner only: a reference takes 1.5 s at this size
        for n, case in enumerate(cases):
            tag = f"{shape[0]}x{shape[1]}#{n}"
            ref = R.reference(case, **R.LAMBDAS)
            got = call(case)
            assert got["rc"] == 0
            compare(got, ref, family, tag, record=True)
            check_placed(case, got, ref, R.LAMBDAS)
            if group != "slots":                                # and without the SSIM term: the L1 gradient alone, exact
                ref0 = R.reference(case, **{**R.LAMBDAS, "lambda_dssim": 0.0})
                got0 = call(case, lambda_dssim=0.0)
                assert got0["ssim"] == 0.0
                compare(got0, ref0, family, tag + " no ssim", record=True)
                check_placed(case, got0, ref0, R.LAMBDAS)
                check_l1_gradient_exact(case, got0)


def test_every_placed_row_under_every_mask_kind():
    for mask in ("none", "binary", "float"):
        case = R.build_case(33, 31, "random", seed=5, mask=mask)
        assert len(case["placed"]) == len(R.DEPTH_ROWS) + len(R.WEIGHT_ROWS) + 1
        ref, got = R.reference(case), call(case)
        compare(got, ref, "random", f"mask {mask}")
        check_placed(case, got, ref, R.LAMBDAS)
        assert np.array_equal(got["g_depth"] != 0, ref["g_depth"] != 0) and np.array_equal(got["g_weight"] != 0, ref["g_weight"] != 0)
        assert not (bits(got["g_depth"]) == np.int32(-2 ** 31)).any() and not (bits(got["g_weight"]) == np.int32(-2 ** 31)).any()      # no -0


# ---- subsets of the requested gradients ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lambda_dssim", [0.0, 0.2])
@pytest.mark.parametrize("sky", ["none", "one", "many"])
def test_requested_gradient_subsets(sky, lambda_dssim):
    """All 8 choices of dL_dimage / dL_ddepth / dL_dweight: each requested gradient is the reference's (all +0 where the reference applies no
    term) and bit for bit the one of the call that requests all three; nothing else moves (checked by call())."""
    case = R.build_case(33, 31, "random", seed=1, sky=sky)
    lam = {**R.LAMBDAS, "lambda_dssim": lambda_dssim}
    ref = R.reference(case, **lam)
    full = call(case, **lam)
    compare(full, ref, "random", f"all three, sky {sky}")
    assert (case["sky_mask"].sum() == 0) == (not ref["g_weight"].any())
    for want in [(i, d, w) for i in (False, True) for d in (False, True) for w in (False, True)]:
        got = call(case, want=want, **lam)
        assert got["rc"] == 0
        compare(got, ref, "random", f"{want}, sky {sky}")
        for k in R.GRADS:
            if k in got:
                assert np.array_equal(bits(got[k]), bits(full[k])), (want, k, "differs from the call that requests all three")
        if want[2] and sky == "none":
            assert not bits(got["g_weight"]).any(), (want, "dL_dweight without a sky pixel")


# ---- terms that are switched off -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lambda_dssim", [0.0, 0.2])
@pytest.mark.parametrize("off", ["lambda_sky 0", "lambda_sky -0.05", "lambda_depth 0", "no valid depth", "no depth input", "no weight input"])
def test_a_term_that_is_off_is_zero_and_its_gradient_is_written_as_zero(off, lambda_dssim):
    case = R.build_case(37, 43, "random", seed=2)
    lam = {**R.LAMBDAS, "lambda_dssim": lambda_dssim}
    kw = {}
    if off.startswith("lambda"):
        name, value = off.split()
        lam[name] = float(value)
    elif off == "no valid depth":                               # no return, the two ends of the gate themselves, and beyond the far end
        case["gt_depth"] = np.resize(np.array([0.0, R.DEPTH_LO, 80.0, 95.0], np.float32), case["gt_depth"].shape)
        case["mask"] = None
    else:
        kw = {"use_depth": False} if "depth" in off else {"use_sky": False}
    ref = R.reference(case, **lam, **kw)
    term, grad = ("depth", "g_depth") if "depth" in off else ("sky", "g_weight")
    assert ref[term] == 0 and not ref[grad].any()
    for want in ((True, True, True), (False, True, True), (False, "depth" in off, "depth" not in off)):
        got = call(case, want=want, **lam, **kw)
        assert got["rc"] == 0
        assert bits(got[term]) == 0, (off, want, term, got[term])
        assert not bits(got[grad]).any(), (off, want, grad, "is not +0 everywhere")
        compare(got, ref, "random", f"{off} {want}")


# ---- reproducibility -----------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    """The gradients depend on the atomic slot sums only through the two counts, which are sums of ones: bit-identical from call to call, with a
    fresh workspace or a used one, on the default stream or another.  The terms are sums of fractions whose order may change: within allowance."""
    case = R.build_case(257, 289, "random", seed=3)
    first = call(case)
    second = call(case, workspace=first["workspace"])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third = call(case, stream=side.cuda_stream)
        fourth = call(case, stream=side.cuda_stream, workspace=third["workspace"])
    for other in (second, third, fourth):
        for k in R.GRADS:
            assert np.array_equal(bits(first[k]), bits(other[k])), k
        for k in R.TERMS:
            assert abs(other[k] - first[k]) <= R.allowance("random", k) * abs(first[k]), (k, first[k], other[k])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_written():
    L, _ = _lib()
    case = R.build_case(10, 11, "random")

    def field(name, value=None):
        def edit(a, args, ws):
            setattr(a, name, value)
            return args, ws
        return edit
    invalid = [field("image"), field("gt"), field("losses"), field("height", 0), field("width", -3), field("height", -1), field("depth"),
               field("gt_depth"), field("weight"), field("sky_mask"), lambda a, args, ws: (None, ws)]
    for edit in invalid:
        assert call(case, edit=edit)["rc"] == L.EMD_ERR_INVALID
    assert call(case, edit=lambda a, args, ws: (args, None))["rc"] == L.EMD_ERR_WORKSPACE
    assert call(case, short=1)["rc"] == L.EMD_ERR_WORKSPACE
    assert call(case)["rc"] == L.EMD_OK


# ---- through emd_amd.loss.image_loss -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["lambda_sky 0", "lambda_depth 0", "detached image, no sky pixel"])
def test_image_loss_hands_on_the_reference_gradients(what):
    """The host op allocates its gradient buffers uninitialised: a term that is off, or a sky mask without a sky pixel beside an image that needs
    no gradient, must still hand zeros -- not that memory -- to the rasterizer backward.  Upstream gradient 2.5."""
    from emd_amd.loss import image_loss
    case = R.build_case(35, 97, "random", seed=4, sky="none" if "no sky" in what else "many")
    lam = dict(R.LAMBDAS)
    if what.startswith("lambda"):
        lam[what.split()[0]] = 0.0
    ref = R.reference(case, **lam)
    dev = lambda k, grad=False: torch.from_numpy(case[k]).to(DEV)[None].requires_grad_(grad)
    image = torch.from_numpy(case["image"]).to(DEV).requires_grad_("detached" not in what)
    depth, weight = dev("depth", "detached" not in what), dev("weight", True)           # (detached: dL_dweight is the ONLY gradient requested)
    for n in (1, 3):                                            # memory that the caching allocator hands out next: NaN, not the zeros of a fresh page
        junk = [torch.full((n, case["H"], case["W"]), float("nan"), device=DEV) for _ in range(4)]
        del junk
    total, terms = image_loss(image, torch.from_numpy(case["gt"]).to(DEV), depth, dev("gt_depth"), dev("mask"), weight,
                              torch.from_numpy(case["sky_mask"] != 0).to(DEV)[None], max_depth=case["max_depth"], **lam)
    (total * 2.5).backward()
    got = dict(total=total.item(), l1=terms["l1"].item(), ssim=terms["ssim"].item(), depth=terms["depth"].item(), sky=terms["sky"].item())
    for k, t in (("g_image", image), ("g_depth", depth), ("g_weight", weight)):
        if t.grad is not None:
            got[k] = (t.grad / 2.5).cpu().numpy().reshape(ref[k].shape)
    assert set(got) & set(R.GRADS) == ({"g_weight"} if "detached" in what else set(R.GRADS))
    compare(got, ref, "random", what)
    zero = {"lambda_sky 0": "g_weight", "lambda_depth 0": "g_depth", "detached image, no sky pixel": "g_weight"}[what]
    assert not ref[zero].any() and not bits(got[zero]).any(), (what, zero)
