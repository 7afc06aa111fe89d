"""-m gpu: OmniRe's ConditionalDeformNetwork on the fused fp32-MFMA kernels of csrc/deform_mlp.hip (ConditionalDeformNetwork(fused=True); DESIGN.md
section 8.20) against the float64 network of tests/deform_mlp_ref.py, the reference golden, and itself: identical bits across runs, streams and graph
replays; guarded buffers; the refusals.  tests/test_deform_mlp_cpu.py sends the float32 torch formulation through the same criterion."""
import ctypes as C
import functools

import pytest
import torch

from emd_amd import _lib as L
from emd_amd import deformation
from tests import deform_mlp_ref as R
from tests import test_deform_gpu as deform_base
from tests.test_track_det_gpu import _same_bits_everywhere

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_fused_network_matches_float64(name):
    ref = R.reference(name)
    c = ref.case
    assert ref.kink_share <= R.kink_cap(c.W), ref.kink_share
    if name == "groups":                                          # the rows span more than one group of the weight-gradient kernels
        lay = L.deform_mlp_layout(c.N, c.W, R.in_dim(c), _cus())
        assert lay["group_rows"] == L.DEFORM_MLP_MIN_GROUP_ROWS < c.N and lay["groups"] == 2
    report = []
    worst = R.worst_ratio(name, lambda net, h0: net.trunk(h0), device=DEV, fused=True, report=report)
    print(name, "worst error / bound:", worst, max(report, key=lambda p: p[1]))
    assert worst <= 1.0, report


def test_golden_holds_with_the_fused_network(monkeypatch):
    """tests/test_deform_gpu.test_nonrigid_deformation_matches_reference_golden as it stands, its bars, with fused=True."""
    monkeypatch.setattr(deformation, "ConditionalDeformNetwork", functools.partial(deformation.ConditionalDeformNetwork, fused=True))
    made = []
    real = deformation._DeformTrunk.apply
    monkeypatch.setattr(deformation._DeformTrunk, "apply", lambda *a: (made.append(1), real(*a))[1])
    deform_base.test_nonrigid_deformation_matches_reference_golden()
    assert len(made) == 2                                          # nonrigid_deformation and the reference signature both took the fused path


def _scene(name, deterministic=True):
    """A DeformableNodes-shaped call on a case's network: rows of three actors, interleaved."""
    c = R.CASES[name]
    net = R.make_network(c, fused=True).to(DEV)
    g = torch.Generator().manual_seed(5)
    means = (torch.rand(c.N, 3, generator=g) - 0.5).to(DEV)
    ids = torch.randint(0, 3, (c.N, 1), generator=g).to(DEV)
    size = (torch.rand(3, 3, generator=g) + 1.0).to(DEV)
    emb = torch.randn(3, c.E, generator=g).to(DEV).requires_grad_(True)
    t = torch.tensor([0.4], device=DEV)
    gouts = [torch.randn(c.N, w, generator=g).to(DEV) for w in (3, 4, 3)]
    leaves = [emb] + list(net.parameters())

    def step():
        outs = deformation.nonrigid_deformation(net, means, ids, size, emb, t, deterministic=deterministic)
        grads = torch.autograd.grad(sum((o * go).sum() for o, go in zip(outs, gouts)), leaves)
        return [o.detach() for o in outs] + list(grads)
    return net, step


def test_no_blas_call_is_left(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the fused network must not call tall_linear")
    monkeypatch.setattr(deformation, "tall_linear", refuse)
    monkeypatch.setattr(deformation, "tall_linear_relu", refuse)
    net, step = _scene("full-97")
    out = step()
    assert all(torch.isfinite(o).all() for o in out)
    net.fused = False                                              # (the patch bites: the default path does call them)
    with pytest.raises(AssertionError, match="tall_linear"):
        step()


@pytest.mark.parametrize("name", ["full-1000", "groups"])
def test_identical_bits_across_runs_streams_and_graph_replay(name):
    _same_bits_everywhere(_scene(name)[1])


def _round(n, m=64):
    return -(-n // m) * m


class _Guarded:
    """The buffers of one emd_deform_mlp_forward + _backward pair carved from ONE NaN-filled allocation with at least 64 NaN floats either side of each."""

    def __init__(self, name):
        ref = R.reference(name)
        c = self.c = ref.case
        net = R.make_network(c)
        net.load_state_dict(ref.state)
        self.net = net.to(DEV)
        self.x = ref.h0.to(DEV)
        self.gouts = [g.to(DEV) for g in ref.gouts]
        N, W, Cin, D = c.N, c.W, R.in_dim(c), c.D
        self.lay = L.deform_mlp_layout(N, W, Cin, _cus())
        lins = list(self.net.linear)
        sizes = [("h%d" % i, N * W) for i in range(D)] + [("out%d" % k, N * w) for k, w in enumerate((3, 4, 3))]
        sizes += [(f"dw{i}", lins[i].weight.numel()) for i in range(D)] + [(f"db{i}", W) for i in range(D)]
        sizes += [(f"dwh{k}", w * W) for k, w in enumerate((3, 4, 3))] + [(f"dbh{k}", w) for k, w in enumerate((3, 4, 3))]
        sizes += [("dx", N * Cin), ("gh0", N * W), ("gh1", N * W), ("slab", self.lay["bytes"] // 4)]
        self.at, pos = {}, 64
        for key, n in sizes:
            self.at[key] = (pos, n)
            pos = _round(pos + n) + 64
        self.buf = torch.full((pos,), float("nan"), device=DEV)
        assert self.buf.data_ptr() % 256 == 0

    def ptr(self, key):
        return self.buf.data_ptr() + 4 * self.at[key][0]

    def view(self, key):
        s, n = self.at[key]
        return self.buf[s:s + n]

    def structs(self):
        c, net = self.c, self.net
        a, g = L.EmdDeformMlpArgs(), L.EmdDeformMlpGrads()
        a.num_points, a.depth, a.width, a.in_dim, a.embed_dim, a.skip, a.ld_x, a.num_cus = c.N, c.D, c.W, R.in_dim(c), c.E, net.skips[0], R.in_dim(c), _cus()
        a.x = self.x.data_ptr()
        for i, lin in enumerate(net.linear):
            a.w[i], a.b[i], a.h[i], g.d_w[i], g.d_b[i] = lin.weight.data_ptr(), lin.bias.data_ptr(), self.ptr(f"h{i}"), self.ptr(f"dw{i}"), self.ptr(f"db{i}")
        for k, head in enumerate(R.heads_of(net)):
            a.w_head[k], a.b_head[k], a.out[k] = head.weight.data_ptr(), head.bias.data_ptr(), self.ptr(f"out{k}")
            g.g_out[k], g.d_w_head[k], g.d_b_head[k] = self.gouts[k].data_ptr(), self.ptr(f"dwh{k}"), self.ptr(f"dbh{k}")
        g.d_x, g.ld_dx = self.ptr("dx"), R.in_dim(c)
        g.g_h[0], g.g_h[1], g.slab, g.slab_bytes = self.ptr("gh0"), self.ptr("gh1"), self.ptr("slab"), self.lay["bytes"]
        return a, g

    def written(self):
        """Mask over the allocation of what the contract says the pair writes."""
        c, lay, m = self.c, self.lay, torch.zeros_like(self.buf, dtype=torch.bool)
        for key, (s, n) in self.at.items():
            if key == "dx":
                cols = torch.arange(n, device=DEV) % R.in_dim(c) >= R.in_dim(c) - c.E
                m[s:s + n] = cols
            elif key == "slab":
                m[s:s + lay["groups"] * lay["pitch_w"]] = True
                m[s + lay["offset_b"] // 4:s + lay["offset_b"] // 4 + lay["groups"] * lay["pitch_b"]] = True
            else:
                m[s:s + n] = True
        return m


@pytest.mark.parametrize("name", ["w32-33", "groups"])
def test_every_promised_element_is_written_and_nothing_else(name):
    q = _Guarded(name)
    a, g = q.structs()
    L.launch("emd_deform_mlp_forward", C.byref(a))
    L.launch("emd_deform_mlp_backward", C.byref(a), C.byref(g))
    torch.cuda.synchronize()
    nan, written = torch.isnan(q.buf), q.written()
    assert not bool((nan & written).any()), "a promised element came back NaN"
    assert bool((nan | written).all()), "an element outside the contract was written"
    # ... and they are the bits of the autograd path
    q.net.fused = True
    for k, o in enumerate(q.net.trunk(q.x)):
        assert torch.equal(o.reshape(-1), q.view(f"out{k}"))


_REFUSALS = {
    "width 48": (lambda a, g: setattr(a, "width", 48), L.EMD_ERR_INVALID),
    "width 288": (lambda a, g: setattr(a, "width", 288), L.EMD_ERR_INVALID),
    "depth 1": (lambda a, g: setattr(a, "depth", 1), L.EMD_ERR_INVALID),
    "concat before the heads": (lambda a, g: setattr(a, "skip", a.depth - 1), L.EMD_ERR_INVALID),
    "null input": (lambda a, g: setattr(a, "x", None), L.EMD_ERR_INVALID),
    "null weight": (lambda a, g: a.w.__setitem__(2, None), L.EMD_ERR_INVALID),
    "null saved activation": (lambda a, g: a.h.__setitem__(1, None), L.EMD_ERR_INVALID),
    "misaligned saved activation": (lambda a, g: a.h.__setitem__(1, a.h[1] + 4), L.EMD_ERR_INVALID),
    "no slab": (lambda a, g: setattr(g, "slab", None), L.EMD_ERR_WORKSPACE),
    "short slab": (lambda a, g: setattr(g, "slab_bytes", g.slab_bytes - 1), L.EMD_ERR_WORKSPACE),
    "misaligned slab": (lambda a, g: setattr(g, "slab", g.slab + 16), L.EMD_ERR_WORKSPACE),
    "null weight gradient": (lambda a, g: g.d_w.__setitem__(0, None), L.EMD_ERR_INVALID),
    "null head gradient": (lambda a, g: g.g_out.__setitem__(1, None), L.EMD_ERR_INVALID),
    "one scratch buffer": (lambda a, g: g.g_h.__setitem__(1, g.g_h[0]), L.EMD_ERR_INVALID),
}


@pytest.mark.parametrize("what", sorted(_REFUSALS))
def test_refusals_write_nothing(what):
    q = _guarded_once()
    a, g = q.structs()
    change, code = _REFUSALS[what]
    change(a, g)
    lib = L.load()
    backward_only = what in ("no slab", "short slab", "misaligned slab", "null weight gradient", "null head gradient", "one scratch buffer")
    if not backward_only:
        assert lib.emd_deform_mlp_forward(C.byref(a), L.stream()) == code, what
        assert lib.emd_last_error()
    assert lib.emd_deform_mlp_backward(C.byref(a), C.byref(g), L.stream()) == code, what
    assert lib.emd_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(q.buf).all())


@functools.lru_cache(maxsize=None)
def _guarded_once():
    return _Guarded("w32-33")          # (never launched on: the refusal tests leave it NaN-filled)


def test_python_refusals():
    for kw, word in ((dict(D=8, W=48), "multiple of 32"), (dict(D=2, W=32), "concat")):
        net = deformation.ConditionalDeformNetwork(embed_dim=4, fused=True, **kw).to(DEV)
        with pytest.raises(NotImplementedError, match=word):
            net(torch.zeros(5, 3, device=DEV), torch.zeros(5, 1, device=DEV), torch.zeros(5, 4, device=DEV))
    net = deformation.ConditionalDeformNetwork(D=4, W=32, embed_dim=4, fused=True)          # parameters left on the host
    with pytest.raises(L.EmdError, match="no CPU path"):
        net.trunk(torch.zeros(5, net.input_ch, device=DEV))


def test_empty_input_launches_nothing():
    net = deformation.ConditionalDeformNetwork(D=4, W=32, embed_dim=4, fused=True).to(DEV)
    h0 = torch.zeros(0, net.input_ch, device=DEV, requires_grad=True)
    outs = net.trunk(h0)
    assert [tuple(o.shape) for o in outs] == [(0, 3), (0, 4), (0, 3)]
    sum(o.sum() for o in outs).backward()
    assert all(p.grad is not None and float(p.grad.abs().sum()) == 0.0 for p in net.parameters())


def _parent_trunk(net, h0):
    """ConditionalDeformNetwork.trunk of the commit before `fused` existed, verbatim."""
    tall_linear, tall_linear_relu = deformation.tall_linear, deformation.tall_linear_relu
    h, skipped = h0, False
    for i, lin in enumerate(net.linear):
        if skipped:
            h = tall_linear(h, lin.weight[:, net.input_ch:], tall_linear(h0, lin.weight[:, :net.input_ch], lin.bias))
            h = torch.relu(h)
        else:
            h = tall_linear_relu(h, lin.weight, lin.bias)
        skipped = i in net.skips
    out = lambda lin: tall_linear(h, lin.weight, lin.bias)
    return (out(net.gaussian_warp), out(net.gaussian_rotation) if net.deform_quat else None, out(net.gaussian_scaling) if net.deform_scale else None)


def test_default_path_keeps_its_bits():
    ref = R.reference("full-97")
    results = []
    for trunk in (_parent_trunk, lambda net, h0: net.trunk(h0)):
        net = R.make_network(ref.case)
        assert net.fused is False
        net.load_state_dict(ref.state)
        net = net.to(DEV)
        h0 = ref.h0.to(DEV).requires_grad_(True)
        outs = trunk(net, h0)
        sum((o * g.to(DEV)).sum() for o, g in zip(outs, ref.gouts)).backward()
        results.append([o.detach() for o in outs] + [h0.grad] + [p.grad for p in net.parameters()])
    assert len(results[0]) == len(results[1]) and all(torch.equal(a, b) for a, b in zip(*results))
