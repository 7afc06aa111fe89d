"""-m gpu: `emd_adam_step` (csrc/optim.hip) driven through ctypes as emd_amd.optim.Adam.step fills EmdAdamArgs, against the float64 reference
and the per-element bounds of tests/adam_ref.py (whose docstring states the input set, the bounds and how their constants were fixed).

Memory: one flat device buffer per role (param, grad, exp_avg, exp_avg_sq); the 32 tensors are carved out of it with at least 8 guard words
(a fixed NaN bit pattern, compared as int32) in front of, between and behind them.  After every launch every guard word, every grad word and
every word of a tensor the launch did not name is bit-identical.
Values: STEPS consecutive steps from the kernel's own fp32 state (the reference starts each step from the kernel's previous output, so the
bounds do not compound); one NaN and one Inf gradient element; the capturable form (step and learning rate on the device, steps 1, 2, 3, 10,
1000, 30000 and on); every refusal of the entry point; two launches on the same inputs give the same bits.
Every test prints the worst observed multiple of each bound; adam_ref.py's docstring records them."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import adam_ref as ar

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
STEPS_DEV = (1, 2, 3, 10, 1000, 30000)


class Slabs:
    def __init__(self, specs):
        self.specs = specs
        carved = [ar.carve(specs, s) for s in range(4)]
        self.starts = [c[0] for c in carved]
        self.buf = [torch.full((c[1],), int(ar.GUARD_BITS), dtype=torch.int32, device=DEV) for c in carved]
        for i, sp in enumerate(specs):
            self.put(0, i, ar.initial_param(i, sp))
            self.put(2, i, np.zeros(sp.numel, np.float32))
            self.put(3, i, np.zeros(sp.numel, np.float32))
            self.put(1, i, ar.gradient(i, sp, 0))

    def put(self, slab, i, values):
        s = self.starts[slab][i]
        self.buf[slab][s:s + self.specs[i].numel] = torch.from_numpy(np.ascontiguousarray(values)).view(torch.int32).to(DEV)

    def ptr(self, slab, i):
        p = self.buf[slab].data_ptr() + 4 * self.starts[slab][i]
        assert p % 16 == 4 * self.specs[i].offs[slab]
        return p

    def host(self):
        """The four slabs on the host as float32 numpy (bit copies)."""
        torch.cuda.synchronize()
        return [b.cpu().numpy().view(np.float32) for b in self.buf]

    def cut(self, host, slab, i):
        s = self.starts[slab][i]
        return host[slab][s:s + self.specs[i].numel]

    def assert_only_named_written(self, before, after, named):
        for slab in range(4):
            keep = np.ones(before[slab].shape, dtype=bool)
            if slab != 1:
                for i in named:
                    s = self.starts[slab][i]
                    keep[s:s + self.specs[i].numel] = False
            assert np.array_equal(before[slab].view(np.int32)[keep], after[slab].view(np.int32)[keep]), f"slab {slab}: a word outside the named tensors changed"
        for slab in range(4):           # (the guards are where they were carved, and still hold the pattern)
            g = np.ones(after[slab].shape, dtype=bool)
            for i, sp in enumerate(self.specs):
                g[self.starts[slab][i]:self.starts[slab][i] + sp.numel] = False
            assert g.sum() >= ar.GUARD_WORDS * (len(self.specs) + 1) and bool((after[slab].view(np.int32)[g] == ar.GUARD_BITS).all())


def launch(slabs, named, scalars, step_dev=None, lr_dev=None, edit=None, num_tensors=None):
    """One emd_adam_step over the tensors `named` (in that order) -> return code."""
    from emd_amd import _lib as L
    a = L.EmdAdamArgs()
    a.num_tensors = len(named) if num_tensors is None else num_tensors
    for slot, i in enumerate(named):
        t, s = a.tensors[slot], scalars[i]
        t.param, t.grad, t.exp_avg, t.exp_avg_sq = (slabs.ptr(k, i) for k in range(4))
        t.numel = slabs.specs[i].numel
        t.step_size, t.bias_correction2_sqrt, t.one_minus_beta1, t.beta2, t.one_minus_beta2, t.eps = (float(x) for x in s)
        if step_dev is not None:
            t.step_dev, t.lr_dev = step_dev.data_ptr() + 4 * i, lr_dev.data_ptr() + 4 * i
    if edit is not None:
        edit(a)
    rc = L.load().emd_adam_step(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def host_scalars(specs, k):
    return [ar.host_scalars(sp.step0 + k, sp.lr, *sp.betas, sp.eps) for sp in specs]


def compare(slabs, before, after, named, reference, worst, skip=None):
    """Every named tensor against reference(i, p, g, m, v) -> (ref, bounds); `skip[i]`: elements left out (checked by the caller)."""
    for i in named:
        p, g, m, v = (slabs.cut(before, k, i) for k in range(4))
        ref, (bm, bv, bp) = reference(i, p, g, m, v)
        ok = np.ones(p.shape, dtype=bool)
        if skip and i in skip:
            ok[skip[i]] = False
        got_m, got_v, got_p = slabs.cut(after, 2, i), slabs.cut(after, 3, i), slabs.cut(after, 0, i)
        x = (ar.multiple(got_m[ok], ref[0][ok], bm[ok]), ar.multiple(got_v[ok], ref[1][ok], bv[ok]),
             ar.multiple(got_p[ok].astype(np.float64) - p[ok], ref[3][ok], bp[ok]))
        for key, val in zip(("m", "v", "update_tiny" if slabs.specs[i].tiny else "update"), x):
            worst[key] = max(worst.get(key, 0.0), val)
        assert max(x) <= 1.0, (i, slabs.specs[i], x)


def test_steps_of_a_full_batch_meet_the_bounds_and_write_nothing_else():
    from emd_amd import _lib as L
    specs = ar.batch()
    assert len(specs) == L.ADAM_MAX_TENSORS and specs[0].numel == specs[16].numel == specs[31].numel == 0
    slabs, named, worst = Slabs(specs), list(range(len(specs))), {}
    for k in range(ar.STEPS):
        for i, sp in enumerate(specs):
            slabs.put(1, i, ar.gradient(i, sp, k))
        sc, before = host_scalars(specs, k), slabs.host()
        assert launch(slabs, named, sc) == L.EMD_OK
        after = slabs.host()
        slabs.assert_only_named_written(before, after, named)

        def reference(i, p, g, m, v):
            ref = ar.adam_step64(p, g, m, v, sc[i])
            return ref, ar.bounds(ref, g, m, sc[i], specs[i].tiny)
        compare(slabs, before, after, named, reference, worst)
    print("emd_adam_step, full batch, worst multiple of each bound:", {k: round(x, 3) for k, x in worst.items()})


def test_a_partial_batch_leaves_the_other_tensors_alone_and_repeats_bit_for_bit():
    from emd_amd import _lib as L
    specs = ar.batch()
    slabs, named, worst = Slabs(specs), [30, 3, 16, 17, 9, 24, 12, 21], {}
    sc, before = host_scalars(specs, 0), slabs.host()
    start = [b.clone() for b in slabs.buf]
    assert launch(slabs, named, sc) == L.EMD_OK
    after = slabs.host()
    slabs.assert_only_named_written(before, after, named)

    def reference(i, p, g, m, v):
        ref = ar.adam_step64(p, g, m, v, sc[i])
        return ref, ar.bounds(ref, g, m, sc[i], specs[i].tiny)
    compare(slabs, before, after, named, reference, worst)
    for b, s in zip(slabs.buf, start):
        b.copy_(s)
    assert launch(slabs, named, sc) == L.EMD_OK
    again = slabs.host()
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(after, again))
    print("emd_adam_step, partial batch, worst multiple of each bound:", {k: round(x, 3) for k, x in worst.items()})


def test_non_finite_gradients_stay_in_their_elements():
    from emd_amd import _lib as L
    specs = ar.batch()
    slabs, named, worst = Slabs(specs), list(range(len(specs))), {}
    assert launch(slabs, named, host_scalars(specs, 0)) == L.EMD_OK           # one clean step first: the moments are no longer zero
    poison = {11: [100, 2050], 22: [5, 1023]}                                 # a vector-path tensor and a scalar-path one: [NaN at, Inf at]
    for i, sp in enumerate(specs):
        g = ar.gradient(i, sp, 1)
        if i in poison:
            g[poison[i][0]], g[poison[i][1]] = np.nan, -np.inf
        slabs.put(1, i, g)
    sc, before = host_scalars(specs, 1), slabs.host()
    assert launch(slabs, named, sc) == L.EMD_OK
    after = slabs.host()
    slabs.assert_only_named_written(before, after, named)

    def reference(i, p, g, m, v):
        ref = ar.adam_step64(p, g, m, v, sc[i])
        return ref, ar.bounds(ref, g, m, sc[i], specs[i].tiny)
    compare(slabs, before, after, named, reference, worst, skip=poison)
    for i, at in poison.items():
        ref = ar.adam_step64(*(slabs.cut(before, k, i) for k in range(4)), sc[i])
        for slab, r in ((2, ref[0]), (3, ref[1]), (0, ref[2])):
            got = slabs.cut(after, slab, i)[at]
            assert not np.isfinite(r[at]).any() and np.array_equal(np.isnan(got), np.isnan(r[at])) and np.array_equal(got[~np.isnan(got)], r[at][~np.isnan(got)]), (i, slab, got, r[at])
    print("emd_adam_step, NaN / Inf gradients, worst multiple of each bound elsewhere:", {k: round(x, 3) for k, x in worst.items()})


def test_capturable_form_reads_step_and_rate_from_the_device_and_ignores_the_host_scalars():
    from emd_amd import _lib as L
    specs = ar.batch()
    slabs, named, worst = Slabs(specs), list(range(len(specs))), {}
    steps = np.array([STEPS_DEV[(i + i // 6) % 6] for i in range(len(specs))], np.float32)           # every step value meets every pair of betas
    lrs = np.array([1.7 * sp.lr for sp in specs], np.float32)
    step_dev, lr_dev = torch.tensor(steps, device=DEV), torch.tensor(lrs, device=DEV)
    for k in range(3):
        for i, sp in enumerate(specs):
            slabs.put(1, i, ar.gradient(i, sp, k + 1))
        # step_size / bias_correction2_sqrt of the struct: values that would miss the bound by far if the kernel used them
        sc = [s._replace(step_size=np.float32(5.0), bias_correction2_sqrt=np.float32(0.01)) for s in host_scalars(specs, 0)]
        before = slabs.host()
        assert launch(slabs, named, sc, step_dev, lr_dev) == L.EMD_OK
        after = slabs.host()
        slabs.assert_only_named_written(before, after, named)
        assert np.array_equal(step_dev.cpu().numpy(), steps + k) and np.array_equal(lr_dev.cpu().numpy(), lrs)

        def reference(i, p, g, m, v):
            ref = ar.adam_step64_capturable(p, g, m, v, steps[i] + k, lrs[i], sc[i])
            return ref, ar.bounds(ref, g, m, sc[i], specs[i].tiny, capturable_step=steps[i] + k)
        for i in named:
            compare(slabs, before, after, [i], reference, worst.setdefault(int(steps[i]), {}))
        step_dev += 1.0
    for t0 in STEPS_DEV:
        print(f"emd_adam_step, capturable, steps {t0}..{t0 + 2}, worst multiple of each bound:", {k: round(x, 3) for k, x in worst[t0].items()})


def test_refusals_and_empty_batches_write_nothing():
    from emd_amd import _lib as L
    specs = ar.batch()
    slabs, sc = Slabs(specs), host_scalars(specs, 0)
    before = slabs.host()
    dev = torch.ones(len(specs), device=DEV)
    named = [3, 0, 7]

    def null(field):
        return lambda a: setattr(a.tensors[2], field, None)
    bad = {"num_tensors -1": dict(num_tensors=-1), "num_tensors 33": dict(num_tensors=L.ADAM_MAX_TENSORS + 1),
           "negative numel": dict(edit=lambda a: setattr(a.tensors[0], "numel", -1)),
           "step_dev without lr_dev": dict(step_dev=dev, lr_dev=dev, edit=null("lr_dev")),
           "bias_correction2_sqrt 0": dict(edit=lambda a: setattr(a.tensors[2], "bias_correction2_sqrt", 0.0)),
           "bias_correction2_sqrt < 0": dict(edit=lambda a: setattr(a.tensors[0], "bias_correction2_sqrt", -0.5))}
    bad.update({f"NULL {f}": dict(edit=null(f)) for f in ("param", "grad", "exp_avg", "exp_avg_sq")})
    for what, kw in bad.items():
        assert launch(slabs, named, sc, **kw) == L.EMD_ERR_INVALID, what
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(before, slabs.host())), what
    for what, kw in {"no tensors": dict(named=[]), "empty tensors only": dict(named=[0, 16, 31])}.items():
        assert launch(slabs, kw["named"], sc) == L.EMD_OK, what
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(before, slabs.host())), what
