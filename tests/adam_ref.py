"""float64 reference of one Adam step (`emd_adam_step`, csrc/optim.hip), its per-element bounds, and the input set that
tests/test_adam_ref_cpu.py (no GPU) and tests/test_adam_direct_gpu.py share.  TEST INFRASTRUCTURE ONLY.

Reference.  `adam_step64` evaluates the four formula lines of optim.hip in float64 numpy on float32 inputs, with the six scalars exactly as
the host hands them to the kernel (`host_scalars`: formed in double as emd_amd/optim.py does, each rounded to fp32).  `adam_step64_capturable`
is the device-scalar form: `step` and `lr` are fp32 values, `bc2 = sqrt(1 - beta2^step)` and `step_size = lr / (1 - b1^step)` are formed in
float64 from the fp32-rounded betas (`b1 = 1 - fp32(1 - beta1)`).

Bounds, per element, u = 2^-24, from the reference's own magnitudes (never from the output under test):
    m        K_m u (|m_ref| + (1 - beta1) |g - m_old|)
    v        K_v u |v_ref|
    update   K_p u (|dp_ref| + |p_ref|)          update = p_new(fp32) - p_old, dp_ref = p_ref - p_old
    capturable form: the update's bound gains  POW_ULP u (b1^t / (1 - b1^t) + 0.5 beta2^t / (1 - beta2^t)) |dp_ref|,  the error of powf in the
    two bias corrections (halved through the square root).  POW_ULP = 16 is OpenCL's full-profile bound for pow: the ROCm installation this
    was written against carries no document that states an ulp bound for powf.
An element whose bound is 0 (g = 0 on zero moments) must be exact.

Constants.  Measured on the CPU (test_adam_ref_cpu.py re-measures them on every run): the worst multiple of u x (the magnitudes above) that
oracle.adam_oracle.adam_step, a plain float32 numpy restatement of the same four lines, reaches against adam_step64 over all tensors and
steps of `batch()`, chained from its own fp32 state.  Times 4, because the kernel contracts into fmaf and may order the division otherwise.
    measured   m 1.57   v 2.58    update, ordinary gradients 46.47   update, gradients near eps 4.24
    constants  K_M = 7  K_V = 11  K_P = 186                           K_P_TINY = 17
With them each of the wrong variants of test_adam_ref_cpu.py (eps inside the bias correction, no second bias correction, beta2 for
1 - beta2, the neighbouring tensor's step size) exceeds a bound by more than 100 x somewhere in the set.

Worst multiples of the WHOLE bound that k_adam reached on an MI355X (printed by test_adam_direct_gpu.py):
    full batch, 4 steps      m 0.142   v 0.178   update 0.203   update of the tensors with gradients near eps 0.249
    partial batch, 1 step    m 0.068   v 0.167   update 0.008
    NaN / Inf step           m 0.139   v 0.166   update 0.023   near eps 0.149   (the elements beside the poisoned ones)
    capturable, 3 steps from step 1 / 2 / 3 / 10 / 1000 / 30000, the bound with its powf term:
        m <= 0.140   v <= 0.178   update 0.016 / 0.025 / 0.038 / 0.021 / 0.025 / 0.019   near eps 0.214 / 0.058 / 0.058 / 0.069 / - / 0.043

Input set (`batch()`): 32 tensors (EMD_ADAM_MAX_TENSORS) of 0, 1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 3*2048-1 elements (the
halves and the end of a 2048-element block, and the float4 tail), each seam once with all four pointers 16-byte aligned and once at
+4 / +8 / +12 bytes or with one misaligned slab only (an aligned param beside a misaligned moment); empty tensors in the first, the middle and
the last slot.  Every tensor has its own learning rate (1e-4 .. 1e-2), betas, eps (1e-15 / 1e-8) and step number.  Gradients of step k are
N(0, 1) 10^(k-2) with exact zeros in every fifth element, or -- `tiny` tensors -- |g| log-uniform over three decades around the tensor's eps
(where sqrt(v)/bc2 + eps and (sqrt(v) + eps)/bc2 part).  Half of the tensors start from p = 0 (the bound then holds no rounding of p)."""
import math
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
K_M, K_V, K_P, K_P_TINY = 7.0, 11.0, 186.0, 17.0
POW_ULP = 16.0
GUARD_WORDS = 8
GUARD_BITS = np.array([0xFFA5C3E1], dtype=np.uint32).view(np.int32)[0]        # a NaN payload no kernel here produces; compared as int32
STEPS = 4

Scalars = namedtuple("Scalars", "step_size bias_correction2_sqrt one_minus_beta1 beta2 one_minus_beta2 eps")
Spec = namedtuple("Spec", "numel offs lr betas eps step0 p_zero tiny")            # offs: start of the tensor in words mod 4, per slab (p, g, m, v)


def host_scalars(step, lr, beta1, beta2, eps):
    """The six fp32 scalars of EmdAdamTensor as emd_amd.optim.Adam.step forms them."""
    f = np.float32
    return Scalars(f(lr / (1 - beta1 ** step)), f(math.sqrt(1 - beta2 ** step)), f(1 - beta1), f(beta2), f(1 - beta2), f(eps))


def adam_step64(p, g, m, v, s):
    """-> (m, v, p, dp) in float64."""
    p, g, m, v = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (p, g, m, v))
    s = Scalars(*(float(np.float32(x)) for x in s))
    with np.errstate(all="ignore"):
        m1 = m + s.one_minus_beta1 * (g - m)
        v1 = v * s.beta2 + s.one_minus_beta2 * g * g
        p1 = p - s.step_size * (m1 / (np.sqrt(v1) / s.bias_correction2_sqrt + s.eps))
        return m1, v1, p1, p1 - p


def capturable_terms(step, s):
    """-> (b1^t / (1 - b1^t), beta2^t / (1 - beta2^t)) in float64 from the fp32-rounded betas."""
    t, b1, b2 = float(np.float32(step)), 1.0 - float(np.float32(s.one_minus_beta1)), float(np.float32(s.beta2))
    return b1 ** t / (1.0 - b1 ** t), b2 ** t / (1.0 - b2 ** t)


def adam_step64_capturable(p, g, m, v, step, lr, s):
    """The device-scalar form: `s.step_size` and `s.bias_correction2_sqrt` are ignored."""
    t, b1, b2 = float(np.float32(step)), 1.0 - float(np.float32(s.one_minus_beta1)), float(np.float32(s.beta2))
    s64 = s._replace(step_size=float(np.float32(lr)) / (1.0 - b1 ** t), bias_correction2_sqrt=math.sqrt(1.0 - b2 ** t))
    p, g, m, v = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        m1 = m + float(s.one_minus_beta1) * (g - m)
        v1 = v * b2 + float(s.one_minus_beta2) * g * g
        p1 = p - s64.step_size * (m1 / (np.sqrt(v1) / s64.bias_correction2_sqrt + float(s.eps)))
        return m1, v1, p1, p1 - p


def magnitudes(ref, g, m_old, s):
    """The three bracketed magnitudes of the bounds, without K u."""
    m, v, p, dp = ref
    g, m_old = np.asarray(g, dtype=np.float64), np.asarray(m_old, dtype=np.float64)
    return np.abs(m) + float(s.one_minus_beta1) * np.abs(g - m_old), np.abs(v), np.abs(dp) + np.abs(p)


def bounds(ref, g, m_old, s, tiny, capturable_step=None):
    """-> (bound of m, of v, of the update)."""
    mm, mv, mp = magnitudes(ref, g, m_old, s)
    bp = (K_P_TINY if tiny else K_P) * U * mp
    if capturable_step is not None:
        r1, r2 = capturable_terms(capturable_step, s)
        bp = bp + POW_ULP * U * (r1 + 0.5 * r2) * np.abs(ref[3])
    return K_M * U * mm, K_V * U * mv, bp


def multiple(got, ref, bound):
    """Worst |got - ref| / bound over the elements; an element with bound 0 must be exact (else inf).  0.0 for an empty tensor."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(all="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


SEAMS = (1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 3 * 2048 - 1)
_OFFS = ((1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (0, 0, 1, 0), (0, 0, 0, 2), (0, 3, 0, 0), (1, 0, 0, 0), (1, 2, 3, 0))
_BETAS = ((0.9, 0.999), (0.8, 0.99), (0.5, 0.75))
_TINY_SIZES = (5, 1025, 2049, 4097)


def batch():
    """The 32 tensor specs."""
    al = (0, 0, 0, 0)
    lay = [(0, al, False)] + [(n, al, False) for n in SEAMS] + [(7, _OFFS[0], False), (2, _OFFS[3], False), (6, _OFFS[7], False)] + [(0, _OFFS[1], False)]
    lay += [(n, _OFFS[k % len(_OFFS)], n in _TINY_SIZES) for k, n in enumerate(SEAMS)] + [(1025, al, True), (9, _OFFS[2], False), (0, al, False)]
    assert len(lay) == 32
    return [Spec(n, offs, 10.0 ** (-4 + 2 * ((5 * i) % 32) / 31), _BETAS[i % 3], (1e-15, 1e-8)[(i // 3) % 2], i + 1, i % 2 == 0, tiny)
            for i, (n, offs, tiny) in enumerate(lay)]


def carve(specs, slab):
    """Start of every tensor in slab `slab` (0 param, 1 grad, 2 exp_avg, 3 exp_avg_sq), in words, and the slab's size: at least GUARD_WORDS
    guard words in front of, between and behind the tensors; start = offs[slab] mod 4."""
    cur, starts = 0, []
    for sp in specs:
        cur = (cur + GUARD_WORDS + 3) // 4 * 4 + sp.offs[slab]
        starts.append(cur)
        cur += sp.numel
    return starts, (cur + GUARD_WORDS + 3) // 4 * 4


def initial_param(i, sp):
    return np.zeros(sp.numel, np.float32) if sp.p_zero else np.random.default_rng([11, i]).standard_normal(sp.numel).astype(np.float32)


def gradient(i, sp, k):
    """The fp32 gradient of tensor i at step k of the sequence."""
    rng = np.random.default_rng([7, i, k])
    if sp.tiny:
        g = sp.eps * 10.0 ** rng.uniform(-1.5, 1.5, sp.numel) * rng.choice([-1.0, 1.0], sp.numel)
    else:
        g = rng.standard_normal(sp.numel) * 10.0 ** (k - 2)
    g[(np.arange(sp.numel) + k) % 5 == 0] = 0.0
    return g.astype(np.float32)
