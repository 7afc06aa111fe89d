"""CPU: tests/adam_ref.py holds up without a GPU.
(a) adam_step64 reproduces the reference optimiser's recorded run (tests/golden/s3g_adam.npz) within the bar of test_adam_cpu.py.
(b) The constants K_M, K_V, K_P, K_P_TINY are 4 x the worst multiple that the float32 numpy oracle reaches against adam_step64 on the input
    set of the GPU test (chained from the oracle's own fp32 state, as the GPU test chains from the kernel's).
(c) The mutation condition: each of four wrong variants of the formula, run in float32 numpy on the same inputs, exceeds a bound by at
    least 100 x somewhere in that set -- so the bounds tell the right formula from these."""
import os

import numpy as np
import pytest

from oracle import adam_oracle as ao
from tests import adam_ref as ar
from tests.test_adam_cpu import schedule

G = os.path.join(os.path.dirname(__file__), "golden")


def test_adam_step64_reproduces_the_reference_optimizer_golden():
    g = np.load(os.path.join(G, "s3g_adam.npz"))
    # (the fixture stores the options as fp32; the optimiser ran with the Python doubles 0.9, 0.999, 1e-15, and 1 - fp32(0.999) is not 1e-3)
    assert abs(float(g["eps"]) / 1e-15 - 1) < 1e-6 and abs(float(g["beta1"]) - 0.9) < 1e-7 and abs(float(g["beta2"]) - 0.999) < 1e-7
    for n in (str(x) for x in g["group_names"]):
        p = g[f"init_{n}"]
        m, v = np.zeros_like(p), np.zeros_like(p)
        for k in range(len(g["iters"])):
            s = ar.host_scalars(k + 1, schedule(g, n, int(g["iters"][k])), 0.9, 0.999, 1e-15)
            m64, v64, p64, _ = ar.adam_step64(p, g[f"grad_{k}_{n}"], m, v, s)
            m, v, p = m64.astype(np.float32), v64.astype(np.float32), p64.astype(np.float32)          # the optimiser's state is fp32
        for got, key in ((m, "exp_avg"), (v, "exp_avg_sq"), (p, "final")):
            want = g[f"{key}_{n}"]
            np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-6 * np.abs(want).max(), err_msg=f"{key} {n}")


def wrong_step(p, g, m, v, s, variant, neighbour):
    """The four formula lines in float32 numpy with one deliberate error."""
    f = np.float32
    with np.errstate(all="ignore"):
        m = m + s.one_minus_beta1 * (g - m)
        v = v * s.beta2 + (s.beta2 if variant == "beta2_for_one_minus_beta2" else s.one_minus_beta2) * g * g
        if variant == "eps_inside":
            denom = (np.sqrt(v) + s.eps) / s.bias_correction2_sqrt
        elif variant == "no_bias_correction2":
            denom = np.sqrt(v) + s.eps
        else:
            denom = np.sqrt(v) / s.bias_correction2_sqrt + s.eps
        p = p - (neighbour.step_size if variant == "neighbour_step_size" else s.step_size) * (m / denom)
    return m.astype(f), v.astype(f), p.astype(f)


@pytest.fixture(scope="module")
def oracle_run():
    """Every (tensor, step) of the set: inputs, scalars, the fp64 reference and the float32 oracle's result, chained from the oracle's state."""
    specs, rows = ar.batch(), []
    for i, sp in enumerate(specs):
        if sp.numel == 0:
            continue
        p, m, v = ar.initial_param(i, sp), np.zeros(sp.numel, np.float32), np.zeros(sp.numel, np.float32)
        for k in range(ar.STEPS):
            g, s = ar.gradient(i, sp, k), ar.host_scalars(sp.step0 + k, sp.lr, *sp.betas, sp.eps)
            ref = ar.adam_step64(p, g, m, v, s)
            p1, m1, v1 = ao.adam_step(p, g, m, v, sp.step0 + k, sp.lr, *sp.betas, sp.eps)
            rows.append(dict(i=i, sp=sp, k=k, p=p, g=g, m=m, v=v, s=s, ref=ref, got=(m1, v1, p1)))
            p, m, v = p1, m1, v1
    return specs, rows


def test_constants_are_four_times_the_float32_oracles_worst_multiple(oracle_run):
    worst = dict(m=0.0, v=0.0, p=0.0, p_tiny=0.0)
    for r in oracle_run[1]:
        mm, mv, mp = (ar.U * x for x in ar.magnitudes(r["ref"], r["g"], r["m"], r["s"]))
        m1, v1, p1 = r["got"]
        worst["m"] = max(worst["m"], ar.multiple(m1, r["ref"][0], mm))
        worst["v"] = max(worst["v"], ar.multiple(v1, r["ref"][1], mv))
        key = "p_tiny" if r["sp"].tiny else "p"
        worst[key] = max(worst[key], ar.multiple(p1.astype(np.float64) - r["p"], r["ref"][3], mp))
    print("float32 oracle, worst multiples of u x magnitude:", {k: round(x, 2) for k, x in worst.items()})
    for key, K in (("m", ar.K_M), ("v", ar.K_V), ("p", ar.K_P), ("p_tiny", ar.K_P_TINY)):
        assert 4.0 * worst[key] <= K <= 4.0 * worst[key] + 1.0, (key, worst[key], K)          # 4 x measured, rounded up to an integer


@pytest.mark.parametrize("variant", ["eps_inside", "no_bias_correction2", "beta2_for_one_minus_beta2", "neighbour_step_size"])
def test_each_wrong_variant_exceeds_a_bound_a_hundredfold(oracle_run, variant):
    specs, rows = oracle_run
    nonempty = [i for i, sp in enumerate(specs) if sp.numel > 0]
    worst = 0.0
    for r in rows:
        j = nonempty[(nonempty.index(r["i"]) + 1) % len(nonempty)]                             # the next tensor that owns a block
        nb = ar.host_scalars(specs[j].step0 + r["k"], specs[j].lr, *specs[j].betas, specs[j].eps)
        m1, v1, p1 = wrong_step(r["p"], r["g"], r["m"], r["v"], r["s"], variant, nb)
        bm, bv, bp = ar.bounds(r["ref"], r["g"], r["m"], r["s"], r["sp"].tiny)
        worst = max(worst, ar.multiple(m1, r["ref"][0], bm), ar.multiple(v1, r["ref"][1], bv),
                    ar.multiple(p1.astype(np.float64) - r["p"], r["ref"][3], bp))
    print(variant, "worst multiple of a bound:", worst)
    assert worst >= 100.0


def test_the_right_formula_in_float32_is_within_the_bounds(oracle_run):
    for r in oracle_run[1]:
        bm, bv, bp = ar.bounds(r["ref"], r["g"], r["m"], r["s"], r["sp"].tiny)
        m1, v1, p1 = r["got"]
        assert ar.multiple(m1, r["ref"][0], bm) <= 0.25 and ar.multiple(v1, r["ref"][1], bv) <= 0.25
        assert ar.multiple(p1.astype(np.float64) - r["p"], r["ref"][3], bp) <= 0.25
