"""The premises of tests/test_sh_paths_gpu.py, checked without a GPU: the fp64 restatement of tests/sh_ref.py against the golden vectors of the
imported reference at every degree, the properties the kernels are held to (rows the degree does not use take no gradient, no gradient for the
directions at degree 0, no radial component in dL/ddirs), the conditions on the generated inputs, and the same formula in fp32 against the fp64
result under the project's criterion on every case of the GPU file -- the bar is met by plain fp32 arithmetic with room to spare, so a kernel
that misses it is wrong.  Run with -s to see the ratios."""
import numpy as np
import pytest
import torch

from tests import sh_ref as R
from tests.test_golden_cpu import ld

F32 = torch.float32


def test_reference_reproduces_the_golden_colours_at_every_degree():
    z = ld("s3g_sh.npz")
    shs, dirs = torch.tensor(z["shs"]), torch.tensor(z["xyz"] - z["campos"])
    assert shs.shape[1:] == (16, 3)
    for deg in range(4):
        ref = R.sh_colour(deg, shs, dirs)
        assert ref.dtype == torch.float64
        R.criterion(torch.tensor(z[f"sh_deg{deg}"]), ref, f"golden sh_deg{deg} (fp32, recorded) against sh_colour")
        K = (deg + 1) ** 2
        assert torch.equal(R.sh_colour(deg, shs[:, :K], dirs), ref), "rows >= (deg + 1)^2 do not enter the colour"


@pytest.mark.parametrize("deg,M", R.SH_DEG_ROWS)
def test_reference_gradient_properties(deg, M):
    c, ref = R.sh_case(deg, M, 1000), R.sh_reference(deg, M, 1000)
    K = c["K"]
    assert ref["d_coeffs"].shape == (1000, M, 3) and ref["d_coeffs"][:, :K].abs().min() > 0
    assert (ref["d_coeffs"][:, K:] == 0).all(), "rows the degree does not use take no gradient"
    dd, d = ref["d_dirs"], c["dirs"].double()
    if deg == 0:
        assert (dd == 0).all(), "degree 0 does not depend on the direction"
        return
    radial = (dd * d).sum(-1).abs().max()
    size = (dd.norm(dim=-1) * d.norm(dim=-1)).max()
    print(f"deg {deg} M {M}: largest radial component {float(radial):.2e} of {float(size):.2e}")
    assert size > 0 and radial <= 1e-12 * size


def test_input_conditions_of_the_stand_alone_cases():
    for deg, M, N in R.SH_CASES:
        c = R.sh_case(deg, M, N)
        nrm = c["dirs"].double().norm(dim=-1)
        assert c["dirs"].shape == (N, 3) and c["coeffs"].shape == (N, M, 3) and c["dirs"].dtype == F32
        assert R.DIR_NORM[0] <= float(nrm.min()) and float(nrm.max()) <= R.DIR_NORM[1]
    n1000 = torch.cat([R.sh_case(3, 16, 1000)["dirs"].double().norm(dim=-1)])
    assert float(n1000.min()) < 1.0 and float(n1000.max()) > 19.0            # the whole range of lengths is used


def _factor_keys():
    return [(deg, V, N, "shared", 1.0 / V) for deg, V, N in R.FACTOR_SWEEP] + list(R.FACTOR_FORM_CASES)


def test_input_conditions_of_the_factor_cases():
    for deg, V, N, form, _ in _factor_keys():
        c = R.factor_case(deg, V, N, form)
        zero = c["zero"]
        assert ((c["factors"] == 0).all(-1) == zero).all()
        assert int(zero.sum()) >= (V * N) // 3
        if V >= 2:
            assert bool(zero[0, 0]) and not bool(zero[1, 0]), "Gaussian 0: invisible in view 0, visible in view 1"
        if N >= 2:
            assert bool(zero[:, N - 1].all()), "the last Gaussian is invisible in every view"
        assert float(c["means"].abs().max()) <= 0.5
        for v in range(V):
            pose = c["pose"] if (c["pose"] is None or c["pose"].dim() == 2) else c["pose"][v]
            dist = (R.world_means(c["means"], c["ids"], pose, c["rdx"]) - c["campos"][v].double()).norm(dim=-1)
            assert float(dist.min()) >= R.CAMERA_DISTANCE, (deg, V, N, form, v, float(dist.min()))
        if form != "static":
            assert int((c["ids"] < 0).sum()) == (N + 1) // 3 and int(c["ids"].max()) < R.FACTOR_ACTORS
        if form == "per_view":
            assert c["pose"].shape == (V, R.FACTOR_ACTORS, 12) and not torch.equal(c["pose"][0], c["pose"][1])
        assert (c["rdx"] is not None) == (form == "residual")


def test_reference_dense_gradient_properties():
    for deg, V, N, form, scale in _factor_keys():
        c, ref = R.factor_case(deg, V, N, form), R.factor_reference(deg, V, N, form, scale)
        assert ref.shape == (N, 16, 3)
        assert (ref[:, c["K"]:] == 0).all()
        assert (ref[c["zero"].all(0)] == 0).all(), "a Gaussian no view sees gets a zero row"
        if N > 1:
            assert float(ref[:, :c["K"]].abs().max()) > 0


def test_clamp_premise_of_the_caller_cases():
    """No pre-clamp value of the fp64 reference lies within 1e-5 of a clamp edge, so the fp32 paths clamp the same elements; a seed that
    violated this would be replaced, no element is ever left out.  Each case has elements on both sides of every edge it clamps at."""
    for sh_degree, step in R.NODE_CASES:
        pre = R.node_reference(sh_degree, step)["pre"] + 0.5
        gap = float(torch.minimum(pre.abs(), (pre - 1.0).abs()).min())
        print(f"nodes sh_degree {sh_degree} step {step}: closest pre-clamp value {gap:.2e} from an edge; {int((pre < 0).sum())} below 0, "
              f"{int((pre > 1).sum())} above 1 of {pre.numel()}")
        assert gap > R.CLAMP_MARGIN
        assert bool((pre < 0).any()) and bool((pre > 1).any()) and bool(((pre > 0) & (pre < 1)).any())
    for deg in R.PRECOMPUTE_DEGREES:
        c = R.precompute_case(deg)
        pre = R.precompute_reference(deg)["pre"] + 0.5
        gap = float(pre.abs().min())
        print(f"pre_compute_colors degree {deg}: closest pre-clamp value {gap:.2e} from 0; {int((pre < 0).sum())} below 0 of {pre.numel()}")
        assert gap > R.CLAMP_MARGIN and bool((pre < 0).any()) and bool((pre > 0).any())
        dist = (c["xyz"].double() - c["camera_center"].double()).norm(dim=-1)
        assert float(dist.min()) >= R.CAMERA_DISTANCE


def test_node_cases_cover_the_degree_ramp():
    assert [R.node_case(d, s)["n"] for d, s in R.NODE_CASES] == [0, 1, 2, 3, 1, 2]
    assert [R.node_case(d, s)["features_rest"].shape[1] + 1 for d, s in R.NODE_CASES] == [16, 16, 16, 16, 4, 9]
    for d, s in R.NODE_CASES:
        ids = R.node_case(d, s)["point_ids"]
        assert int((ids >= 0).sum()) == R.NODE_POINTS // 3 and set(ids.tolist()) == {-1, 0, 1}
        ref = R.node_reference(d, s)
        rest = ref["d_features_rest"]
        K = (R.node_case(d, s)["n"] + 1) ** 2
        assert (rest[:, K - 1:] == 0).all() and (K == 1 or float(rest[:, :K - 1].abs().max()) > 0)
        assert float(ref["d_features_dc"].abs().max()) > 0


# ---- the same formula in fp32 against fp64, under the criterion, on every case the GPU file uses ----

@pytest.mark.parametrize("deg,M", R.SH_DEG_ROWS)
def test_fp32_restatement_meets_the_criterion_stand_alone(deg, M):
    for N in R.SH_COUNTS:
        lo, hi = R.sh_reference(deg, M, N, F32), R.sh_reference(deg, M, N)
        for k in ("colour", "d_coeffs", "d_dirs"):
            assert lo[k].dtype == F32 and hi[k].dtype == torch.float64
            R.criterion(lo[k], hi[k], f"fp32 restatement, sh deg {deg} M {M} N {N}: {k}")


def test_fp32_restatement_meets_the_criterion_dense_from_factors():
    for deg, V, N, form, scale in _factor_keys():
        lo, hi = R.factor_reference(deg, V, N, form, scale, F32), R.factor_reference(deg, V, N, form, scale)
        assert lo.dtype == F32
        R.criterion(lo, hi, f"fp32 restatement, factors deg {deg} V {V} N {N} {form} scale {scale:.3f}")


def test_fp32_restatement_meets_the_criterion_callers():
    for sh_degree, step in R.NODE_CASES:
        lo, hi = R.node_reference(sh_degree, step, F32), R.node_reference(sh_degree, step)
        for k in ("colour", "d_features_dc", "d_features_rest"):
            R.criterion(lo[k], hi[k], f"fp32 restatement, nodes sh_degree {sh_degree} step {step}: {k}")
    for deg in R.PRECOMPUTE_DEGREES:
        lo, hi = R.precompute_reference(deg, F32), R.precompute_reference(deg)
        for k in ("colour", "d_coeffs", "d_dirs"):
            R.criterion(lo[k], hi[k], f"fp32 restatement, pre_compute_colors degree {deg}: {k}")


def test_case_lists_hold_every_degree_seam_and_form():
    """The GPU file iterates these lists; shrinking one would shrink what it checks without a failure anywhere else."""
    assert R.SH_DEG_ROWS == ((0, 1), (0, 16), (1, 4), (1, 16), (2, 9), (2, 16), (3, 16)) and R.SH_COUNTS == (1, 255, 256, 257, 1000)
    sweep = set(R.FACTOR_SWEEP)
    assert all((2, 2, N) in sweep for N in (1, 127, 128, 129, 255, 256, 257, 700))
    assert all((deg, V, 257) in sweep for deg in range(4) for V in (1, 2, 3)) and len(sweep) == 19
    assert {(d, f) for d, _, _, f, _ in R.FACTOR_FORM_CASES} == {(d, f) for d in (1, 3) for f in ("static", "shared", "per_view", "residual")}
    assert {s for *_, s in R.FACTOR_FORM_CASES} == {1.0, 1.0 / 3.0}
    assert np.all([c[1:3] == (3, 700) for c in R.FACTOR_FORM_CASES])
