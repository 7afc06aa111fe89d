"""CPU: tests/loss_ref.py -- the float64 reference of the image-loss tail that tests/test_loss_edges_gpu.py holds the kernel to -- pinned to the
golden vectors of the reference's own loss functions (tests/golden/s3g_loss.npz, at the tolerances of tests/test_loss_cpu.py) and to the float32
oracle on every case family; the builders' input conditions; and the float32 floor table (loss_ref.FLOORS), measured and asserted current."""
import os

import numpy as np
import pytest
import torch

from oracle import loss_oracle as lo
from tests import loss_ref as R

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def floors():
    return R.measure_floors()


def test_reference_matches_the_golden_values_and_gradients():
    g = np.load(os.path.join(G, "s3g_loss.npz"))
    sky = g["sky_mask"].reshape(g["image"].shape[-2:]) != 0
    hw = lambda k: g[k].reshape(sky.shape).astype(np.float32)
    case = dict(image=g["image"], gt=g["gt"], depth=hw("depth"), gt_depth=hw("gt_depth"), mask=(~sky).astype(np.float32), weight=hw("weight"),
                sky_mask=sky.astype(np.uint8))
    lam = g["lambdas"]
    ref = R.reference(case, float(lam[0]), float(lam[1]), float(lam[2]))
    for k, name in (("l1", "l1"), ("ssim", "ssim"), ("depth", "depth_l2"), ("sky", "sky"), ("total", "total")):
        np.testing.assert_allclose(ref[k], g[name], rtol=1e-6, err_msg=k)
    for k in R.GRADS:
        np.testing.assert_allclose(ref[k], g[k].reshape(ref[k].shape), atol=1e-9, rtol=1e-5, err_msg=k)
    # the fixture's own edge rows: no lidar return / beyond max depth, clamped weights
    assert np.all(ref["g_depth"][::3] == 0) and np.all(ref["g_depth"][:, :4] == 0) and np.all(ref["g_weight"][:2, :5] == 0)


def test_the_window_is_the_oracles_and_the_thresholds_are_the_float32_values():
    w1 = lo.window_1d().unsqueeze(1)
    assert torch.equal(R.window_2d(), w1.mm(w1.t()).float().double())
    assert abs(float(R.window_2d().sum()) - 1.0) < 1e-6
    # what a float32 implementation writes as 1.f - 1e-6f is the float32 of the reference's 1 - 1e-6
    assert np.float32(1) - np.float32(1e-6) == R.W_HI and R.W_LO == np.float32(1e-6) and R.DEPTH_LO == np.float32(0.01)
    # torch compares and clamps a float32 tensor against the scalar rounded to float32
    t = torch.tensor([R.DEPTH_LO, R.next_up(R.DEPTH_LO)])
    assert (t > 0.01).tolist() == [False, True]
    w = torch.tensor([R.next_down(R.W_LO), R.W_LO, R.W_HI, R.next_up(R.W_HI)], requires_grad=True)
    torch.clamp(w, min=1e-6, max=1.0 - 1e-6).sum().backward()
    assert w.grad.tolist() == [0.0, 1.0, 1.0, 0.0]
    # one ulp above max_depth does not survive the division: the clamp holds it back (80 + 2^-17 over 80 rounds to 1 + 2^-23)
    assert R.next_up(80.0) / np.float32(80.0) > 1 and np.float32(80.0) / np.float32(80.0) == 1


@pytest.mark.parametrize("family", R.FAMILIES)
def test_builders_keep_their_conditions(family):
    cases = R.family_cases(family)
    assert len(cases) >= len(R.ALL_SHAPES)
    for case in cases:
        assert R.conditions_hold(case), (family, case["H"], case["W"])
        big = case["H"] * case["W"] >= R.PLACE_MIN
        want = {name for name, *_ in R.DEPTH_ROWS} | {name for name, *_ in R.WEIGHT_ROWS} | {"image == gt"}
        assert set(case["placed"]) == (want if big else set())
        if case["mask"] is not None:
            assert set(np.unique(case["mask"]).tolist()) <= {0.0, 0.5, 1.0, 2.0}
    assert {None if c["mask"] is None else len(np.unique(c["mask"])) > 2 for c in cases if c["H"] * c["W"] > 100} == {None, False, True}
    assert {int(c["sky_mask"].sum() > 1) + int(c["sky_mask"].sum() > 0) for c in cases} == {0, 1, 2}
    if family == "equal":
        assert all(np.array_equal(c["image"], c["gt"]) for c in cases)
    if family == "wide":
        assert min(c["image"].min() for c in cases) < -0.5 and max(c["image"].max() for c in cases) > 1.5
    if family == "pixel":
        assert all((c["image"] != 0).sum() == 3 for c in cases)
        assert {(31, 31), (32, 32), (0, 0)} <= {tuple(np.argwhere(c["image"][0])[0]) for c in cases}


def test_placed_rows_decide_as_their_names_say():
    """On the gates the float32 outcome is exact: the reference's gradient is 0 where the name says the gate is shut and not 0 where it is open,
    under every mask kind."""
    for mask in ("none", "binary", "float"):
        case = R.build_case(33, 31, "random", seed=5, mask=mask)
        ref, dec = R.reference(case), R.decisions(case)
        for name, _gd, _pd, valid, passes in R.DEPTH_ROWS:
            (at,) = case["placed"][name]
            assert bool(dec["valid"].flat[at]) == valid, name
            assert (ref["g_depth"].flat[at] != 0) == bool(valid and passes), name
        for name, _w, passes in R.WEIGHT_ROWS:
            for at in case["placed"][name]:
                assert (ref["g_weight"].flat[at] != 0) == passes, name
        ref0 = R.reference(case, lambda_dssim=0.0)
        for at in case["placed"]["image == gt"]:
            assert (ref0["g_image"].reshape(3, -1)[:, at] == 0).all()
        assert set(np.unique(np.abs(ref0["g_image"])).tolist()) == {0.0, 1.0 / ref0["g_image"].size}


def test_terms_that_are_off_are_zero_with_zero_gradients():
    case = R.build_case(10, 11, "random")
    ref = R.reference(case, lambda_depth=0.0, lambda_sky=-0.05)
    assert ref["depth"] == 0 and ref["sky"] == 0 and not ref["g_depth"].any() and not ref["g_weight"].any()
    assert ref["total"] == pytest.approx(ref["l1"] + 0.2 * (1 - ref["ssim"]), rel=1e-14)
    dead = dict(case, gt_depth=np.zeros_like(case["gt_depth"]), sky_mask=np.zeros_like(case["sky_mask"]))
    ref = R.reference(dead)
    assert ref["depth"] == 0 and ref["sky"] == 0 and not ref["g_depth"].any() and not ref["g_weight"].any()
    ref = R.reference(case, use_depth=False, use_sky=False, lambda_dssim=0.0)
    assert ref["total"] == ref["l1"] and ref["ssim"] == 0 and not ref["g_depth"].any() and not ref["g_weight"].any()


@pytest.mark.parametrize("family", R.FAMILIES)
def test_reference_agrees_with_the_float32_oracle(floors, family):
    """The oracle is the reference's formulation in float32: on every case of the family it agrees with the float64 restatement within the bounds
    tests/test_loss_gpu.py grants a float32 implementation -- except dL/dimage of piecewise-constant blocks, where float32 loses
    sigma^2 = E[x^2] - mu^2 to cancellation (within 1e-3 of the largest entry there; the table carries the measured figure)."""
    for k in R.TERMS:
        assert floors[family][k] <= 1e-5, (family, k, floors[family][k])
    assert floors[family]["total share"] <= 1.0                 # the total, under the bound derived from the terms' (loss_ref.total_allowance)
    for k in R.GRADS:
        assert floors[family][k] <= (1e-3 if (family, k) == ("blocks", "g_image") else 1e-4), (family, k, floors[family][k])


def test_floor_table_is_current(floors):
    for family in R.FAMILIES:
        assert set(R.FLOORS[family]) == set(R.TERMS + R.GRADS)
        for k, table in R.FLOORS[family].items():
            now = floors[family][k]
            assert table >= 0.99 * R.HALF_ULP and table / 2 <= now <= table * 2, (family, k, table, now)
            assert R.allowance(family, k) <= (1e-4 if k in R.GRADS else 1e-5)
