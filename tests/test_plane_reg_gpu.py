"""-m gpu: the HexPlane regularisers on the device (emd_amd.hexplane.plane_regulation, csrc/plane_reg.hip) against the fp64 restatement of
tests/plane_reg_ref.py under the criterion of DESIGN.md section 5: values, terms and every plane gradient, sign(0) = 0, the GaussianModel methods,
bit-reproducibility (eager, a side stream, hipGraph replay) and that every gradient element is written.

The shapes (tests/plane_reg_ref.py CASES) and what each is for:
  tiny         C = 5, [5, 3, 4, 3]: H = 3 (one d2 row, every gradient row a boundary row) and H = 4; W * C = 15, 20, 25 floats: tails, rows off 16-byte alignment
  tiny_h5      C = 5, [4, 5, 3, 4]: adds H = 5, the first H with a fully interior gradient row
  two_scales   C = 32, [9, 7, 6, 5] + [18, 14, 12, 5]: planes of different sizes in one launch
  chunks       C = 32, [40, 5, 4, 3] and C = 5, [300, 4, 3, 5]: W * C = 1280 and 1500, two column chunks with the second partly filled (wide / dword accesses)
  segments     C = 16, H one below, at and one above a multiple of EMD_PLANE_REG_SEG; the last spans three segments
  workload     C = 32, [512, 512, 512, 25]: the workload's reduction length (8.4 M elements per plane), where accumulation width can go wrong"""
import ctypes as C

import pytest
import torch

from emd_amd import _lib as L
from emd_amd import hexplane
from tests import plane_reg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _device_grids(grids):
    """Leaves on the device in channel-last memory, as init_grid_param creates them."""
    return [[p.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True) for p in g] for g in grids]


def _run(grids, weights=R.WEIGHTS, leaves=None):
    leaves = leaves or _device_grids(grids)
    for g in leaves:
        for p in g:
            p.grad = None
    loss, terms = hexplane.plane_regulation(leaves, return_terms=True, **weights)
    assert loss.dim() == 0 and terms.shape == (3,) and loss.requires_grad and not terms.requires_grad
    (R.UPSTREAM * loss + 1).backward()
    return dict(loss=loss.detach(), terms=terms, grads=[[p.grad for p in g] for g in leaves])


@pytest.mark.parametrize("name", list(R.CASES))
def test_values_terms_and_all_plane_gradients_match_the_fp64_reference(name):
    got = _run(R.case(name))
    for g in got["grads"]:
        for t in g:
            assert t[0].permute(1, 2, 0).is_contiguous()                    # channel-last, like the planes
    R.criterion(got, R.reference(name, DEV), name)


def test_planes_that_are_not_channel_last_or_fp32_are_copied():
    grids = R.case("tiny_h5-s5e-2")
    leaves = [[p.to(DEV).contiguous().double().requires_grad_(True) for p in g] for g in grids]            # NCHW memory, fp64
    R.criterion(_run(None, leaves=leaves), R.reference("tiny_h5-s5e-2", DEV), "NCHW fp64 leaves")


def test_time_planes_at_exactly_one_have_zero_l1_and_zero_l1_gradient():
    """sign(0) = 0: init_grid_param leaves every time-plane entry at the kink of |1 - x|."""
    field = hexplane.HexPlaneField(1.6, {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 8, "resolution": [6, 5, 7, 4]},
                                   [1, 2]).to(DEV)
    loss, terms = field.regulation(0.0, 1.0, 0.0, return_terms=True)
    loss.backward()
    assert float(terms[2]) == 0.0 and float(terms[1]) == 0.0 and float(loss) == 0.0 and float(terms[0]) > 0.0
    for g in field.grids:
        for p in g:
            assert p.grad is not None and float(p.grad.abs().max()) == 0.0       # the spatial planes' weight is 0, the time planes sit at the kink
    for g in field.grids:
        for p in g:
            p.grad = None
    loss, terms = field.regulation(1.0, 1.0, 1.0, return_terms=True)
    loss.backward()
    for g in field.grids:
        for p in R.TIME:
            assert float(g[p].grad.abs().max()) == 0.0                          # flat along time as well: no smoothness gradient either
        for p in R.SPATIAL:
            assert float(g[p].grad.abs().max()) > 0.0


def _small_model():
    from emd_amd.deformation import DeformOptions, deform_network
    from emd_amd.gaussian_model import GaussianModel
    opt = DeformOptions(multires=[1, 2], kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 8,
                                                         "resolution": [6, 5, 7, 4]})
    net = deform_network(opt).to(DEV)
    grids = net.deformation_net.grid.grids
    src = R.make_grids(8, [[6, 5, 7, 4], [12, 10, 14, 4]], 0.05, seed=3)
    with torch.no_grad():
        for g, s in zip(grids, src):
            for p, q in zip(g, s):
                assert p.shape == q.shape
                p.copy_(q.to(DEV))
    return GaussianModel(device=DEV, deformation=net), grids, src


def test_gaussian_model_methods_reproduce_each_term_and_their_weighted_sum():
    gm, grids, src = _small_model()
    w = R.WEIGHTS
    ref = R.run(src, torch.float64, DEV)
    loss, terms = gm._hexplane_field().regulation(return_terms=True, **w)
    singles = torch.stack([gm._plane_regulation(), gm._time_regulation(), gm._l1_regulation()]).detach()
    assert torch.equal(singles, terms)                                          # each weight alone IS the term, bit for bit
    total = gm.compute_regulation(w["time_smoothness_weight"], w["l1_time_planes_weight"], w["plane_tv_weight"])        # the reference's argument order
    assert torch.equal(total.detach(), loss.detach())
    (R.UPSTREAM * total + 1).backward()
    got = dict(loss=total.detach(), terms=singles, grads=[[p.grad for p in g] for g in grids])
    R.criterion(got, ref, "GaussianModel.compute_regulation")
    weighted = w["plane_tv_weight"] * singles[0].double() + w["time_smoothness_weight"] * singles[1].double() + w["l1_time_planes_weight"] * singles[2].double()
    assert abs(float(total) - float(weighted)) <= 1e-5 * abs(float(weighted))
    # each method's gradient alone: only its planes, only its term
    for fn, key in ((gm._plane_regulation, "plane_tv_weight"), (gm._time_regulation, "time_smoothness_weight"), (gm._l1_regulation, "l1_time_planes_weight")):
        for g in grids:
            for p in g:
                p.grad = None
        value = fn()
        (R.UPSTREAM * value + 1).backward()
        one = {k: (1.0 if k == key else 0.0) for k in w}
        R.criterion(dict(loss=value.detach(), terms=singles, grads=[[p.grad for p in g] for g in grids]), R.run(src, torch.float64, DEV, weights=one), key + " alone")


def _flat(res):
    return [res["loss"].reshape(1), res["terms"]] + [t for g in res["grads"] for t in g]


@pytest.mark.parametrize("name", ["two_scales-s5e-2", "segments-s1e-3"])
def test_bit_reproducible_across_runs_streams_and_graph_replay(name):
    leaves = _device_grids(R.case(name))
    first = _flat(_run(None, leaves=leaves))
    first = [t.clone() for t in first]
    second = _flat(_run(None, leaves=leaves))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = [t.clone() for t in _flat(_run(None, leaves=leaves))]
    torch.cuda.current_stream().wait_stream(side)
    side.synchronize()
    for i, (a, b, c) in enumerate(zip(first, second, third)):
        assert torch.equal(a, b) and torch.equal(a, c), i

    def step():
        loss, terms = hexplane.plane_regulation(leaves, return_terms=True, **R.WEIGHTS)
        grads = torch.autograd.grad(R.UPSTREAM * loss + 1, [p for g in leaves for p in g])
        return [loss.detach().reshape(1), terms] + list(grads)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for replay in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(first, captured)):
            assert torch.equal(a, b), (replay, i)


@pytest.mark.parametrize("name", ["tiny-s5e-2", "segments-s5e-2", "chunks-s5e-2", "chunks_odd-s1e-3"])
def test_every_gradient_element_is_written(name):
    """The C entry point on one flat buffer laid out as the autograd node lays it out, pre-filled with NaN: no NaN survives, nothing next to it is touched."""
    ch, resolutions, _ = R.CASES[name]
    cl = [p.to(DEV)[0].permute(1, 2, 0).contiguous() for g in R.case(name) for p in g]
    n = sum(t.numel() for t in cl)
    guard = 64
    flat = torch.full((n + 2 * guard,), float("nan"), device=DEV)
    a = L.EmdPlaneRegArgs()
    a.channels, a.num_scales = ch, len(resolutions)
    a.time_smoothness_weight, a.l1_time_planes_weight, a.plane_tv_weight = 0.5, 0.25, 2.0
    off = guard
    for s, res in enumerate(resolutions):
        for k in range(4):
            a.res[s][k] = res[k]
        for p in range(6):
            t = cl[s * 6 + p]
            a.planes[s][p], a.dL_dplanes[s][p] = t.data_ptr(), flat.data_ptr() + 4 * off
            off += t.numel()
    g = torch.ones(1, device=DEV)
    a.g = g.data_ptr()
    L.check(L.load().emd_plane_reg_backward(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "emd_plane_reg_backward")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(flat[guard:guard + n]).all())
    assert bool(torch.isnan(flat[:guard]).all()) and bool(torch.isnan(flat[guard + n:]).all())
