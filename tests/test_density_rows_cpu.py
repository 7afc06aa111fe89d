"""No GPU: `density.EventRows`, the one place that says which rows travel for a parameter and how the outputs return to the store and its
optimiser.  Plain CPU tensors and a torch.optim.Adam: neither the helper nor `hand_over` needs a device."""
import torch
from torch.nn import Parameter

from emd_amd import _lib as L
from emd_amd.density import EventRows


def test_moments_follow_their_parameter_and_return_to_the_new_leaf():
    N, M = 5, 7
    stepped, fresh, loose = Parameter(torch.randn(N, 3)), Parameter(torch.randn(N, 3)), Parameter(torch.randn(N, 1))
    opt = torch.optim.Adam([{"params": [stepped], "name": "xyz"}, {"params": [fresh], "name": "scaling"}], lr=1e-2)
    stepped.grad = torch.ones_like(stepped)                      # one step of the first group only: the second has no state yet
    opt.step()
    g_stepped, g_fresh = opt.param_groups
    st = opt.state[stepped]
    step, exp_avg, exp_avg_sq = st["step"], st["exp_avg"], st["exp_avg_sq"]
    assert fresh not in opt.state
    stat, table = torch.rand(N), torch.ones(N)

    rows = EventRows(opt)
    rows.add_param("stepped", stepped, L.DENSIFY_ROLE_XYZ, g_stepped)
    rows.add("stat", stat, L.DENSIFY_ROLE_ZERO)
    rows.add_param("fresh", fresh, L.DENSIFY_ROLE_SCALING, g_fresh)
    rows.add_param("loose", loose, L.DENSIFY_ROLE_COPY)          # a parameter no group holds
    rows.add("table", table, L.DENSIFY_ROLE_COPY)
    want = [(stepped, L.DENSIFY_ROLE_XYZ), (exp_avg, L.DENSIFY_ROLE_STATE), (exp_avg_sq, L.DENSIFY_ROLE_STATE), (stat, L.DENSIFY_ROLE_ZERO),
            (fresh, L.DENSIFY_ROLE_SCALING), (loose, L.DENSIFY_ROLE_COPY), (table, L.DENSIFY_ROLE_COPY)]
    assert len(rows.jobs) == len(want)
    for (t, role), (t_want, role_want) in zip(rows.jobs, want):
        assert t is t_want and role == role_want

    outs = [torch.randn((M,) + tuple(t.shape[1:])) for t, _ in rows.jobs]          # what a driver's gather would hand back, in job order
    got = rows.install(outs)
    assert list(got) == ["stepped", "stat", "fresh", "loose", "table"]
    for key, k in (("stepped", 0), ("fresh", 4), ("loose", 5)):
        assert isinstance(got[key], Parameter) and got[key].is_leaf and got[key].requires_grad and got[key].data_ptr() == outs[k].data_ptr()
    assert got["stat"] is outs[3] and got["table"] is outs[6]                       # other rows come back untouched

    assert len(g_stepped["params"]) == 1 and g_stepped["params"][0] is got["stepped"]
    assert len(g_fresh["params"]) == 1 and g_fresh["params"][0] is got["fresh"]
    assert [id(p) for p in opt.state] == [id(got["stepped"])]    # the old parameters are gone, the group that never stepped still has no state
    new = opt.state[got["stepped"]]
    assert new["exp_avg"] is outs[1] and new["exp_avg_sq"] is outs[2] and new["step"] is step
    got["stepped"].grad, got["fresh"].grad = torch.ones(M, 3), torch.ones(M, 3)
    opt.step()                                                   # the optimiser goes on with the seven rows
    assert float(opt.state[got["stepped"]]["step"]) == 2 and float(opt.state[got["fresh"]]["step"]) == 1


def test_front_rows_take_no_part_and_are_copied_over():
    N, front, M = 5, 2, 4                                        # 3 rows take part and become 4, behind the 2 in front
    p, stat = Parameter(torch.randn(N, 3)), torch.rand(N)
    opt = torch.optim.Adam([{"params": [p], "name": "xyz"}], lr=1e-2)
    p.grad = torch.ones_like(p)
    opt.step()
    old = p.detach().clone()
    exp_avg, exp_avg_sq = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
    rows = EventRows(opt, front_rows=front)
    rows.add_param("p", p, L.DENSIFY_ROLE_XYZ, opt.param_groups[0])
    rows.add("stat", stat, L.DENSIFY_ROLE_ZERO)
    for (t, _), whole in zip(rows.jobs, (p, exp_avg, exp_avg_sq, stat)):
        assert t.shape[0] == N - front and t.data_ptr() == whole[front:].data_ptr() and not t.requires_grad
    outs = [torch.full((front + M,) + tuple(t.shape[1:]), 7.0) for t, _ in rows.jobs]          # a driver leaves the front rows for the caller
    got = rows.install(outs)
    st = opt.state[got["p"]]
    for new, whole in ((got["p"].detach(), old), (st["exp_avg"], exp_avg), (st["exp_avg_sq"], exp_avg_sq), (got["stat"], stat)):
        assert new.shape[0] == front + M and torch.equal(new[:front], whole[:front]) and bool((new[front:] == 7.0).all())


def test_no_optimizer_no_moments():
    p = Parameter(torch.zeros(5, 3))
    rows = EventRows()
    rows.add_param("p", p, L.DENSIFY_ROLE_COPY)
    assert len(rows.jobs) == 1 and rows.jobs[0][0] is p
    out = torch.ones(7, 3)
    assert rows.install([out])["p"].data_ptr() == out.data_ptr()
