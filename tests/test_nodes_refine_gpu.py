"""-m gpu: the refinement event of the OmniRe actor classes on the device -- emd_refine_nodes_decide / emd_refine_nodes_index behind
`density.restructure_node_rows`, and `nodes.RigidNodes` / `nodes.DeformableNodes` on top -- against `restructure_rows(REFINE)` where the two must
coincide (box test off, grouping off), against its own ungrouped output (grouping = a stable sort by actor), and against the torch restatement of
the reference (tests/nodes_refine_ref.py) on inputs whose float32 and float64 decisions agree (tests/test_nodes_refine_cpu.py asserts that, row by
row), so rows, ids and counts are compared exactly.  Positions of split samples: to the rounding bound of two float32 evaluations against the reference's float32 value, and BIT for bit against
the box test -- the position the decision tested is the position the gather stored."""
import ctypes as C
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nodes_refine_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAMES = ("means", "log_scales", "quats", "opacity", "tag", "moment")
# Two float32 evaluations of a split sample's position differ by at most 2 * 8 u * S, S the sum of magnitudes of ((R0 e0 + R1 e1) + R2 e2) + v.  In the
# cases of nodes_refine_ref: |v| <= 0.56 * 2 * 1.25 = 1.4; a kept row has exp(scale) <= 1.6 (cull size 1.0 after the division by 1.6) and the largest of
# the 3 * 9 000 normal draws is below 4.5, so sum |R_k e_k| <= sqrt(3) |e| <= 1.74 * 1.6 * 1.74 * 4.5 = 21.8: S <= 23.2, 16 u S = 2.2e-5.
POSITION_ATOL = 2.2e-5


def cases():
    return dict(R.gpu_cases())


def _device(case):
    N = case.means.shape[0]
    d = {k: getattr(case, k).to(DEV).float().contiguous() for k in ("means", "log_scales", "quats", "opacity", "grad_norm", "vis_counts", "max_2Dsize",
                                                                    "instances_size", "moment")}
    d["ids"] = case.ids.to(DEV).to(torch.int32).contiguous()
    d["tag"] = torch.arange(N, device=DEV, dtype=torch.float32)
    return d


def _jobs(L, d):
    return [(d["means"], L.DENSIFY_ROLE_XYZ), (d["log_scales"], L.DENSIFY_ROLE_SCALING), (d["quats"], L.DENSIFY_ROLE_COPY),
            (d["opacity"][:, None], L.DENSIFY_ROLE_COPY), (d["tag"][:, None], L.DENSIFY_ROLE_COPY), (d["moment"], L.DENSIFY_ROLE_STATE)]


def _fill(a, d, cfg):
    a.do_densify, a.do_cull, a.use_split_screen, a.cull_big, a.use_cull_screen = (int(cfg[k]) for k in ("do_densify", "do_cull", "use_split_screen", "cull_big",
                                                                                                     "use_cull_screen"))
    a.scaling, a.opacity, a.grad_norm, a.vis_counts, a.max_2Dsize = (d[k].data_ptr() for k in ("log_scales", "opacity", "grad_norm", "vis_counts", "max_2Dsize"))
    for k in ("grad_threshold", "size_threshold", "split_screen", "cull_alpha", "cull_size", "cull_screen"):
        setattr(a, k, cfg[k])


def run_nodes(case, group, box=None, normals=True, seed=5, d=None):
    """-> (outs by name or None, ids_out, segment_start, counts)"""
    from emd_amd import _lib as L
    from emd_amd.density import restructure_node_rows
    d = d or _device(case)
    a = L.EmdRefineNodesArgs()
    _fill(a, d, case.cfg)
    a.means, a.rotation, a.ids, a.instances_size = d["means"].data_ptr(), d["quats"].data_ptr(), d["ids"].data_ptr(), d["instances_size"].data_ptr()
    a.num_actors, a.num_samples, a.group_by_actor, a.seed = case.num_actors, case.num_samples, int(group), seed
    a.cull_out_of_bound = int(case.cfg["cull_out_of_bound"] if box is None else box)
    outs, ids_out, seg, counts = restructure_node_rows(a, _jobs(L, d), case.means.shape[0], samples=case.normals if normals else None)
    return (None if outs is None else dict(zip(NAMES, outs))), ids_out, seg, counts


def run_vanilla(case, split_mask, normals=True, seed=5):
    from emd_amd import _lib as L
    from emd_amd.density import restructure_rows
    d = _device(case)
    a = L.EmdRefineArgs()
    _fill(a, d, case.cfg)
    samples = case.normals[:, split_mask] if normals else None
    outs, counts = restructure_rows(L.DENSIFY_MODE_REFINE, a, _jobs(L, d), case.means.shape[0], seed=seed, samples=samples, scaling=d["log_scales"],
                                    rotation=d["quats"], num_samples=case.num_samples)
    return dict(zip(NAMES, outs)), counts


def _same(a, b, what):
    for k in NAMES:
        assert a[k].shape == b[k].shape and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k)


def _out_of_box(case, means, ids):
    half = case.instances_size.to(DEV)[ids.long()] / 2
    return (means.abs() > half).any(dim=-1)


# ---- 1. box test off, grouping off: the event of restructure_rows(REFINE) ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "N1000 A33 sorted", "N257 A3 interleaved"])
@pytest.mark.parametrize("normals", [False, True], ids=["philox", "supplied"])
def test_without_box_and_grouping_it_is_the_vanilla_event(name, normals):
    case = cases()[name]
    split = R.refine(case).split_mask
    want, (n_keep, n_dup, n_samp, n_split) = run_vanilla(case, split, normals)
    got, ids_out, seg, counts = run_nodes(case, group=False, box=False, normals=normals)
    _same(got, want, name)
    assert counts == (n_keep, n_dup, n_split, [n_samp] * case.num_samples) and seg is None and n_split == int(split.sum()) > 0
    assert ids_out.dtype == torch.int32 and torch.equal(ids_out.long(), case.ids.to(DEV)[got["tag"][:, 0].long()])


# ---- 2. grouping is the stable sort of the ungrouped order by actor ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "N1000 A513 interleaved", "N1000 A33 gaps", "N513 A3 sorted", "N257 A1 one"])
@pytest.mark.parametrize("normals", [False, True], ids=["philox", "supplied"])
def test_grouped_is_the_stable_sort_of_ungrouped(name, normals):
    case = cases()[name]
    flat, ids_flat, _, counts_flat = run_nodes(case, group=False, normals=normals)
    got, ids_out, seg, counts = run_nodes(case, group=True, normals=normals)
    order = torch.argsort(ids_flat.long(), stable=True)
    _same(got, {k: v[order] for k, v in flat.items()}, name)
    assert counts == counts_flat and torch.equal(ids_out, ids_flat[order])
    A = case.num_actors
    assert seg.dtype == torch.int32 and torch.equal(seg.long(), torch.searchsorted(ids_out.long(), torch.arange(A + 1, device=DEV)))
    assert int(seg[A]) == ids_out.numel() > 0


# ---- 3. the box cull against the reference; tested position = stored position ----------------------------------------------------------------------
def _against_reference(case, group, name):
    ref = R.refine(case, group=group)
    got, ids_out, seg, counts = run_nodes(case, group=group)
    if got is None:                                             # (the driver's "nothing changes": the reference keeps every row and adds none)
        assert ref.counts == counts == (case.means.shape[0], 0, 0, [0] * case.num_samples), name
        return None
    assert counts == ref.counts, (name, counts, ref.counts)
    assert torch.equal(got["tag"][:, 0].long().cpu(), ref.src) and torch.equal(ids_out.long().cpu(), ref.ids), name
    fresh = ref.kind != 0
    assert torch.equal(got["moment"].cpu(), torch.where(fresh[:, None], torch.zeros(1), case.moment[ref.src])), name
    torch.testing.assert_close(got["means"].cpu(), ref.means, rtol=0, atol=POSITION_ATOL, msg=name)
    torch.testing.assert_close(got["log_scales"].cpu(), ref.log_scales, rtol=2e-6, atol=2e-6, msg=name)
    assert torch.equal(got["means"].cpu()[ref.kind < 2], ref.means[ref.kind < 2]), name          # originals and duplicates are copies
    if ref.box_active:
        assert not bool(_out_of_box(case, got["means"], ids_out).any()), name                   # every stored row passes the test on its stored bits
    if group:
        assert torch.equal(seg.long().cpu(), torch.searchsorted(ref.ids, torch.arange(case.num_actors + 1))), name
    return got


@pytest.mark.parametrize("group", [False, True], ids=["reference_order", "grouped"])
def test_box_cull_matches_the_reference(group):
    _against_reference(cases()["box"], group, "box")


@pytest.mark.parametrize("normals", [False, True], ids=["philox", "supplied"])
def test_the_tested_position_is_the_stored_position(normals):
    """The same event without the box test stores EVERY candidate row, samples at their sampled positions.  The box test on those stored bits splits
    them into the rows the event with the box test must keep (every tensor bit-equal, in order) and the rows it must have culled."""
    case = cases()["box"]
    free, ids_free, _, counts_free = run_nodes(case, group=False, box=False, normals=normals)
    got, ids_out, _, counts = run_nodes(case, group=False, box=True, normals=normals)
    out = _out_of_box(case, free["means"], ids_free)
    _same(got, {k: v[~out] for k, v in free.items()}, "kept")
    assert torch.equal(ids_out, ids_free[~out])
    assert not bool(_out_of_box(case, got["means"], ids_out).any())
    new = free["moment"].abs().sum(-1) == 0                       # (no source moment row of the case is all zero)
    assert int((out & new).sum()) > 300 and int((~out & new).sum()) > 300 and int((out & ~new).sum()) > 100
    assert sum(counts_free[3]) - sum(counts[3]) + counts_free[1] - counts[1] == int((out & new).sum())


# ---- 4. shapes at the seams -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 255, 256, 257, 513, 1000])
def test_seams_against_the_reference(N):
    """A in {1, 3, 33, 513} (one and two 9-bit digits of the actor id) x ids sorted / round-robin / all on one actor / actors without points, the
    number of samples cycling through 1, 2, 3; grouped, box test on, supplied normals."""
    seen = set()
    for name, case in cases().items():
        if not name.startswith(f"N{N} "):
            continue
        seen.add((case.num_actors, case.num_samples))
        if N == 0:
            assert run_nodes(case, group=True) == (None, None, None, (0, 0, 0, [0] * case.num_samples))
        else:
            _against_reference(case, True, name)
    assert {a for a, _ in seen} == {1, 3, 33, 513} and {s for _, s in seen} == {1, 2, 3}


def test_no_points_zeroes_the_segment_table():
    from emd_amd import _lib as L
    lib = L.load()
    a = L.EmdRefineNodesArgs()
    a.num_points, a.num_actors, a.num_samples, a.group_by_actor = 0, 5, 2, 1
    seg = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.emd_refine_nodes_decide(C.byref(a), seg.data_ptr(), seg.data_ptr(), st) == L.EMD_OK          # nothing is launched, nothing written
    assert seg.tolist() == [-7] * 8
    assert lib.emd_refine_nodes_index(C.byref(a), 0, None, None, None, None, None, None, seg.data_ptr(), None, None, 0, st) == L.EMD_OK
    assert seg.tolist() == [0] * 6 + [-7] * 2


def test_everything_culled_and_nothing_to_do():
    case = types.SimpleNamespace(**vars(cases()["N513 A33 interleaved"]))
    case.opacity = torch.full_like(case.opacity, -12.0)
    got, ids_out, seg, counts = run_nodes(case, group=True)
    assert counts[0] == counts[1] == 0 and sum(counts[3]) == 0 and counts[2] > 0
    assert all(v.shape[0] == 0 for v in got.values()) and ids_out.numel() == 0 and seg.tolist() == [0] * 34
    # nothing above the gradient threshold, everything opaque, small and inside: the driver returns None and writes nothing
    case.opacity = torch.full_like(case.opacity, 3.0)
    case.grad_norm = torch.full_like(case.grad_norm, 1e-7)
    case.log_scales = torch.full_like(case.log_scales, -4.0)
    case.max_2Dsize = torch.zeros_like(case.max_2Dsize)
    case.means = case.means * 0.5
    d = _device(case)
    before = {k: v.clone() for k, v in d.items()}
    assert run_nodes(case, group=True, d=d) == (None, None, None, (513, 0, 0, [0] * case.num_samples))
    assert all(torch.equal(d[k], before[k]) for k in d)


def test_an_id_outside_the_actors_raises_before_anything_is_gathered():
    case = types.SimpleNamespace(**vars(cases()["N513 A33 sorted"]))
    for bad in (33, -1):
        case.ids = case.ids.clone()
        case.ids[300] = bad
        with pytest.raises(ValueError, match="1 point ids outside"):
            run_nodes(case, group=True)


# ---- 5. the classes -----------------------------------------------------------------------------------------------------------------------------------
CTRL = dict(sh_degree=1, warmup_steps=500, reset_alpha_interval=3000, refine_interval=100, n_split_samples=2, reset_alpha_value=0.01, densify_grad_thresh=0.0003,
            densify_size_thresh=0.025, cull_alpha_thresh=0.005, cull_scale_thresh=0.5, cull_screen_size=0.15, split_screen_size=0.05, stop_screen_size_at=4000,
            stop_split_at=15000, gaussian_embedding_dim=4, cull_out_of_bound=True, check_finite=False)
ATTR = dict(xyz="_means", sh_dc="_features_dc", sh_rest="_features_rest", opacity="_opacities", scaling="_scales", rotation="_quats", embedding="_embeddings")
A_, F_ = 5, 6


def _node(cls, g, N=1500, sorted_ids=False, **ctrl):
    node = cls("RigidNodes", {**CTRL, **ctrl}, scene_scale=2.0, num_train_images=10, device=DEV)
    size = torch.tensor([2.0, 1.0, 1.5]) * (0.75 + 0.5 * torch.rand(A_, 1, generator=g))
    ids = torch.randint(0, A_, (N,), generator=g)                                       # unsorted: the first event has to group them
    if sorted_ids:                                                                      # (sorted: the track heads' forward is a fixed function of its inputs)
        ids = torch.sort(ids).values
    node.create_from_tensors((torch.rand(N, 3, generator=g) * 2 - 1) * 0.55 * size[ids], torch.rand(N, 3, generator=g),
                             torch.log(torch.tensor(0.004)) + torch.rand(N, 3, generator=g) * 5.0, ids,
                             torch.randn(F_, A_, 4, generator=g), torch.randn(F_, A_, 3, generator=g), size, torch.rand(F_, A_, generator=g) < 0.8,
                             quats=torch.randn(N, 4, generator=g), embeddings=torch.randn(N, 4, generator=g))
    with torch.no_grad():
        node._opacities.copy_((torch.randn(N, 1, generator=g) * 3.0 - 1.0).to(DEV))
        node._features_rest.copy_((torch.randn(N, 3, 3, generator=g) * 0.1).to(DEV))
    node.set_cur_frame(2)
    return node


def _stats(node, g):
    n = node.num_points
    node.xys_grad_norm = (torch.rand(n, generator=g) * 1.2e-3).to(DEV)
    node.vis_counts = torch.randint(1, 4, (n,), generator=g).float().to(DEV)
    node.max_2Dsize = (torch.rand(n, generator=g) * 0.2).to(DEV)


def _heads(g):
    from emd_amd.motion import TrackOffsetHeads
    h = TrackOffsetHeads(A_, gaussian_embedding_dim=4)
    with torch.no_grad():
        for p in h.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return h.to(DEV)


@pytest.mark.parametrize("optimizer", ["hip_adam", "torch_adam"])
def test_rigid_nodes_three_events(optimizer):
    from emd_amd.motion import TrackOffsetHeads
    from emd_amd.nodes import RigidNodes
    from emd_amd.optim import Adam
    g = torch.Generator().manual_seed(21)
    node = _node(RigidNodes, g)
    heads = _heads(g)
    node.attach_track_heads(heads)
    groups = node.get_param_groups()
    p = node.class_prefix
    assert list(groups) == [p + k for k in ("xyz", "sh_dc", "sh_rest", "opacity", "scaling", "rotation", "ins_rotation", "ins_translation", "embedding")]
    opt = (Adam if optimizer == "hip_adam" else torch.optim.Adam)([{"params": v, "lr": 1e-3, "name": k} for k, v in groups.items()], lr=0.0, eps=1e-15)
    assert node.point_ids.dtype == torch.int64 and node.point_ids.shape == (1500, 1) and node.segment_start is None
    for event, step in enumerate((3600, 3700, 3800)):
        n = node.num_points
        tag = torch.arange(n, device=DEV, dtype=torch.float32)
        with torch.no_grad():
            node._embeddings[:, 0] = tag                                                # column 0 of a copied parameter names the source row
        old = {k: getattr(node, a).detach().clone() for k, a in ATTR.items()}
        old_ids = node.point_ids.clone()
        for k, a in ATTR.items():                                                       # moments that name their row: tag + 1 everywhere
            prm = getattr(node, a)
            opt.state[prm] = {"step": torch.tensor(2.0), "exp_avg": (tag + 1).reshape(n, *[1] * (prm.dim() - 1)).expand_as(prm).contiguous(),
                              "exp_avg_sq": (2 * tag + 2).reshape(n, *[1] * (prm.dim() - 1)).expand_as(prm).contiguous()}
        _stats(node, g)
        node.preprocess_per_train_step(step)
        info = node.refinement_after(step, opt)
        m = node.num_points
        assert info["n_before"] == n and info["n_after"] == m and info["split"] > 0 and info["dups_kept"] > 0 and 0 < info["originals_kept"] < n
        assert info["samples_kept"] < 2 * info["split"]                                 # the box test culled samples on their own
        src = node._embeddings.detach()[:, 0].long()
        assert node.point_ids.dtype == torch.int64 and node.point_ids.shape == (m, 1) and node.ids32.dtype == torch.int32
        assert torch.equal(node.point_ids[:, 0], old_ids[src, 0]) and torch.equal(node.ids32.long(), node.point_ids[:, 0])
        assert bool((node.ids32[1:] >= node.ids32[:-1]).all())                          # grouped: an actor's rows are contiguous
        assert torch.equal(node.segment_start.long(), torch.searchsorted(node.point_ids[:, 0].contiguous(), torch.arange(A_ + 1, device=DEV)))
        assert not bool(node.get_out_of_bound_mask().any())
        survivor = None
        for k, a in ATTR.items():
            prm = getattr(node, a)
            grp = [x for x in opt.param_groups if x["name"] == p + k][0]
            assert isinstance(prm, torch.nn.Parameter) and prm.shape[0] == m and len(grp["params"]) == 1 and grp["params"][0] is prm, k
            st = opt.state[prm]
            row = st["exp_avg"].reshape(m, -1)
            alive = row[:, 0] != 0
            survivor = alive if survivor is None else survivor
            assert torch.equal(alive, survivor) and int(alive.sum()) == info["originals_kept"], k
            want = torch.where(alive, src.float() + 1, torch.zeros(()).to(DEV))         # survivors keep their moments, new rows start at zero
            assert torch.equal(row, want[:, None].expand_as(row)) and torch.equal(st["exp_avg_sq"].reshape(m, -1), 2 * want[:, None].expand_as(row)), k
            if k not in ("xyz", "scaling"):
                assert torch.equal(prm.detach(), old[k][src]), k                        # copied rows, _embeddings among them
        assert torch.equal(node._means.detach()[survivor], old["xyz"][src[survivor]])
        for k in ("ins_rotation", "ins_translation"):                                   # the actor tables never change
            grp = [x for x in opt.param_groups if x["name"] == p + k][0]
            assert grp["params"][0] is getattr(node, RigidNodes.NODE_PARAM_GROUPS[k]) and grp["params"][0].shape[1] == A_
        # the track heads took the event's layout over: no re-preparation, and the same pose table as heads that prepare their own ids
        assert heads._seg is node.segment_start and heads._prepare_ids(node._ids_flat)[2] is node.segment_start
        pose = node._actor_pose()
        fresh = TrackOffsetHeads(A_, gaussian_embedding_dim=4).to(DEV)
        fresh.load_state_dict(heads.state_dict())
        want = fresh.pose_table(node.instances_quats, node.instances_trans, node.instances_fv, 2, node._embeddings, node.point_ids[:, 0].clone(), step)
        assert fresh._seg is not None and torch.equal(fresh._seg, heads._seg) and torch.equal(fresh._cnt, heads._cnt) and torch.equal(pose, want)
    assert node.refine_events == 3


def test_get_gaussians_are_the_node_functions():
    from emd_amd.deformation import ConditionalDeformNetwork
    from emd_amd.motion import build_actor_pose
    from emd_amd.nodes import DeformableNodes, RigidNodes, deformable_gaussians, rigid_gaussians
    g = torch.Generator().manual_seed(22)
    cam = types.SimpleNamespace(camtoworlds=torch.eye(4, device=DEV) + torch.tensor([[0, 0, 0, 0.3], [0, 0, 0, -2.0], [0, 0, 0, 5.0], [0, 0, 0, 0]], device=DEV))
    center = cam.camtoworlds[:3, 3]
    node = _node(RigidNodes, g, N=700, sorted_ids=True)
    node.preprocess_per_train_step(2500)
    kw = dict(sh_degree=1, step=2500, sh_degree_interval=1000, check_finite=False, deterministic=False)
    args = lambda n: (n._means, n._quats, n._opacities, n._scales, n._features_dc, n._features_rest, n.point_ids)
    same = lambda a, b: a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    pose = build_actor_pose(node.instances_quats, node.instances_trans, node.instances_fv, 2)
    assert same(node.get_gaussians(cam), rigid_gaussians(*args(node), pose, center, **kw))
    heads = _heads(g)
    node.attach_track_heads(heads)
    pose = heads.pose_table(node.instances_quats, node.instances_trans, node.instances_fv, 2, node._embeddings, node._ids_flat, 2500)
    got = node.get_gaussians(cam)
    assert same(got, rigid_gaussians(*args(node), pose, center, **kw)) and got["_means"].requires_grad
    # DeformableNodes
    node = _node(DeformableNodes, g, N=700)
    node.preprocess_per_train_step(2500)
    net = ConditionalDeformNetwork(D=4, W=32, input_ch=3, embed_dim=8, x_multires=4, t_multires=4).to(DEV)
    node.set_deformation(net, torch.randn(A_, 8, generator=g), torch.linspace(0, 1, F_))
    pose = build_actor_pose(node.instances_quats, node.instances_trans, node.instances_fv, 2)
    want = deformable_gaussians(net, *args(node), pose, center, node.instances_size, node.instances_embedding, node.normalized_timestamps[2].reshape(1),
                                use_deformation=True, stop_optimizing_canonical_xyz=True, **kw)
    assert same(node.get_gaussians(cam), want)
    assert isinstance(node, RigidNodes) and isinstance(node.instances_embedding, torch.nn.Parameter)


def test_a_bad_id_leaves_the_model_unchanged_and_ungrouped_keeps_the_reference_order():
    from emd_amd.nodes import RigidNodes
    from emd_amd.optim import Adam
    g = torch.Generator().manual_seed(23)
    node = _node(RigidNodes, g, N=600)
    opt = Adam([{"params": v, "lr": 1e-3, "name": k} for k, v in node.get_param_groups().items()], lr=0.0, eps=1e-15)
    _stats(node, g)
    node.preprocess_per_train_step(3600)
    before = {a: getattr(node, a) for a in ATTR.values()}
    ids_before = node.point_ids
    node.ids32[17] = A_                                              # an id equal to the number of actors
    with pytest.raises(ValueError, match="point ids outside"):
        node.refinement_after(3600, opt)
    assert all(getattr(node, a) is before[a] for a in ATTR.values()) and node.point_ids is ids_before and node.num_points == 600
    assert all(x["params"][0] is getattr(node, ATTR[x["name"].split("#")[1]]) for x in opt.param_groups if x["name"].split("#")[1] in ATTR)
    # group_by_actor False: the reference's order (survivors first, in source order), no segment table
    node = _node(RigidNodes, g, N=600, group_by_actor=False)
    old_ids = node.point_ids.clone()
    _stats(node, g)
    node.preprocess_per_train_step(3600)
    with torch.no_grad():
        node._embeddings[:, 0] = torch.arange(600, device=DEV)
    info = node.refinement_after(3600, None)
    src = node._embeddings.detach()[:, 0].long()
    k = info["originals_kept"]
    assert node.segment_start is None and bool((src[1:k] > src[:k - 1]).all()) and torch.equal(node.point_ids[:, 0], old_ids[src, 0])
    assert not bool((node.ids32[1:] >= node.ids32[:-1]).all())


# ---- 6. determinism --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "N1000 A513 interleaved"])
def test_the_event_is_deterministic_also_on_a_side_stream(name):
    case = cases()[name]
    d = _device(case)
    first = run_nodes(case, group=True, normals=False, d=d)
    second = run_nodes(case, group=True, normals=False, d=d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run_nodes(case, group=True, normals=False, d=d)
    side.synchronize()
    for other in (second, third):
        _same(first[0], other[0], name)
        assert torch.equal(first[1], other[1]) and torch.equal(first[2], other[2]) and first[3] == other[3]
