"""-m "not gpu": linear-blend skinning of SMPL nodes (emd_amd.smpl, csrc/skinning.hip) without a GPU -- the fp64 restatement of the contract
(tests/skinning_ref.py) checked against closed forms and its own numerical derivative, and the host layer: exported symbols, struct layout,
argument validation, the cached point layout, the refusal of CPU tensors."""
import ctypes as C

import pytest
import torch

from emd_amd import _lib as L
from emd_amd import smpl
from tests import skinning_ref as R

J = 24


def _rand(*s, seed=0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---- the reference itself ----------------------------------------------------------------------------

def test_parent_tables_agree():
    assert smpl.SMPL_PARENTS == R.SMPL_PARENTS and len(R.SMPL_PARENTS) == J
    for tab in (R.SMPL_PARENTS, R.PATH_PARENTS, R.STAR_PARENTS):
        assert tab[0] == -1 and all(0 <= tab[j] < j for j in range(1, J))


@pytest.mark.parametrize("parents", [R.SMPL_PARENTS, R.PATH_PARENTS, R.STAR_PARENTS])
def test_identity_pose_gives_identity_skinning_matrices(parents):
    theta = torch.zeros(3, J, 4, dtype=torch.float64)
    theta[..., 0] = 1.7                                                      # unnormalised identity
    A = R.joint_chain(theta, _rand(3, J, 3), parents)
    want = torch.cat([torch.eye(3, dtype=torch.float64), torch.zeros(3, 1, dtype=torch.float64)], 1).reshape(12)
    assert torch.allclose(A, want.expand(3, J, 12), atol=1e-14)


def test_matrix_to_quaternion_inverts_quat_to_R_up_to_sign():
    q = _rand(400, 4, seed=1) * (0.3 + torch.rand(400, 1, generator=torch.Generator().manual_seed(2), dtype=torch.float64))
    got, q_abs = R.matrix_to_quaternion(R.quat_to_R(q))
    unit = q / q.norm(dim=-1, keepdim=True)
    sign = torch.sign((got * unit).sum(-1, keepdim=True))
    assert torch.allclose(got * sign, unit, atol=1e-12)
    assert set(q_abs.argmax(-1).tolist()) == {0, 1, 2, 3}                   # every branch is taken
    assert float(q_abs.max(-1).values.min()) >= 1.0                         # the 0.1 floor never acts on the chosen row


def test_one_hot_root_weights_reduce_to_the_rigid_transform():
    P, N = 2, 16
    theta, joints, trans = _rand(P, J, 4, seed=3), _rand(P, J, 3, seed=4), _rand(P, 3, seed=5)
    joints[:, 0] = 0
    means, quats = _rand(N, 3, seed=6), _rand(N, 4, seed=7)
    ids = torch.arange(N) % P
    w = torch.zeros(N, J, dtype=torch.float64)
    w[:, 0] = 1
    wm, wq, wo, _ = R.skin(means, quats, torch.ones(N, dtype=torch.float64), ids, w, R.joint_chain(theta, joints), trans,
                           torch.tensor([True, False]))
    Rm = R.quat_to_R(theta[:, 0])[ids]
    assert torch.allclose(wm, torch.einsum("nij,nj->ni", Rm, means) + trans[ids], atol=1e-12)
    want_q = R.quat_act(R.quat_mult(R.quat_act(theta[:, 0])[ids], R.quat_act(quats)))
    sign = torch.sign((wq * want_q).sum(-1, keepdim=True))
    assert torch.allclose(wq * sign, want_q, atol=1e-12)
    assert torch.equal(wo, (ids == 0).double())


def test_unbound_rows_pass_through_in_the_reference():
    c = R.make_case(shuffled=True)
    D = lambda k: c[k].double()
    wm, wq, wo, _ = R.skin(D("means"), D("quats"), D("opacities"), c["ids"], D("weights"), R.joint_chain(D("theta"), D("joints")), D("trans"), c["valid"])
    u = c["ids"] < 0
    assert int(u.sum()) == 17
    assert torch.equal(wm[u], D("means")[u]) and torch.equal(wq[u], D("quats")[u]) and torch.equal(wo[u], D("opacities")[u])


def test_reference_gradcheck_fp64():
    P, N = 2, 8
    g = torch.Generator().manual_seed(8)
    leaf = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True)
    theta, means, quats, trans = leaf(P, J, 4), leaf(N, 3), leaf(N, 4), leaf(P, 3)
    opac = torch.rand(N, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.rand(N, J, generator=g, dtype=torch.float64) ** 4
    weights = (w / w.sum(-1, keepdim=True)).requires_grad_(True)
    joints, canon = 0.3 * _rand(P, J, 3, seed=9), torch.cat([R.quat_to_R(_rand(P, J, 4, seed=10)), _rand(P, J, 3, 1, seed=12)], -1).reshape(P, J, 12)
    ids = torch.tensor([0, 1, 1, -1, 0, 1, 0, 1])
    valid = torch.tensor([True, True])

    def f(theta, means, quats, opac, weights, trans):
        wm, wq, wo, q_abs = R.skin(means, quats, opac, ids, weights, R.joint_chain(theta, joints, R.SMPL_PARENTS, canon), trans, valid)
        return wm, wq, wo

    top = R.skin(means, quats, opac, ids, weights, R.joint_chain(theta, joints, R.SMPL_PARENTS, canon), trans, valid)[3].detach().sort(-1).values
    assert float((top[ids >= 0, 3] - top[ids >= 0, 2]).min()) > 1e-3        # no point near a branch boundary
    assert torch.autograd.gradcheck(f, (theta, means, quats, opac, weights, trans), eps=1e-6, atol=1e-6, rtol=1e-5, fast_mode=True)


def test_case_facts_the_gpu_tests_rely_on():
    """At most 1 % of the points sit within 1e-3 of a branch boundary of matrix_to_quaternion, and every branch is taken."""
    for shuffled in (False, True):
        c = R.make_case(shuffled=shuffled, canon=True)
        ref = R.reference(c)
        assert int(ref["tie"].sum()) <= 0.01 * sum(R.COUNTS)
        assert int(ref["branch_counts"].min()) >= 10, ref["branch_counts"]
        assert int((c["ids"] >= 0).sum()) == 500 and torch.bincount(c["ids"][c["ids"] >= 0], minlength=5).tolist() == list(R.COUNTS)


# ---- host layer --------------------------------------------------------------------------------------

NEW_SYMBOLS = ("emd_joint_chain_forward", "emd_joint_chain_backward", "emd_skin_forward", "emd_skin_backward")


def test_new_symbols_exported():
    lib = L.load()
    for n in NEW_SYMBOLS:
        assert n in L.EXPORTED_SYMBOLS and hasattr(lib, n)
    assert lib.emd_abi_version() == L.ABI_VERSION


def test_new_struct_layout_matches_c():
    """(The three structs and the EMD_SKIN_* constants against the compiler: tests/test_abi.py.)"""
    assert L.SKIN_PARTIAL_FLOATS == L.SKIN_JOINTS * 12 + 3


FAKE = 0x1000        # a non-null pointer value: every call below is refused on the host, before anything is launched or read


def _skin_args(n=500, p=5, chunks=5):
    a = L.EmdSkinArgs()
    a.num_points, a.num_instances, a.num_chunks = n, p, chunks
    for f in ("means", "quats", "opacities", "ids", "weights", "A", "trans", "chunks", "world_means", "world_quats", "opacities_out"):
        setattr(a, f, FAKE)
    return a


def _skin_grads():
    g = L.EmdSkinGrads()
    for f in ("g_world_means", "g_world_quats", "g_opacities_out", "d_means", "d_quats", "d_opacities", "partials"):
        setattr(g, f, FAKE)
    return g


def test_argument_validation_reports_errors():
    lib = L.load()
    bad = lambda rc, word: rc == L.EMD_ERR_INVALID and word in lib.emd_last_error()
    a = _skin_args()
    a.weights = None
    assert bad(lib.emd_skin_forward(C.byref(a), None), b"null")
    a = _skin_args(n=-1)
    assert bad(lib.emd_skin_forward(C.byref(a), None), b"num_points")
    a = _skin_args(p=0)
    assert bad(lib.emd_skin_forward(C.byref(a), None), b"num_instances")
    a = _skin_args()
    a.world_quats = None
    assert bad(lib.emd_skin_forward(C.byref(a), None), b"null output")
    # 500 points of 5 instances: 2 .. 7 chunks
    for chunks in (1, 8):
        assert bad(lib.emd_skin_backward(C.byref(_skin_args(chunks=chunks)), C.byref(_skin_grads()), None), b"chunk table inconsistent")
    a = _skin_args()
    a.chunks = None
    assert bad(lib.emd_skin_backward(C.byref(a), C.byref(_skin_grads()), None), b"chunk table inconsistent")
    g = _skin_grads()
    g.partials = None
    assert bad(lib.emd_skin_backward(C.byref(_skin_args()), C.byref(g), None), b"null gradient")
    assert bad(lib.emd_skin_backward(C.byref(_skin_args()), None, None), b"null gradient")
    assert bad(lib.emd_skin_forward(None, None), b"null")

    ch = L.EmdJointChainArgs()
    ch.num_instances, ch.theta, ch.joints, ch.parents, ch.A = 2, FAKE, FAKE, FAKE, FAKE
    ch.num_instances = 0
    assert bad(lib.emd_joint_chain_forward(C.byref(ch), None), b"num_instances")
    ch.num_instances, ch.parents = 2, None
    assert bad(lib.emd_joint_chain_forward(C.byref(ch), None), b"null")
    ch.parents, ch.A = FAKE, None
    assert bad(lib.emd_joint_chain_forward(C.byref(ch), None), b"null A")
    assert bad(lib.emd_joint_chain_backward(C.byref(ch), None, None, None, None, None, FAKE, None), b"exactly one")
    assert bad(lib.emd_joint_chain_backward(C.byref(ch), FAKE, FAKE, FAKE, None, None, FAKE, None), b"exactly one")
    assert bad(lib.emd_joint_chain_backward(C.byref(ch), None, FAKE, None, None, None, FAKE, None), b"instance_chunk_start")
    assert bad(lib.emd_joint_chain_backward(C.byref(ch), FAKE, None, None, None, None, None, None), b"nothing to compute")
    ch.theta = None
    assert bad(lib.emd_joint_chain_backward(C.byref(ch), FAKE, None, None, None, None, FAKE, None), b"null")


def test_skin_layout_unsorted_ids_with_an_empty_instance():
    g = torch.Generator().manual_seed(3)
    counts = [300, 0, 257, 5]                                               # instance 1 is empty
    ids = torch.cat([torch.full((n,), p) for p, n in enumerate(counts)] + [torch.full((9,), -1), torch.full((2,), -7)])
    ids = ids[torch.randperm(ids.numel(), generator=g)]
    layout = smpl.SkinLayout(4)
    lay = layout.prepare(ids)
    key = ids.clamp_min(-1)
    order = lay.order.long()
    assert torch.equal(order, torch.argsort(key, stable=True))              # stable: ascending point index inside an instance
    assert torch.equal(lay.ids32, ids.to(torch.int32))
    per_group = [11] + counts
    want_chunks = [(n + 255) // 256 for n in per_group]
    assert lay.num_chunks == sum(want_chunks) == lay.chunks.shape[0]
    assert lay.chunk_start.tolist() == torch.tensor(want_chunks).cumsum(0).tolist()
    seen = []
    for inst, first, cnt in lay.chunks.tolist():
        assert 0 < cnt <= 256
        rows = order[first:first + cnt]
        assert bool((key[rows] == inst).all())
        seen.append(rows)
    assert torch.equal(torch.cat(seen), order)                              # every point in exactly one chunk, in order
    for p, n in enumerate(counts):
        c0, c1 = lay.chunk_start[p], lay.chunk_start[p + 1]
        assert lay.chunks[c0:c1, 0].tolist() == [p] * ((n + 255) // 256)
        assert lay.chunks[c0:c1, 2].sum() == n
    # cached on the tensor's identity and version; an in-place edit or invalidate() rebuilds
    assert layout.prepare(ids) is lay
    ids[0] = 3 if int(ids[0]) != 3 else 0
    edited = layout.prepare(ids)
    assert edited is not lay and torch.equal(edited.ids32, ids.to(torch.int32))
    layout.invalidate()
    assert layout.prepare(ids) is not edited
    # sorted ids need no gather indirection
    srt = ids.sort().values
    assert smpl.SkinLayout(4).prepare(srt).order is None
    with pytest.raises(ValueError, match="num_instances"):
        smpl.SkinLayout(3).prepare(ids)


def test_cpu_tensors_are_refused():
    c = R.make_case()
    A = R.joint_chain(c["theta"].double(), c["joints"].double()).float()
    with pytest.raises(L.EmdError, match="no CPU path"):
        smpl.skin_gaussians(c["means"], c["quats"], c["opacities"], c["ids"], c["weights"], A, c["trans"], c["valid"])
    with pytest.raises(L.EmdError, match="no CPU path"):
        smpl.joint_transforms(c["theta"], c["joints"])
    with pytest.raises(L.EmdError, match="no CPU path"):
        smpl.posed_skin_gaussians(c["means"], c["quats"], c["opacities"], c["ids"], c["weights"], c["theta"], c["joints"], c["trans"], c["valid"])
    with pytest.raises(ValueError, match="parents"):
        smpl._parents_dev((-1,) + (5,) * 23, "cpu")
