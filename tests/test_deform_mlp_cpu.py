"""-m "not gpu": the host side of the fused ConditionalDeformNetwork (csrc/deform_mlp.hip) -- the signature, the slab layout and its
refusals through the library, the kink caps of the float64 reference, and the float32 torch formulation of the network (today's trunk() with plain addmm
on CPU tensors) through the criterion the GPU test applies to the kernels: a GPU failure is then the kernels'."""
import ctypes as C
import inspect

import pytest
import torch

from emd_amd import _lib as L
from tests import deform_mlp_ref as R


def test_fused_is_off_by_default():
    from emd_amd.deformation import ConditionalDeformNetwork
    assert inspect.signature(ConditionalDeformNetwork.__init__).parameters["fused"].default is False
    net = ConditionalDeformNetwork(D=2, W=8, embed_dim=4)
    assert net.fused is False
    assert ConditionalDeformNetwork(D=4, W=32, embed_dim=4, fused=True).fused is True
    # parameter names and shapes do not depend on the flag: reference state_dicts load strictly either way
    a, b = ConditionalDeformNetwork(D=4, W=32, embed_dim=4), ConditionalDeformNetwork(D=4, W=32, embed_dim=4, fused=True)
    assert {k: v.shape for k, v in a.state_dict().items()} == {k: v.shape for k, v in b.state_dict().items()}
    b.load_state_dict(a.state_dict(), strict=True)


def test_fused_refusals_name_the_reason():
    from emd_amd.deformation import ConditionalDeformNetwork
    assert ConditionalDeformNetwork(fused=True).fused_refusal() is None
    for kw, word in ((dict(D=8, W=48), "multiple of 32"), (dict(D=8, W=288), "multiple of 32"), (dict(D=1, W=32), "D = 1"), (dict(D=2, W=32), "concat")):
        net = ConditionalDeformNetwork(embed_dim=4, fused=True, **kw)
        assert word in net.fused_refusal()
        with pytest.raises(NotImplementedError, match=word):
            net.trunk(torch.zeros(3, net.input_ch))


def test_workspace_layout_and_refusals():
    lay = L.deform_mlp_layout(160000, 256, 94, 256)
    rows = -(-160000 // 128)
    rows = -(-rows // 32) * 32
    assert lay["group_rows"] == rows == 1280 and lay["groups"] == 125
    assert lay["pitch_w"] == 256 * 256 and lay["pitch_b"] == 256 and lay["offset_w"] == 0
    assert lay["offset_b"] == 125 * 65536 * 4 and lay["bytes"] == lay["offset_b"] + 125 * 256 * 4
    # a function of N and the CU count alone; never fewer rows than the exported minimum, whole 32-row steps
    small = L.deform_mlp_layout(300, 64, 44, 256)
    assert small["group_rows"] == L.DEFORM_MLP_MIN_GROUP_ROWS and small["groups"] == 2 and small["pitch_w"] == 64 * 64
    assert L.deform_mlp_layout(300, 64, 44, 8)["group_rows"] == 256 and L.deform_mlp_layout(4000, 64, 44, 8)["group_rows"] == 1024
    assert L.deform_mlp_layout(97, 32, 94, 256)["pitch_w"] == 32 * 94          # the widest input of a layer sets the pitch
    assert L.deform_mlp_layout(0, 256, 94, 256)["bytes"] == 0
    assert L.deform_mlp_layout(1, 32, 94, 1) == dict(groups=1, group_rows=256, pitch_w=32 * 94, pitch_b=32, offset_w=0, offset_b=32 * 94 * 4 + 0,
                                                     bytes=32 * 94 * 4 + 256)
    lib = L.load()
    for n, w, c, cus in ((10, 48, 94, 256), (10, 288, 94, 256), (10, 0, 94, 256), (-1, 256, 94, 256), (10, 256, 0, 256), (10, 256, 257, 256), (10, 256, 94, 0)):
        out = L.EmdDeformMlpLayout()
        assert lib.emd_deform_mlp_workspace(n, w, c, cus, C.byref(out)) == L.EMD_ERR_INVALID
        assert b"deform_mlp_workspace" in lib.emd_last_error()


def test_entry_points_refuse_before_touching_the_device():
    """Every refusal that needs no device memory: decided on the host (this test runs without a GPU; the pointers are never dereferenced)."""
    lib = L.load()

    def args(**kw):
        a = L.EmdDeformMlpArgs()
        a.num_points, a.depth, a.width, a.in_dim, a.embed_dim, a.skip, a.ld_x, a.num_cus = 10, 8, 256, 94, 10, 4, 94, 256
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for kw, word in ((dict(width=48), b"multiple of 32"), (dict(width=288), b"multiple of 32"), (dict(depth=1), b"depth"), (dict(skip=7), b"concat"),
                     (dict(depth=2, skip=1), b"concat"), (dict(), b"null pointer"), (dict(ld_x=90), b"bad sizes"), (dict(embed_dim=40), b"bad sizes")):
        assert lib.emd_deform_mlp_forward(C.byref(args(**kw)), None) == L.EMD_ERR_INVALID
        assert word in lib.emd_last_error(), (kw, lib.emd_last_error())
        assert lib.emd_deform_mlp_backward(C.byref(args(**kw)), C.byref(L.EmdDeformMlpGrads()), None) == L.EMD_ERR_INVALID
    # nothing to do is not an error, whatever the pointers
    assert lib.emd_deform_mlp_forward(C.byref(args(num_points=0)), None) == 0
    assert lib.emd_deform_mlp_backward(C.byref(args(num_points=0)), None, None) == 0


def test_cpu_tensors_are_refused():
    from emd_amd.deformation import ConditionalDeformNetwork
    net = ConditionalDeformNetwork(D=4, W=32, embed_dim=4, fused=True)
    with pytest.raises(L.EmdError, match="no CPU path"):
        net.trunk(torch.zeros(3, net.input_ch))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_kink_share_of_the_reference_is_inside_its_cap(name):
    ref = R.reference(name)
    assert ref.kink_share <= R.kink_cap(ref.case.W), (name, ref.kink_share)


def _addmm_trunk(net, h0):
    """ConditionalDeformNetwork.trunk as it stands (fused=False), with torch.addmm where it calls tall_linear / tall_linear_relu."""
    h, skipped = h0, False
    for i, lin in enumerate(net.linear):
        if skipped:
            h = torch.relu(torch.addmm(torch.addmm(lin.bias, h0, lin.weight[:, :net.input_ch].t()), h, lin.weight[:, net.input_ch:].t()))
        else:
            h = torch.relu(torch.addmm(lin.bias, h, lin.weight.t()))
        skipped = i in net.skips
    out = lambda lin: torch.addmm(lin.bias, h, lin.weight.t())
    return (out(net.gaussian_warp), out(net.gaussian_rotation) if net.deform_quat else None, out(net.gaussian_scaling) if net.deform_scale else None)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_float32_formulation_meets_the_criterion(name):
    report = []
    worst = R.worst_ratio(name, _addmm_trunk, report=report)
    print(name, "worst error / bound:", worst, max(report, key=lambda p: p[1]))
    assert worst <= 1.0, report
