"""Linear-blend skinning of SMPL nodes (csrc/skinning.hip) at 64 instances x 10 000 points (N = 640 k), SMPL parents, with canon_inv:
forward and backward of `joint_transforms` + `skin_gaussians`, the one-node form `posed_skin_gaussians`, and each of the four entry points on
its own, beside the yardstick -- the same contract in the reference's formulation (tests/skinning_ref.py: the Python loop over 24 joints of 4x4
products, the [N,24] x [N,24,16] blend, bmm, four quaternion candidates) in fp32 torch on the same GPU.

Clock: HIP events on the launch stream around ONE call (a forward, or a backward through a retained graph); `--warmup` untimed calls, then the
median of `--reps`.  Event pairs around a single small launch include the launch gap (a few microseconds): the chain kernels' figures are upper
bounds.  Bytes: what the algorithm has to move, from the shapes (below); the copy peak is a device-to-device `copy_` of 2 x 256 MiB timed the
same way.  The outputs of the timed code are compared with the yardstick's at this size before anything is timed.
    python profiles/skinning_microbench.py [--instances 64] [--points 10000] [--reps 50] [--out profiles/skinning_microbench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emd_amd import _lib as L  # noqa: E402
from emd_amd import smpl  # noqa: E402
from tests import skinning_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--points", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "skinning_microbench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("skinning_microbench needs a GPU: a CPU run gives no time")
    dev, P, N, J = "cuda:0", a.instances, a.instances * a.points, 24
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g)
    leaf = lambda t: t.to(dev).requires_grad_(True)
    theta, means, quats, opac = leaf(rn(P, J, 4)), leaf(0.5 * rn(N, 3)), leaf(rn(N, 4)), leaf(torch.rand(N, generator=g))
    w = torch.rand(N, J, generator=g) ** 4
    weights, trans = leaf(w / w.sum(-1, keepdim=True)), leaf(5 * rn(P, 3))
    joints = (0.3 * rn(P, J, 3)).to(dev)
    canon = torch.cat([R.quat_to_R(rn(P, J, 4)), 0.2 * rn(P, J, 3, 1)], -1).reshape(P, J, 12).to(dev)
    ids = torch.repeat_interleave(torch.arange(P), a.points).to(dev)
    valid = torch.ones(P, dtype=torch.bool, device=dev)
    gouts = [rn(N, 3).to(dev), rn(N, 4).to(dev), rn(N).to(dev)]
    leaves = [theta, means, quats, opac, weights, trans]
    lay = smpl.SkinLayout(P)

    def hip_two_nodes():
        return smpl.skin_gaussians(means, quats, opac, ids, weights, smpl.joint_transforms(theta, joints, smpl.SMPL_PARENTS, canon), trans, valid, layout=lay)

    def hip_one_node():
        return smpl.posed_skin_gaussians(means, quats, opac, ids, weights, theta, joints, trans, valid, smpl.SMPL_PARENTS, canon, layout=lay)

    def torch_ref():
        return R.skin(means, quats, opac, ids, weights, R.joint_chain(theta, joints, R.SMPL_PARENTS, canon), trans, valid)[:3]

    def timed(fn):
        ts = []
        for _ in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = sorted(ts[a.warmup:])
        return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4))

    def fwd_bwd(fn, inputs=leaves):
        outs = fn()
        back = lambda: torch.autograd.grad(outs, inputs, gouts, retain_graph=True)
        return dict(forward=timed(lambda: fn()), backward=timed(back)), outs, back()

    res = dict(instances=P, points_per_instance=a.points, num_points=N, reps=a.reps, warmup=a.warmup,
               clock="HIP events on the launch stream around one call; median of reps after warmup")
    r_two, o_hip, g_hip = fwd_bwd(hip_two_nodes)
    r_one, o_one, g_one = fwd_bwd(hip_one_node)
    r_ref, o_ref, g_ref = fwd_bwd(torch_ref)
    rel = lambda x, y: float((x.detach() - y.detach()).norm() / y.detach().norm().clamp_min(1e-30))
    res["relative_l2_vs_torch_fp32"] = dict(outputs=[round(rel(x, y), 9) for x, y in zip(o_hip, o_ref)],
                                            gradients=[round(rel(x, y), 9) for x, y in zip(g_hip, g_ref)])
    res["one_node_equals_two_nodes_bitwise"] = all(torch.equal(x, y) for x, y in zip(list(o_hip) + list(g_hip), list(o_one) + list(g_one)))
    no_w = [theta, means, quats, opac, trans]
    res["hip_joint_transforms_plus_skin_gaussians"] = r_two
    res["hip_posed_skin_gaussians"] = r_one
    res["hip_posed_skin_gaussians_no_weight_grad"] = fwd_bwd(hip_one_node, no_w)[0]["backward"]
    res["torch_fp32_reference_formulation"] = r_ref

    # the four entry points on their own
    lib, st = L.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pl = lay.prepare(ids)
    f = lambda t: t.detach().contiguous()
    A = torch.empty(P, J, 12, device=dev)
    ch = smpl._chain_args(f(theta), joints, smpl._parents_dev(smpl.SMPL_PARENTS, theta.device), canon, A)
    outs = (torch.empty(N, 3, device=dev), torch.empty(N, 4, device=dev), torch.empty(N, device=dev))
    vf = valid.float()
    sk = smpl._skin_args(f(means), f(quats), f(opac), f(weights), A, f(trans), vf, pl, outs)
    gr = L.EmdSkinGrads()
    d = [torch.empty(N, 3, device=dev), torch.empty(N, 4, device=dev), torch.empty(N, device=dev), torch.empty(N, J, device=dev),
         torch.empty(pl.num_chunks, L.SKIN_PARTIAL_FLOATS, device=dev)]
    gr.g_world_means, gr.g_world_quats, gr.g_opacities_out = (t.data_ptr() for t in gouts)
    gr.d_means, gr.d_quats, gr.d_opacities, gr.d_weights, gr.partials = (t.data_ptr() for t in d)
    d_theta, d_trans = torch.empty(P, J, 4, device=dev), torch.empty(P, 3, device=dev)
    kernels = dict(
        joint_chain_forward=lambda: L.check(lib.emd_joint_chain_forward(C.byref(ch), st), "chain fwd"),
        skin_forward=lambda: L.check(lib.emd_skin_forward(C.byref(sk), st), "skin fwd"),
        skin_backward=lambda: L.check(lib.emd_skin_backward(C.byref(sk), C.byref(gr), st), "skin bwd"),
        joint_chain_backward=lambda: L.check(lib.emd_joint_chain_backward(C.byref(ch), None, d[4].data_ptr(), pl.chunk_start.data_ptr(), None,
                                                                          d_trans.data_ptr(), d_theta.data_ptr(), st), "chain bwd"))
    res["entry_points"] = {k: timed(fn) for k, fn in kernels.items()}
    assert torch.equal(d_theta, g_one[0]) and torch.equal(d[3], g_one[4])

    # copy peak, and the bytes each skinning kernel has to move
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    cp = timed(lambda: dst.copy_(src))
    peak = 2 * src.numel() / (cp["median_ms"] * 1e-3)
    res["copy_peak"] = dict(bytes=2 * src.numel(), **cp, bytes_per_s=round(peak))
    table = P * J * 12 * 4
    fwd_bytes = N * (12 + 16 + 4 + 4 + 96) + N * (12 + 16 + 4) + table                      # means, quats, opacity, id, weights; the three outputs
    bwd_bytes = N * (12 + 16 + 4 + 96) + N * (12 + 16 + 4) + N * (12 + 16 + 4 + 96) + pl.num_chunks * (12 + L.SKIN_PARTIAL_FLOATS * 4) + table
    for k, nbytes in (("skin_forward", fwd_bytes), ("skin_backward", bwd_bytes)):
        t = res["entry_points"][k]["median_ms"] * 1e-3
        res["entry_points"][k].update(bytes=nbytes, bytes_per_s=round(nbytes / t), fraction_of_copy_peak=round(nbytes / t / peak, 3))
    res["chunks"] = pl.num_chunks
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
