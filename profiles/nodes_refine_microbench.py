"""The refinement event of the actor classes and what its row order costs and saves, at 32 actors x 5 000 points (the bench scene's actors).

  (a) one event: `RigidNodes.refinement_after` grouped by actor and ungrouped, and -- block `baseline`, which uses nothing this event added and so
      runs on the parent commit as well -- `VanillaGaussians.refinement_after` on the same rows plus the torch restatement of the masks and the
      `cat` / indexing that carries the ids (what bolting refinement on without the event would do).  Host clock around the event, which ends in
      its own host read, then a device synchronise; every repetition starts from a fresh copy of the same store.
  (b) after ONE event that appends about 20 % rows: `TrackOffsetHeads.pose_table` forward + backward, the motion backward alone and
      dL/d instances_embedding alone, on the grouped layout and on the appended layout (the reference's order).  HIP events around each call.

Every block is written to the JSON as soon as it is measured (blocks of earlier runs are kept):
    python profiles/nodes_refine_microbench.py [--blocks baseline,event,layout] [--reps 30] [--out profiles/nodes_refine_microbench.json]
The committed JSON also holds `baseline_on_parent_commit`: this file copied into a checkout of the parent commit and run there as
    python profiles/nodes_refine_microbench.py --blocks baseline --baseline-name baseline_on_parent_commit --out <the same JSON>"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV, A, PER, F, E = "cuda:0", 32, 5000, 50, 4
CTRL = dict(sh_degree=3, warmup_steps=500, reset_alpha_interval=3000, refine_interval=100, n_split_samples=2, reset_alpha_value=0.01, densify_grad_thresh=0.0003,
            densify_size_thresh=0.025, cull_alpha_thresh=0.005, cull_scale_thresh=0.5, cull_screen_size=0.15, split_screen_size=0.05, stop_screen_size_at=4000,
            stop_split_at=15000, gaussian_embedding_dim=E, check_finite=False)
STEP, SCENE_SCALE = 3600, 2.0


def tensors(seed=0):
    """The rows of 32 actors, sorted by actor (the reference's initial layout).  12 % of the rows are above the gradient threshold; half of those are
    large (split into 2 samples), half small (duplicated): the event appends about 18 % rows, and culls the 2 % that are transparent."""
    g = torch.Generator().manual_seed(seed)
    N = A * PER
    t = dict(ids=torch.arange(N) // PER, size=torch.tensor([4.0, 2.0, 1.6]) * (0.8 + 0.4 * torch.rand(A, 1, generator=g)))
    t["means"] = (torch.rand(N, 3, generator=g) * 2 - 1) * 0.45 * t["size"][t["ids"]]
    large = torch.rand(N, generator=g) < 0.5
    t["log_scales"] = torch.log(torch.where(large, torch.tensor(0.12), torch.tensor(0.01)))[:, None] + torch.rand(N, 3, generator=g) * 0.5
    t["quats"], t["colors"] = torch.randn(N, 4, generator=g), torch.rand(N, 3, generator=g)
    t["opacity"] = torch.where(torch.rand(N, 1, generator=g) < 0.02, torch.tensor(-8.0), torch.tensor(2.0)) + torch.randn(N, 1, generator=g) * 0.1
    hot = torch.rand(N, generator=g) < 0.12
    t["grad_norm"] = torch.where(hot, torch.tensor(1e-3), torch.tensor(1e-5))
    t["iq"], t["it"], t["fv"] = torch.randn(F, A, 4, generator=g), torch.randn(F, A, 3, generator=g), torch.rand(F, A, generator=g) < 0.9
    t["emb"] = torch.randn(N, E, generator=g)
    return t


def store(cls, t, optimizer=True, **ctrl):
    from emd_amd.optim import Adam
    node = cls("Nodes", {**CTRL, **ctrl}, scene_scale=SCENE_SCALE, num_train_images=10, device=DEV)
    N = t["means"].shape[0]
    if hasattr(node, "point_ids"):
        node.create_from_tensors(t["means"], t["colors"], t["log_scales"], t["ids"], t["iq"], t["it"], t["size"], t["fv"], quats=t["quats"], embeddings=t["emb"])
    else:
        node.create_from_tensors(t["means"], t["colors"], t["log_scales"], quats=t["quats"])
    with torch.no_grad():
        node._opacities.copy_(t["opacity"].to(DEV))
    node.xys_grad_norm, node.vis_counts, node.max_2Dsize = t["grad_norm"].to(DEV), torch.ones(N, device=DEV), torch.zeros(N, device=DEV)
    node.preprocess_per_train_step(STEP)
    opt = None
    if optimizer:
        opt = Adam([{"params": v, "lr": 1e-3, "name": k} for k, v in node.get_param_groups().items()], lr=0.0, eps=1e-15)
        for grp in opt.param_groups:
            p = grp["params"][0]
            if p.shape[0] == N:
                opt.state[p] = {"step": torch.tensor(1.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.ones_like(p)}
    return node, opt


def stats(ts):
    ts = sorted(ts)
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4))


def host_timed(make, run, reps):
    ts, info = [], None
    for k in range(reps + 3):
        state = make()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = run(state)
        torch.cuda.synchronize()
        if k >= 3:
            ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts), info


def event_timed(fn, reps):
    ts = []
    for k in range(reps + 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= 5:
            ts.append(e0.elapsed_time(e1))
    return stats(ts)


def carry_ids_with_torch(ids, s, o, grad_norm, vis, m2d):
    """the masks of vanilla.py:218-326 restated with torch, only to carry the ids through `cat` and mask indexing"""
    c, ns = CTRL, CTRL["n_split_samples"]
    high = (grad_norm / vis) > c["densify_grad_thresh"]
    splits = ((torch.exp(s).max(dim=-1).values > c["densify_size_thresh"] * SCENE_SCALE) | (m2d > c["split_screen_size"])) & high
    s = torch.where(splits[:, None], torch.log(torch.exp(s) / 1.6), s)
    dups = (torch.exp(s).max(dim=-1).values <= c["densify_size_thresh"] * SCENE_SCALE) & high
    S_ = torch.cat([s, s[splits].repeat(ns, 1), s[dups]])
    O_ = torch.cat([o, o[splits].repeat(ns, 1), o[dups]])
    m2d = torch.cat([m2d, torch.zeros(S_.shape[0] - s.shape[0], device=s.device)])
    culls = (torch.sigmoid(O_).squeeze(-1) < c["cull_alpha_thresh"]) | (torch.exp(S_).max(dim=-1).values > c["cull_scale_thresh"] * SCENE_SCALE) | (m2d > c["cull_screen_size"])
    return torch.cat([ids, ids[splits].repeat(ns), ids[dups]])[~culls]


def block_baseline(t, reps):
    from emd_amd.vanilla import VanillaGaussians
    ids = t["ids"].to(DEV)

    def run(state):
        node, opt = state
        before = (node._scales.detach(), node._opacities.detach(), node.xys_grad_norm, node.vis_counts, node.max_2Dsize)
        info = node.refinement_after(STEP, opt)
        new_ids = carry_ids_with_torch(ids, *before)
        assert new_ids.shape[0] == node.num_points                      # (a host read the bolt-on makes as well: mask indexing)
        return info
    timing, info = host_timed(lambda: store(VanillaGaussians, t), run, reps)
    return dict(what="VanillaGaussians.refinement_after + torch masks / cat / indexing for the ids", rows_before=info["n_before"], rows_after=info["n_after"], **timing)


def block_event(t, reps):
    from emd_amd.nodes import RigidNodes
    out = {}
    for name, ctrl in (("grouped", dict(group_by_actor=True)), ("ungrouped", dict(group_by_actor=False)), ("grouped_with_box_cull", dict(group_by_actor=True, cull_out_of_bound=True))):
        timing, info = host_timed(lambda: store(RigidNodes, t, **ctrl), lambda s: s[0].refinement_after(STEP, s[1]), reps)
        out[name] = dict(rows_before=info["n_before"], rows_after=info["n_after"], **timing)
    return out


def block_layout(t, reps):
    from emd_amd.deformation import _DeformInput
    from emd_amd.motion import TrackOffsetHeads, build_actor_pose, transform_gaussians
    from emd_amd.nodes import RigidNodes
    out = {}
    g = torch.Generator().manual_seed(5)
    inst_emb = torch.randn(A, 10, generator=g).to(DEV).requires_grad_(True)
    for name, grouped in (("grouped", True), ("appended", False)):
        node, _ = store(RigidNodes, t, optimizer=False, group_by_actor=grouped)
        info = node.refinement_after(STEP, None)
        n, ids = node.num_points, node._ids_flat
        heads = TrackOffsetHeads(A, gaussian_embedding_dim=E).to(DEV)
        node.attach_track_heads(heads)
        if grouped:
            heads.adopt_layout(node._ids_flat, node.ids32, node.segment_start)
        res = dict(rows=n, appended_fraction=round(n / info["n_before"] - 1, 4), sorted_by_actor=bool((ids[1:] >= ids[:-1]).all()))

        def pose_fwd_bwd():
            node.instances_quats.grad = node.instances_trans.grad = node._embeddings.grad = None
            heads.pose_table(node.instances_quats, node.instances_trans, node.instances_fv, 3, node._embeddings, ids, STEP).sum().backward()
        res["pose_table_forward_backward"] = event_timed(pose_fwd_bwd, reps)
        res["one_launch_chain"] = heads._seg is not None
        pose = build_actor_pose(node.instances_quats, node.instances_trans, node.instances_fv, 3).detach().requires_grad_(True)
        wm, wq, wo = transform_gaussians(node._means, node._quats, torch.sigmoid(node._opacities), ids, pose)
        gm, gq, go = torch.randn_like(wm), torch.randn_like(wq), torch.randn_like(wo)
        res["motion_backward"] = event_timed(lambda: torch.autograd.grad((wm, wq, wo), (node._means, node._quats, pose), (gm, gq, go), retain_graph=True), reps)
        for det in (False, True):
            enc = _DeformInput.apply(node._means.detach(), node.ids32, node.instances_size, inst_emb, torch.full((1,), 0.3, device=DEV), 10, 10, det)
            ge = torch.randn_like(enc)
            res["instances_embedding_backward" + ("_deterministic" if det else "")] = event_timed(lambda: torch.autograd.grad(enc, inst_emb, ge, retain_graph=True), reps)
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="baseline,event,layout")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--baseline-name", default="baseline_on_this_commit", help="key of the `baseline` block (run in a checkout of the parent commit: baseline_on_parent_commit)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "nodes_refine_microbench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.update(actors=A, points_per_actor=PER, reps=a.reps, device=torch.cuda.get_device_name(0))
    t = tensors()
    for name in a.blocks.split(","):
        key = a.baseline_name if name == "baseline" else name
        res[key] = dict(baseline=block_baseline, event=block_event, layout=block_layout)[name](t, a.reps)
        json.dump(res, open(a.out, "w"), indent=1)
        print(json.dumps({key: res[key]}))


if __name__ == "__main__":
    main()
