"""Analysis tool (test infrastructure, not product): how many visible Gaussians of the bench scene the render backward reaches, on the CPU oracle.
    python -m tests.analysis.contributing_share [frame] [n]

Runs the oracle's forward and render backward on bench.py's scene (2 M Gaussians, 32 actors, 1066 x 1600, camera 0) with a loss gradient that is
non-zero at every pixel, and counts the radii > 0 Gaussians whose accumulated render gradient (mean2D, conic, opacity, rgb, depth) is zero in
every component: the Gaussians the projection backward writes zero rows for instead of running its chain rule (the contributed words of geom_ws;
DESIGN.md section 6.2).  No GPU."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def contributing(render_grads, n):
    """bool [n]: some component of the Gaussian's render gradient is non-zero."""
    return np.concatenate([np.asarray(render_grads[k]).reshape(n, -1) for k in ("mean2D", "conic", "opacity", "rgb", "depth")], 1).any(1)


def main(frame=10, n=2_000_000):
    from oracle import cpu_oracle as co
    from tests.test_parity_gpu import _bench_scene_case
    from tests.helpers import oracle_settings, oracle_scene
    case, sc = _bench_scene_case(n, frame=frame, actors=True)
    case["scales"], case["opacities"] = torch.exp(sc.log_scales), torch.sigmoid(sc.opacity_logits)
    case["rotations"] = torch.nn.functional.normalize(sc.quats, dim=1)
    assert all((case[k] != 0).all() for k in ("dL_dcolor", "dL_ddepth", "dL_dalpha"))
    S, scene = oracle_settings(case), oracle_scene(case)
    pre, b, img = co.forward(S, scene, case["flags"])
    g = co.render_backward(S, scene, pre, b, img, case["dL_dcolor"], case["dL_ddepth"], case["dL_dalpha"], None, case["flags"])
    vis = pre["radii"] > 0
    c = contributing(g, n) & vis
    V, K = int(vis.sum()), int(c.sum())
    print(f"frame {frame}  N {n}  visible (radii > 0) {V}  contributing {K}  share with an all-zero row {1.0 - K / max(V, 1):.3f}")
    blocks = np.add.reduceat(c.astype(np.int64), np.arange(0, n, 256))
    vblocks = np.add.reduceat(vis.astype(np.int64), np.arange(0, n, 256))
    print(f"per 256-block of the projection backward: {vblocks.mean() / 64:.2f} waves of visible Gaussians, {blocks.mean() / 64:.2f} waves of contributing ones")
    return V, K


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10, int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000)
