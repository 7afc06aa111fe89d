"""The inputs of tests/test_neighbour_std_gpu.py, built on the CPU from seeds so that tests/test_neighbour_std_cpu.py can assert the input
conditions (tests/neighbour_std_ref.py) on exactly what the GPU tests run: about 1 500 clustered points in the ten segments of
`neighbour_std_ref.segment_table`, the neighbour table of the contract (`segment_knn`, K - 1 others per point), the block sets of the class
(quaternions identity, log-scales exp, opacity logits sigmoid, SH dc and rest identity) and two single blocks.  Nothing here is written to after
`build` returns it."""
import functools

import torch

from tests import knn_checks as kc
from tests import neighbour_std_ref as R

N = 1500
KS = (2, 3, 4, 9)
CLASS_ACTS = ("identity", "exp", "sigmoid", "identity", "identity")
SETS = {"deg3": ((4, 3, 1, 3, 45), CLASS_ACTS), "deg1": ((4, 3, 1, 3, 9), CLASS_ACTS), "deg0": ((4, 3, 1, 3), CLASS_ACTS[:4]),
        "wide64": ((64,), ("identity",)), "one": ((1,), ("sigmoid",))}
WEIGHTS = (0.5, 1.0, 2.0, 0.25, 0.125)
G_TERMS = (1.5, -0.5, 2.0, 0.75, 1.25)            # the upstream scalars: not all ones, one negative

CASES = {f"K{K}-{s}": dict(K=K, set=s) for K in KS for s in SETS}
CASES["K3-zero-weights"] = dict(K=3, set="deg1", weights=(0.5, 0.0, 2.0, 0.0, 0.125))
CASES["K3-identical"] = dict(K=3, set="deg1", identical=(0, 2))         # SMPL Gaussians start with identical quaternions and opacities
CASES["K3-tight"] = dict(K=3, set="tight")
CASES["K9-tight"] = dict(K=9, set="tight")


@functools.lru_cache(maxsize=None)
def cloud():
    pts = kc.clustered_points(N, seed=41, clusters=6, copies=0)
    return pts, R.segment_table(N)


@functools.lru_cache(maxsize=None)
def table(K):
    pts, seg = cloud()
    return R.segment_knn(pts, seg, K - 1)[0]


def _values(cols, act, g):
    if cols == 4 and act == "identity":
        return torch.randn(N, 4, generator=g)                                  # unnormalised quaternions
    if act == "exp":
        return torch.randn(N, cols, generator=g) * 0.3 - 2.5                   # log-scales
    if act == "sigmoid":
        return torch.randn(N, cols, generator=g).clamp(-3, 3) + 0.5            # opacity logits
    if cols == 3:
        return torch.rand(N, 3, generator=g) * 2 - 1                           # SH dc
    return torch.randn(N, cols, generator=g) * 0.1                             # SH rest / a wide block


@functools.lru_cache(maxsize=None)
def build(name):
    spec = CASES[name]
    K = spec["K"]
    idx = table(K)
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    if spec["set"] == "tight":
        # sigma about 1.6e-5 max|v|: a shifted two-pass form is exact to a few ulps of sigma here, a sum-of-squares form is not
        blocks, acts = [(5.0 + 8e-5 * torch.randn(N, 4, generator=g)).float()], ("identity",)
        return dict(K=K, idx=idx, blocks=blocks, acts=acts, weights=(1.0,), g_terms=torch.tensor([1.5]), tight=True)
    cols, acts = SETS[spec["set"]]
    blocks = [_values(c, a, g) for c, a in zip(cols, acts)]
    for b in spec.get("identical", ()):
        blocks[b] = blocks[b][:1].expand(N, -1).contiguous()
    blocks = R.settle(blocks, idx, acts)
    if len(cols) == 5:
        blocks[4] = blocks[4].reshape(N, cols[4] // 3, 3)                       # _features_rest keeps its [N, M - 1, 3] shape
    weights = tuple(spec.get("weights", WEIGHTS[:len(cols)]))
    return dict(K=K, idx=idx, blocks=blocks, acts=acts, weights=weights, g_terms=torch.tensor(G_TERMS[:len(cols)]), tight=False)
