"""-m gpu: the fused motion path (K1 / K8) with actor ids laid out in ways the bench scene does not use.

K8 sums the per-point actor-pose gradients of a wave that holds ONE actor id and adds the sum as one 12-lane row; a wave holding several
ids adds lane by lane.  Both layouts below must give the oracle's images and gradients, the actor-pose gradients included: ids shuffled
over the whole scene (most waves hold static points and several actors) and waves of 32 static points + 32 points of one actor."""
import numpy as np
import pytest
import torch

from tests.helpers import IMAGE_TOL, compare_backward, compare_forward, make_case, run_hip, run_oracle

pytestmark = pytest.mark.gpu


def _permuted(case, perm):
    n = case["N"]
    return {k: (v[perm].contiguous() if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == n else v) for k, v in case.items()}


def _layout(ids, kind, seed):
    n = ids.shape[0]
    if kind == "interleaved":
        return torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    # "mixed": each run of 64 points = 32 actor points in id order + 32 static points (so one actor per wave, a few waves excepted)
    dyn = torch.nonzero(ids >= 0).flatten()
    dyn = dyn[torch.argsort(ids[dyn], stable=True)]
    sta = torch.nonzero(ids < 0).flatten()
    parts = []
    for j in range(max(len(dyn), len(sta)) // 32 + 1):
        parts += [dyn[32 * j:32 * j + 32], sta[32 * j:32 * j + 32]]
    return torch.cat(parts)


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("kind", ["interleaved", "mixed"])
def test_actor_layout_matches_oracle(kind, residual):
    base = make_case(n=4000, H=64, W=96, seed=21, motion=True, residual=residual)
    perm = _layout(base["actor_ids"], kind, seed=5)
    assert torch.equal(torch.sort(perm).values, torch.arange(base["N"]))
    case = _permuted(base, perm)
    waves = case["actor_ids"][:64 * (case["N"] // 64)].view(-1, 64).numpy()
    n_ids = np.array([len(set(w[w >= 0].tolist())) for w in waves])
    assert (waves < 0).any(1).all()
    if kind == "interleaved":
        assert (n_ids >= 2).mean() > 0.9
    else:
        assert (n_ids == 1).mean() > 0.9
    orc = run_oracle(case, backward=True)
    hip = run_hip(case, backward=True)
    compare_forward(hip, orc, tol=IMAGE_TOL)
    checked = compare_backward(hip, orc)
    assert "actor_pose" in checked
    if residual:
        assert "residual_dx" in checked
