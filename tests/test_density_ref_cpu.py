"""-m "not gpu": tests/density_ref.py (the numpy restatement of the density-control contract that tests/test_density_index_gpu.py holds the
kernels to) against the reference programs' own order of operations written with torch mask indexing in float32:
  S3Gaussian   densify_and_clone, then densify_and_split with its prune_filter (scene/gaussian_model.py:532-603), and prune (:683-695)
  OmniRe       refinement_after: split -> in-place reduction -> duplicates decided after it -> cull of the grown arrays with max_2Dsize 0 on
               the new rows (models/gaussians/vanilla.py:206-326)
at N = 700 for every mode and all 32 refinement flag combinations; the built inputs keep the margin rule and reach every code a mode can
produce; the threshold-rounding case has its two thresholds, 1.0 as a product of floats and 0.99999994 as the reference forms it."""
import numpy as np
import pytest
import torch

from tests import density_ref as R

N = 700


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def torch_densify(inp, percent_dense, extent):
    """-> src, kind of the rows the reference ends with."""
    s, ga, den = _t(inp["scaling"]), _t(inp["grad_accum"])[:, None], _t(inp["denom"])[:, None]
    thr = float(inp["grad_threshold"])
    n = s.shape[0]
    grads = ga / den
    grads[grads.isnan()] = 0.0
    ids, kind = torch.arange(n), torch.zeros(n, dtype=torch.long)
    clone = (torch.norm(grads, dim=-1) >= thr) & (torch.exp(s).max(dim=1).values <= percent_dense * extent)
    ids, kind, s = torch.cat([ids, ids[clone]]), torch.cat([kind, torch.ones(int(clone.sum()), dtype=torch.long)]), torch.cat([s, s[clone]])
    padded = torch.zeros(ids.shape[0])
    padded[:n] = grads.squeeze()
    split = (padded >= thr) & (torch.exp(s).max(dim=1).values > percent_dense * extent)
    k = int(split.sum())
    ids = torch.cat([ids, ids[split].repeat(2)])
    kind = torch.cat([kind, torch.full((k,), 2), torch.full((k,), 3)])
    valid = ~torch.cat([split, torch.zeros(2 * k, dtype=torch.bool)])
    return ids[valid].numpy(), kind[valid].numpy()


def torch_prune(inp, extent):
    s, op, radii = _t(inp["scaling"]), _t(inp["opacity"])[:, None], _t(inp["max_radii2D"])
    mask = (torch.sigmoid(op) < float(inp["min_opacity"])).squeeze(-1)
    if float(inp["max_screen_size"]):
        mask = mask | (radii > float(inp["max_screen_size"])) | (torch.exp(s).max(dim=1).values > 0.1 * extent)
    if inp["extra_drop"] is not None:
        mask = mask | _t(inp["extra_drop"]).bool()
    return torch.arange(s.shape[0])[~mask].numpy()


def torch_refine(inp, flags, ns):
    """-> src, kind, split_rank of the rows the reference ends with."""
    do_densify, do_cull, use_split_screen, cull_big, use_cull_screen = flags
    t = {k: float(v) for k, v in inp["thr"].items()}
    s, o, m2d = _t(inp["scaling"]).clone(), _t(inp["opacity"])[:, None], _t(inp["max_2Dsize"])
    n = s.shape[0]
    ids, rank = torch.arange(n), torch.zeros(n, dtype=torch.long)
    is_split = torch.zeros(n, dtype=torch.bool)
    kind = torch.zeros(n, dtype=torch.long)
    if do_densify:
        high = (_t(inp["grad_norm"]) / _t(inp["vis_counts"])) > t["grad_threshold"]
        splits = torch.exp(s).max(dim=-1).values > t["size_threshold"]
        if use_split_screen:
            splits = splits | (m2d > t["split_screen"])
        splits = splits & high
        k = int(splits.sum())
        new_s = torch.log(torch.exp(s[splits]) / 1.6).repeat(ns, 1)
        s[splits] = torch.log(torch.exp(s[splits]) / 1.6)
        dups = (torch.exp(s).max(dim=-1).values <= t["size_threshold"]) & high
        d = int(dups.sum())
        is_split = splits
        ids = torch.cat([ids, ids[splits].repeat(ns), ids[dups]])
        kind = torch.cat([16 * splits.long(), torch.cat([torch.full((k,), 2 + r + 16) for r in range(ns)]), 1 + 16 * splits[dups].long()])
        rank = torch.cat([rank, torch.arange(k).repeat(ns), torch.zeros(d, dtype=torch.long)])
        s, o = torch.cat([s, new_s, s[dups]]), torch.cat([o, o[splits].repeat(ns, 1), o[dups]])
        m2d = torch.cat([m2d, torch.zeros(ns * k + d)])
    if do_cull:
        culls = (torch.sigmoid(o) < t["cull_alpha"]).squeeze(-1)
        if cull_big:
            culls = culls | (torch.exp(s).max(dim=-1).values > t["cull_size"])
            if use_cull_screen:
                culls = culls | (m2d > t["cull_screen"])
        ids, kind, rank = ids[~culls], kind[~culls], rank[~culls]
    return ids.numpy(), kind.numpy(), rank.numpy(), is_split.numpy()


@pytest.mark.parametrize("grad_threshold", [R.GRAD_THRESHOLD, 0.0])
def test_densify_reference_matches_the_reference_program(grad_threshold):
    inp = R.build_densify(N, 1, grad_threshold)
    assert R.margins_hold(inp, "densify") and len(inp["hand"]) == 7
    code = R.decide_densify(inp["scaling"], inp["grad_accum"], inp["denom"], inp["grad_threshold"], inp["size_threshold"])
    assert set(code.tolist()) == ({R.KEEP, R.KEEP | R.CLONE, R.SPLIT} if grad_threshold else {R.KEEP | R.CLONE, R.SPLIT})
    want = [3, 4, 1, 1, 4, 3, 1] if grad_threshold else [3, 4, 4, 4, 4, 3, 3]          # the hand rows; at threshold 0 every row is hot, 0/0 included
    assert code[inp["hand"]].tolist() == want
    src, kind = R.index_densify(code)
    t_src, t_kind = torch_densify(inp, R.PERCENT_DENSE, R.EXTENT)
    np.testing.assert_array_equal(src, t_src)
    np.testing.assert_array_equal(kind, t_kind)
    counts = R.block_counts(code, 3)
    offsets, totals = R.exclusive_offsets(counts)
    assert counts.shape == (3, 3) and totals.tolist() == [int((kind == 0).sum()), int((kind == 1).sum()), int((kind == 2).sum())]
    assert offsets[:, 0].tolist() == [0, 0, 0] and (offsets[:, -1] + counts[:, -1] == totals).all()
    rank = R.split_rank_densify(len(src), *totals.tolist())
    split_rows = np.flatnonzero(code & R.SPLIT)
    np.testing.assert_array_equal(split_rows[rank[kind >= 2]], src[kind >= 2])          # the rank names the source among the split rows
    assert (rank[kind < 2] == 0).all()


@pytest.mark.parametrize("screen,extra,min_opacity", [(True, False, R.MIN_OPACITY), (False, False, R.MIN_OPACITY), (True, True, R.MIN_OPACITY),
                                                      (False, True, -1.0)])
def test_prune_reference_matches_the_reference_program(screen, extra, min_opacity):
    inp = R.build_prune(N, 2, screen, extra, min_opacity)
    assert R.margins_hold(inp, "prune") and len(inp["hand"]) == 7
    code = R.decide_prune(inp["scaling"], inp["opacity"], inp["max_radii2D"], inp["extra_drop"], inp["min_opacity"], inp["max_screen_size"],
                          inp["size_threshold"])
    assert set(code.tolist()) == {0, R.KEEP}
    want = [1, 0 if screen else 1, 0 if screen else 1, 0 if extra else 1, 0 if extra else 1, 1, 1 if min_opacity < 0 else 0]
    assert code[inp["hand"]].tolist() == want
    src, kind = R.index_densify(code)
    np.testing.assert_array_equal(src, torch_prune(inp, R.EXTENT))
    assert (kind == 0).all()


@pytest.mark.parametrize("cull_screen", [None, -0.125])
def test_refine_reference_matches_the_reference_program_in_all_flag_combinations(cull_screen):
    inp = R.build_refine(N, 3, cull_screen)
    assert R.margins_hold(inp, "refine") and len(inp["hand"]) == 9
    seen = set()
    for flags in R.ALL_REFINE_FLAGS:
        code = R.decide_refine(flags, inp["scaling"], inp["opacity"], inp["grad_norm"], inp["vis_counts"], inp["max_2Dsize"], inp["thr"])
        assert set(code.tolist()) == R.refine_codes_possible(flags, inp["thr"]), flags
        seen |= set(code.tolist())
        assert not ((code & R.R_SAMPLES != 0) & (code & R.R_SPLIT == 0)).any()          # samples only of a split source
        for ns in (1, 2, 3):
            src, kind, rank = R.index_refine(code, ns)
            t_src, t_kind, t_rank, t_split = torch_refine(inp, flags, ns)
            np.testing.assert_array_equal(src, t_src, err_msg=str(flags))
            np.testing.assert_array_equal(kind, t_kind, err_msg=str(flags))
            np.testing.assert_array_equal(rank, t_rank, err_msg=str(flags))
            np.testing.assert_array_equal((code & R.R_SPLIT) != 0, t_split, err_msg=str(flags))
        counts = R.block_counts(code, 4)
        _, totals = R.exclusive_offsets(counts)
        assert len(src) == totals[0] + 3 * totals[2] + totals[1]
    if cull_screen is None:
        # the hand rows with everything on: quotient == threshold stays unsplit; the float above splits; 0/0 is not high; x/0 duplicates; just above
        # the size threshold: split AND duplicated; max_2Dsize == split_screen: duplicated, not split; == cull_screen: stays; transparent: split and gone
        code = R.decide_refine((1, 1, 1, 1, 1), inp["scaling"], inp["opacity"], inp["grad_norm"], inp["vis_counts"], inp["max_2Dsize"], inp["thr"])
        assert code[inp["hand"]].tolist() == [1, 13, 1, 3, 15, 3, 13, 8, 1]
        assert seen >= {0, 1, 3, 8, 12, 13, 15}
    else:
        # a negative cull_screen culls every new row (their max_2Dsize 0 exceeds it) and every original above it; the original that sits ON it stays
        # while its samples go: keep | split, a code no other setting produces
        code = R.decide_refine((1, 1, 1, 1, 1), inp["scaling"], inp["opacity"], inp["grad_norm"], inp["vis_counts"], inp["max_2Dsize"], inp["thr"])
        assert (code & 6 == 0).all() and (code[np.asarray(inp["max_2Dsize"]) > -0.125] & 1 == 0).all() and code[inp["hand"][6]] == R.R_KEEP | R.R_SPLIT


def test_index_reference_on_a_hand_written_code():
    src, kind = R.index_densify(np.array([1, 3, 4, 0, 4, 1]))
    assert src.tolist() == [0, 1, 5, 1, 2, 4, 2, 4] and kind.tolist() == [0, 0, 0, 1, 2, 2, 3, 3]
    assert R.split_rank_densify(8, 3, 1, 2).tolist() == [0, 0, 0, 0, 0, 1, 0, 1] and R.split_rank_densify(3, 2, 1, 0).tolist() == [0, 0, 0]
    # keep; split with samples, original culled; split, samples culled, duplicate kept; duplicate of an unsplit row; nothing
    src, kind, rank = R.index_refine(np.array([1, 12, 8 | 2 | 1, 3, 0, 13]), 2)
    assert src.tolist() == [0, 2, 3, 5, 1, 5, 1, 5, 2, 3]
    assert kind.tolist() == [0, 16, 0, 16, 18, 18, 19, 19, 17, 1]
    assert rank.tolist() == [0, 0, 0, 0, 0, 2, 0, 2, 0, 0]
    counts = R.block_counts(np.r_[np.ones(300, int), 4 * np.ones(300, int)], 3)
    assert counts.tolist() == [[256, 44, 0], [0, 0, 0], [0, 212, 88]]
    offsets, totals = R.exclusive_offsets(counts)
    assert offsets.tolist() == [[0, 256, 300], [0, 0, 0], [0, 0, 212]] and totals.tolist() == [300, 0, 300]


def test_margin_mover_moves_rows_and_drops_none():
    thr = float(R.f32_product(R.PERCENT_DENSE, R.EXTENT))
    s = np.full((5, 3), np.log(thr), np.float32)
    s[:, 1:] -= 1.0
    s[3] += np.float32(np.log(1.6))
    s[4, 0] = -9.0
    before = s.copy()
    R._clear_scales(s, R.scale_thresholds(thr))
    assert s.shape == before.shape and (s[:4] > before[:4]).all() and (s[4] == before[4]).all()
    assert (np.abs(R.max_scale(s)[:, None] / np.array(R.scale_thresholds(thr)) - 1.0) >= R.MARGIN).all()
    assert (s[:4] - before[:4]).max() < 0.01


def test_threshold_rounding_case():
    """percent_dense = 0.001 and extent = 999.9999389648438: the product of the two floats is 1.0, the reference's double product rounds to the
    float below it -- a Gaussian with max exp(scale) == 1.0 is split by the reference and would be cloned under the device product."""
    pd, extent = 0.001, 999.9999389648438
    assert float(np.float32(extent)) == extent
    device_product = np.float32(pd) * np.float32(extent)
    assert device_product == np.float32(1.0) and R.f32_product(pd, extent) == np.nextafter(np.float32(1.0), np.float32(0)) == np.float32(0.99999994)
    scaling = np.array([[0, 0, 0], [0, -1, -2], [-3, 0, -1]], np.float32)
    assert (R.max_scale(scaling) == 1.0).all()
    ones = np.ones(3, np.float32)
    assert R.decide_densify(scaling, ones, ones, R.GRAD_THRESHOLD, R.f32_product(pd, extent)).tolist() == [R.SPLIT] * 3
    assert R.decide_densify(scaling, ones, ones, R.GRAD_THRESHOLD, device_product).tolist() == [R.KEEP | R.CLONE] * 3
