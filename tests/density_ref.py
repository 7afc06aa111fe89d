"""The density-control chain decide -> scan -> index (csrc/densify.hip) restated from the contract in include/emd_raster.h (EmdDensifyArgs,
EmdRefineArgs, emd_densify_index / emd_refine_index) in numpy float64, and the inputs its tests run on.  No GPU, no torch.

Arithmetic of the reference programs that the restatement keeps: the statistics' quotients (xyz_gradient_accum / denom, xys_grad_norm / vis_counts)
are float32 divisions, as torch performs them; every threshold is a float32 (torch rounds a Python scalar to the tensor's type once), a product
such as percent_dense * extent being formed in double first (`f32_product`); exp, log and the sigmoid are evaluated in float64.

Margin rule of the builders: whatever the kernels compare after expf, logf or a sigmoid keeps a relative distance of at least MARGIN from its
threshold in float64 -- max exp(scale) against the size thresholds, the reduced scale max exp(scale) / 1.6 against the two refinement thresholds,
the opacity against min_opacity / cull_alpha.  A drawn row inside the margin is MOVED (log-scales / logit / numerator nudged by 1e-3, far more
than the margin, far less than the spread of the draw), never dropped.  MARGIN is a condition on the inputs, not a measured tolerance: the
float32 chains involved (up to exp(log(exp(l) / 1.6))) accumulate well under 1e-6.  Rows that sit EXACTLY on a threshold are placed by hand and
only where the compared value reaches the kernel without a transcendental function (the `rows` of each builder)."""
import numpy as np

KEEP, CLONE, SPLIT = 1, 2, 4                        # densify / prune codes; a dropped row is 0
R_KEEP, R_DUP, R_SAMPLES, R_SPLIT = 1, 2, 4, 8      # refinement codes
BLOCK = 256
MARGIN = 1e-5
REDUCE = 1.6                                        # a split row's scale is divided by 0.8 * 2
F32 = np.float32


def f32_product(a, b):
    """A threshold the reference forms as a Python product: multiplied in double, rounded to float32 once."""
    return F32(float(a) * float(b))


def _quotient(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(num, F32) / np.asarray(den, F32)


def max_scale(scaling):
    return np.exp(np.asarray(scaling, np.float64)).max(axis=1)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


# ---- decisions ---------------------------------------------------------------------------------------------------------------------------------
def decide_densify(scaling, grad_accum, denom, grad_threshold, size_threshold):
    """keep 1 | clone 2 where hot and small; split 4 (alone: the original leaves) where hot and large.  hot: grad_accum / denom (NaN -> 0) >=
    grad_threshold; small: max exp(scale) <= size_threshold (= f32_product(percent_dense, extent))."""
    g = _quotient(grad_accum, denom)
    g = np.where(np.isnan(g), F32(0), g)
    hot = g >= F32(grad_threshold)
    small = max_scale(scaling) <= float(F32(size_threshold))
    return np.where(hot & ~small, SPLIT, np.where(hot & small, KEEP | CLONE, KEEP)).astype(np.int32)


def decide_prune(scaling, opacity, max_radii2D, extra_drop, min_opacity, max_screen_size, size_threshold):
    """0 where sigmoid(opacity) < min_opacity, or -- with max_screen_size > 0 -- max_radii2D > max_screen_size or max exp(scale) > size_threshold
    (= f32_product(0.1, extent)), or extra_drop != 0; keep 1 otherwise."""
    drop = sigmoid(opacity) < float(F32(min_opacity))
    if float(F32(max_screen_size)) > 0:
        drop = drop | (np.asarray(max_radii2D, F32) > F32(max_screen_size)) | (max_scale(scaling) > float(F32(size_threshold)))
    if extra_drop is not None:
        drop = drop | (np.asarray(extra_drop) != 0)
    return np.where(drop, 0, KEEP).astype(np.int32)


def decide_refine(flags, scaling, opacity, grad_norm, vis_counts, max_2Dsize, thr):
    """flags: (do_densify, do_cull, use_split_screen, cull_big, use_cull_screen); thr: dict of the six float32 thresholds of EmdRefineArgs."""
    do_densify, do_cull, use_split_screen, cull_big, use_cull_screen = (bool(f) for f in flags)
    t = {k: float(F32(v)) for k, v in thr.items()}
    n = len(scaling)
    smax = max_scale(scaling)
    m2d = np.asarray(max_2Dsize, F32)
    split = np.zeros(n, bool)
    dup = np.zeros(n, bool)
    if do_densify:
        high = _quotient(grad_norm, vis_counts) > F32(thr["grad_threshold"])          # NaN compares false
        split = smax > t["size_threshold"]
        if use_split_screen:
            split = split | (m2d > F32(thr["split_screen"]))
        split = split & high
        smax = np.where(split, smax / REDUCE, smax)          # the original is reduced in place before the duplicates are chosen
        dup = (smax <= t["size_threshold"]) & high
    keep, samples = np.ones(n, bool), split.copy()
    if do_cull:
        gone = sigmoid(opacity) < t["cull_alpha"]
        if cull_big:
            gone = gone | (smax > t["cull_size"])            # the same (possibly reduced) scale on the original, its samples and its duplicate
        screen = cull_big and use_cull_screen
        keep = ~(gone | (screen & (m2d > F32(thr["cull_screen"]))))
        new_gone = gone | (screen and 0.0 > t["cull_screen"])          # new rows carry max_2Dsize 0
        samples, dup = split & ~new_gone, dup & ~new_gone
    return (keep * R_KEEP + dup * R_DUP + samples * R_SAMPLES + split * R_SPLIT).astype(np.int32)


# ---- counts, offsets, index ----------------------------------------------------------------------------------------------------------------------
def block_counts(code, cols):
    """[cols, ceil(N / 256)]: per 256-row block the number of rows whose code has bit c."""
    code = np.asarray(code, np.int64)
    nb = (len(code) + BLOCK - 1) // BLOCK
    padded = np.zeros(nb * BLOCK, np.int64)
    padded[:len(code)] = code
    return np.stack([((padded >> c) & 1).reshape(nb, BLOCK).sum(axis=1) for c in range(cols)]).astype(np.int32)


def exclusive_offsets(counts):
    counts = np.asarray(counts, np.int64)
    inc = np.cumsum(counts, axis=-1)
    return (inc - counts).astype(np.int32), counts.sum(axis=-1).astype(np.int32)


def index_densify(code):
    """-> src, kind: survivors in row order (0), clones (1), split replica 0 (2), replica 1 (3)."""
    code = np.asarray(code)
    keep, clone, split = (np.flatnonzero(code & b) for b in (KEEP, CLONE, SPLIT))
    src = np.concatenate([keep, clone, split, split]).astype(np.int32)
    kind = np.concatenate([np.full(len(keep), 0), np.full(len(clone), 1), np.full(len(split), 2), np.full(len(split), 3)]).astype(np.int32)
    return src, kind


def index_refine(code, num_samples):
    """-> src, kind, split_rank: originals (0), samples of replica 0 .. num_samples - 1 (2 + r), duplicates (1); + 16 where the source is split;
    split_rank: the source's rank among ALL split sources on sample rows, 0 elsewhere."""
    code = np.asarray(code)
    keep, dup, samp = (np.flatnonzero(code & b) for b in (R_KEEP, R_DUP, R_SAMPLES))
    is_split = (code & R_SPLIT) != 0
    rank = np.cumsum(is_split) - is_split
    sp = 16 * is_split
    src = np.concatenate([keep] + [samp] * num_samples + [dup]).astype(np.int32)
    kind = np.concatenate([sp[keep]] + [(2 + r) | sp[samp] for r in range(num_samples)] + [1 | sp[dup]]).astype(np.int32)
    split_rank = np.concatenate([np.zeros(len(keep))] + [rank[samp]] * num_samples + [np.zeros(len(dup))]).astype(np.int32)
    return src, kind, split_rank


def split_rank_densify(num_out, n_keep, n_clone, n_split):
    j = np.arange(num_out)
    base = n_keep + n_clone
    return np.where(j < base, 0, (j - base) % max(n_split, 1)).astype(np.int32)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
# Every product below is exact in float32 and in double alike (powers of two), so the builders' cases do not depend on where a threshold is rounded.
GRAD_THRESHOLD = 2.0 ** -12
PERCENT_DENSE, EXTENT = 0.0078125, 4.0                   # size threshold 2^-5
MIN_OPACITY, MAX_SCREEN_SIZE = 0.0078125, 20.0
REFINE_THR = dict(grad_threshold=2.0 ** -12, size_threshold=0.0078125 * 4.0, split_screen=0.0625, cull_alpha=0.0078125, cull_size=0.0625 * 4.0,
                  cull_screen=0.125)
NUDGE = 1e-3


def _near(value, thresholds):
    value = np.asarray(value, np.float64)
    near = np.zeros(value.shape, bool)
    for t in thresholds:
        if t != 0 and np.isfinite(t):
            near |= np.abs(value / t - 1.0) < MARGIN
    return near


def _clear_scales(scaling, thresholds):
    """Raise all three log-scales of a row by NUDGE until its max scale has left the margin of every threshold."""
    for _ in range(64):
        near = _near(max_scale(scaling), thresholds)
        if not near.any():
            return scaling
        scaling[near] += F32(NUDGE)
    raise AssertionError("a scale row does not leave the margin")


def _clear_logits(logit, thresholds):
    for _ in range(64):
        near = _near(sigmoid(logit), thresholds)
        if not near.any():
            return logit
        logit[near] += F32(NUDGE)
    raise AssertionError("a logit does not leave the margin")


def _clear_quotients(num, den, threshold):
    for _ in range(64):
        q = _quotient(num, den).astype(np.float64)
        near = np.isfinite(q) & _near(np.where(np.isfinite(q), q, 0.0), [threshold])
        if not near.any():
            return num
        num[near] *= F32(1.0 + NUDGE)
    raise AssertionError("a quotient does not leave the margin")


def scale_thresholds(*thresholds):
    """The values max exp(scale) must stay clear of: each threshold, and 1.6 times it (the reduced scale against the same threshold)."""
    return [float(F32(t)) * f for t in thresholds for f in (1.0, float(F32(REDUCE)))]


def _hand_positions(n, count):
    """Where the hand-placed rows go: spread over the rows (lane 0 of the first block included); the first min(n, count) of them when n is small."""
    stride = max(n // max(count, 1), 1)
    return [k * stride for k in range(count) if k * stride < n]


def _scale_row(log_max, where):
    row = [log_max - 1.0, log_max - 2.0, log_max - 0.5]
    row[where] = log_max
    return row


def build_densify(n, seed, grad_threshold=GRAD_THRESHOLD):
    """-> dict(scaling [n,3], grad_accum [n], denom [n], grad_threshold, size_threshold, hand = rows placed by hand).  Drawn rows: about a tenth
    with denom 0, a tenth with grad_accum 0 (so 0/0 and x/0 both occur); the numerators are sums of norms, never negative (the reference takes
    torch.norm of the quotient for one mask and the quotient itself for the other), so with grad_threshold == 0 every row is hot, 0/0 included.
    Hand rows: quotient == threshold (small and large Gaussian), the float below the threshold, 0/0, x/0 small and large, 0/x."""
    rng = np.random.default_rng(seed)
    thr = f32_product(PERCENT_DENSE, EXTENT)
    scaling = (np.log(float(thr)) + rng.uniform(-3.0, 3.0, (n, 3))).astype(F32)
    denom = rng.integers(0, 5, n).astype(F32)
    denom[rng.random(n) < 0.1] = 0
    gt = F32(grad_threshold)
    spread = float(gt) if gt > 0 else GRAD_THRESHOLD
    grad_accum = (rng.uniform(0.0, 2.0 * spread, n) * np.maximum(denom, 1)).astype(F32)
    grad_accum[rng.random(n) < 0.1] = 0
    _clear_scales(scaling, [float(thr)])
    _clear_quotients(grad_accum, denom, float(gt))
    small, large = np.log(float(thr)) - 1.0, np.log(float(thr)) + 1.0
    below = np.nextafter(gt, F32(-1)) if gt > 0 else F32(0)
    rows = [(_scale_row(small, 0), 2 * gt, 2),            # == threshold: hot (>=), small -> keep | clone
            (_scale_row(large, 1), 3 * gt, 3),            # == threshold, large -> split
            (_scale_row(large, 2), below, 1),             # one float below: not hot   (0/1, hot, when the threshold is 0)
            (_scale_row(large, 0), 0, 0),                 # 0/0 -> NaN -> 0: hot only where the threshold is 0
            (_scale_row(large, 1), 1, 0),                 # x/0 -> inf: hot, large
            (_scale_row(small, 2), gt, 0),                # x/0 -> inf: hot, small   (0/0 when the threshold is 0)
            (_scale_row(small, 0), 0, 2)]                 # 0/x: hot only where the threshold is 0
    hand = _hand_positions(n, len(rows))
    for i, (s, ga, de) in zip(hand, rows):
        scaling[i], grad_accum[i], denom[i] = s, ga, de
    return dict(scaling=scaling, grad_accum=grad_accum, denom=denom, grad_threshold=gt, size_threshold=thr, hand=hand)


def build_prune(n, seed, screen=True, extra=False, min_opacity=MIN_OPACITY):
    """-> dict(scaling, opacity, max_radii2D, extra_drop or None, min_opacity, max_screen_size, size_threshold, hand).  max_radii2D are whole numbers
    0 .. 40 (equality with max_screen_size = 20 occurs in the draw as well).  Hand rows: radius == max_screen_size, the float above it, a huge and
    wide Gaussian (dropped only while the size tests are on), extra_drop bytes 1 and 255 on rows that would stay, 0 on one that stays."""
    rng = np.random.default_rng(seed)
    thr = f32_product(0.1, EXTENT)
    mss = F32(MAX_SCREEN_SIZE if screen else 0.0)
    scaling = (np.log(float(thr)) + rng.uniform(-3.0, 1.0, (n, 3))).astype(F32)
    opacity = (rng.normal(size=n) * 3.0 - 2.0).astype(F32)
    radii = rng.integers(0, 41, n).astype(F32)
    extra_drop = None
    if extra:
        extra_drop = np.where(rng.random(n) < 0.2, rng.choice(np.array([1, 7, 255], np.uint8), n), 0).astype(np.uint8)
    _clear_scales(scaling, [float(thr)])
    _clear_logits(opacity, [float(F32(min_opacity))])
    small = np.log(float(thr)) - 1.0
    rows = [(_scale_row(small, 0), 3.0, MAX_SCREEN_SIZE, 0),                                        # == max_screen_size: stays (>)
            (_scale_row(small, 1), 3.0, np.nextafter(F32(MAX_SCREEN_SIZE), F32(np.inf)), 0),          # the float above: dropped while the tests are on
            (_scale_row(10.0, 2), 3.0, 1e6, 0),                                                      # huge and wide
            (_scale_row(small, 2), 3.0, 1.0, 1),
            (_scale_row(small, 0), 3.0, 1.0, 255),
            (_scale_row(small, 1), 3.0, 1.0, 0),
            (_scale_row(small, 2), -9.0, 1.0, 0)]                                                    # transparent: dropped unless min_opacity < 0
    hand = _hand_positions(n, len(rows))
    for i, (s, op, r, x) in zip(hand, rows):
        scaling[i], opacity[i], radii[i] = s, op, r
        if extra_drop is not None:
            extra_drop[i] = x
    return dict(scaling=scaling, opacity=opacity, max_radii2D=radii, extra_drop=extra_drop, min_opacity=F32(min_opacity), max_screen_size=mss,
                size_threshold=thr, hand=hand)


def build_refine(n, seed, cull_screen=None):
    """-> dict(scaling, opacity, grad_norm, vis_counts, max_2Dsize, thr, hand); the same inputs serve all 32 flag combinations.  max_2Dsize are
    multiples of 1/64 in 0 .. 0.25 (equality with split_screen = 4/64 and cull_screen = 8/64 occurs in the draw as well).  Hand rows: quotient
    == threshold (not high: >), the float above it, 0/0, x/0, a Gaussian just above the size threshold (split AND duplicated), max_2Dsize ==
    split_screen and == cull_screen."""
    rng = np.random.default_rng(seed)
    thr = {k: F32(v) for k, v in REFINE_THR.items()}
    if cull_screen is not None:
        thr["cull_screen"] = F32(cull_screen)
    size = float(thr["size_threshold"])
    scaling = (np.log(size) + rng.uniform(-3.0, 3.5, (n, 3))).astype(F32)
    opacity = (rng.normal(size=n) * 3.0 - 2.0).astype(F32)
    vis = rng.integers(0, 4, n).astype(F32)
    gt = thr["grad_threshold"]
    grad_norm = (rng.uniform(0.0, 2.0 * float(gt), n) * np.maximum(vis, 1)).astype(F32)
    grad_norm[rng.random(n) < 0.1] = 0
    m2d = (rng.integers(0, 17, n) / 64.0).astype(F32)
    _clear_scales(scaling, scale_thresholds(thr["size_threshold"], thr["cull_size"]))
    _clear_logits(opacity, [float(thr["cull_alpha"])])
    _clear_quotients(grad_norm, vis, float(gt))
    small, above, large = np.log(size) - 1.0, np.log(size) + 0.2, np.log(size) + 1.0
    over = np.nextafter(gt, F32(1))
    rows = [(_scale_row(large, 0), 3.0, 2 * gt, 2, 0.0),                        # == threshold: not high
            (_scale_row(large, 1), 3.0, over, 1, 0.0),                          # the float above: high, large -> split
            (_scale_row(large, 2), 3.0, 0, 0, 0.0),                             # 0/0 -> NaN: not high
            (_scale_row(small, 0), 3.0, 1, 0, 0.0),                             # x/0 -> inf: high, small -> duplicate
            (_scale_row(above, 1), 3.0, 4 * gt, 1, 0.0),                        # just above the size threshold: split, reduced below it, duplicated
            (_scale_row(small, 2), 3.0, 4 * gt, 1, REFINE_THR["split_screen"]),  # == split_screen: not split on its screen size
            (_scale_row(large, 0), 3.0, 4 * gt, 1, float(thr["cull_screen"])),  # == cull_screen: stays (and is split; below 0 its samples are culled)
            (_scale_row(large, 1), -9.0, 4 * gt, 1, 0.0),                       # transparent, high and large: split, and every copy culled
            (_scale_row(small, 2), 3.0, 0, 1, float(thr["cull_screen"]))]       # == cull_screen, cold: stays as it is
    hand = _hand_positions(n, len(rows))
    for i, (s, op, gn, v, m) in zip(hand, rows):
        scaling[i], opacity[i], grad_norm[i], vis[i], m2d[i] = s, op, gn, v, m
    return dict(scaling=scaling, opacity=opacity, grad_norm=grad_norm, vis_counts=vis, max_2Dsize=m2d, thr=thr, hand=hand)


def margins_hold(inputs, mode):
    """The margin rule on built inputs (hand rows included: their scales and logits are placed clear of every threshold)."""
    if mode == "densify":
        return not _near(max_scale(inputs["scaling"]), [float(inputs["size_threshold"])]).any()
    if mode == "prune":
        return not (_near(max_scale(inputs["scaling"]), [float(inputs["size_threshold"])]).any() or
                    _near(sigmoid(inputs["opacity"]), [float(inputs["min_opacity"])]).any())
    t = inputs["thr"]
    return not (_near(max_scale(inputs["scaling"]), scale_thresholds(t["size_threshold"], t["cull_size"])).any() or
                _near(sigmoid(inputs["opacity"]), [float(t["cull_alpha"])]).any())


def refine_codes_possible(flags, thr):
    """The set of codes a flag combination can produce: decide_refine on one archetype row per region of (max scale, gradient, screen size, opacity)."""
    size, cull = float(thr["size_threshold"]), float(thr["cull_size"])
    assert size * REDUCE < cull
    scales = [size / 2, size * 1.3, size * 2, cull * 1.3, cull * 2]          # below | split and duplicated | split | culled unless reduced | culled
    screens = [0.0, (float(thr["split_screen"]) + abs(float(thr["cull_screen"]))) / 2, abs(float(thr["cull_screen"])) * 1.5, float(thr["cull_screen"])]
    rows = [(s, g, m, o) for s in scales for g in (0.0, 1.0) for m in screens for o in (-9.0, 3.0)]
    s, g, m, o = (np.array(c) for c in zip(*rows))
    scaling = np.log(s)[:, None] + np.array([0.0, -1.0, -2.0])
    return set(decide_refine(flags, scaling, o, g, np.ones(len(rows)), m, thr).tolist())


ALL_REFINE_FLAGS = [tuple((k >> b) & 1 for b in range(5)) for k in range(32)]          # (do_densify, do_cull, use_split_screen, cull_big, use_cull_screen)
