"""-m gpu: the actor chain and the encoder-input gradient without float atomics (csrc/track_det.hip; TrackOffsetHeads.deterministic,
nonrigid_deformation(..., deterministic=True)).
  1. emd_actor_row_sum_det is the pinned segmented sum (tests/segsum_checks.py) of the rows in ascending point index, bit for bit, with or without
     segment starts;
  2. every head gradient is the fp64 ascending-actor sum of the slab the call left, rounded once, bit for bit, and nothing is written outside the buffers;
  3. the temporal-table gradient is the numpy restatement of the gather's enumeration over the per-lane dL/dh rows the call left, bit for bit;
  4. every gradient stays inside the existing bars against the checker (oracle/torch_ref.track_offsets, fp64) and against the default mode;
  5. every gradient has identical bits from run to run, on a side stream and in two replays of a captured graph -- both launch forms,
     nonrigid_deformation and a small StreetGaussians(track_heads=True) step -- with the default entries patched to raise;
  6. the gradient of the instance embeddings is check 1's sum, and the reference golden's bars hold with the switch on."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from emd_amd import _lib as L
from emd_amd import motion
from oracle import torch_ref as tr
from tests import det_list_checks as dl
from tests import segsum_checks as sg
from tests import test_deform_gpu as deform_base
from tests.test_mlp_det_gpu import _f, _reflect, _resized_row

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("track_trans_c", "track_trans_f", "track_rot_c", "track_rot_f")


def _refuse(name):
    def f(*a, **k):
        raise AssertionError(f"{name} must not be called here")
    return f


def _refuse_defaults(monkeypatch):
    for name in ("emd_tracked_pose_backward", "emd_track_heads_backward", "emd_deform_input_backward"):
        monkeypatch.setattr(L.load(), name, _refuse(name))


# ---- 1. the row sum ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows_case(n, sizes, width, seed=0):
    """The shape of tests/test_motion_det_gpu._case: sizes[a] points of actor a, the rest with id -1, interleaved by a random permutation."""
    rng = np.random.default_rng(seed)
    ids = np.full(n, -1, np.int32)
    ids[:sum(sizes)] = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    ids = ids[rng.permutation(n)]
    rows = rng.standard_normal((n, width + 3)).astype(np.float32)
    return ids, rows


def _row_sum(ids, rows, width, A, seg=None):
    """emd_actor_row_sum_det through ctypes: NaN-filled out, 0xA5-filled workspace, the rows behind the workspace in the same allocation (so that
    tests/det_list_checks.py reads them where it reads a call's own rows) -> out [A, width] numpy, the allocation, its layout."""
    n, pitch = rows.shape
    nbytes = L.track_det_workspace_size(A, 0, n, width)
    lay = L.track_det_layout(A, 0, n, width)
    buf = torch.empty(nbytes + 4 * n * pitch, dtype=torch.uint8, device=DEV)
    buf.fill_(0xA5)
    buf[nbytes:].view(torch.float32).copy_(torch.from_numpy(rows).reshape(-1))
    ids_d = torch.from_numpy(ids).to(DEV)
    seg_d = None if seg is None else torch.from_numpy(seg).to(DEV)
    out = torch.full((A, width), float("nan"), device=DEV)
    L.check(L.load().emd_actor_row_sum_det(n, width, buf.data_ptr() + nbytes, pitch, ids_d.data_ptr(), A, L.ptr(seg_d), out.data_ptr(), width, buf.data_ptr(),
                                           nbytes, L.stream()), "emd_actor_row_sum_det")
    torch.cuda.synchronize()
    lay = dict(lay, rows=nbytes)
    return out.cpu().numpy(), buf, lay


def _pinned(ids, rows, width, A):
    """tests/segsum_checks.segsum_reference over the ids in ascending point index; an actor without a point: +0.0."""
    kept = np.flatnonzero((ids >= 0) & (ids < A))
    order = kept[np.argsort(ids[kept], kind="stable")]
    want = np.zeros((A, width), np.float32)
    sg.segsum_reference(ids[order], order, rows, width, want)
    return want


def _check_row_sum(n, sizes, width, seed=0):
    ids, rows = _rows_case(n, sizes, width, seed)
    A = len(sizes)
    out, buf, lay = _row_sum(ids, rows, width, A)
    want = _pinned(ids, rows, width, A)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    for a, size in enumerate(sizes):
        if size == 0:
            assert (out[a].view(np.uint32) == 0).all()           # +0.0
    if width <= 32:                                              # one band: the list checks of the other deterministic entries, as they stand
        _, raw, keys, _ = dl.check_lists(buf, lay, n, rows.shape[1], width, out, A)
        assert np.array_equal(raw.view(np.int32), np.where(ids >= 0, ids, -1))
    else:                                                        # two bands over the same sorted list
        _, raw, keys, slots, count = dl.read_workspace(buf, lay, n, rows.shape[1])
        assert count == sum(sizes) and (np.diff(keys.astype(np.int64)) >= 0).all() and np.array_equal(raw[slots], keys)
    # the same points sorted by actor, with and without segment starts: the bits of the interleaved call
    kept = np.flatnonzero(ids >= 0)
    if len(kept):
        order = kept[np.argsort(ids[kept], kind="stable")]
        ids_s, rows_s = np.ascontiguousarray(ids[order]), np.ascontiguousarray(rows[order])
        seg = np.searchsorted(ids_s, np.arange(A + 1)).astype(np.int32)
        plain = _row_sum(ids_s, rows_s, width, A)[0]
        with_seg = _row_sum(ids_s, rows_s, width, A, seg=seg)[0]
        assert np.array_equal(plain.view(np.uint32), out.view(np.uint32))
        assert np.array_equal(with_seg.view(np.uint32), out.view(np.uint32))
    return out


@pytest.mark.parametrize("width", [4, 10, 32, 40, 64])
def test_row_sum_is_the_pinned_sum(width):
    """4000 points, actors of 1500 (three chunks), 700 (two), 300 (one), 1 and 0 points, the rest without an actor, all interleaved; row pitch width + 3."""
    out = _check_row_sum(4000, (1500, 700, 300, 1, 0), width)
    assert (np.abs(out[:4]).max(axis=1) > 0).all()


@pytest.mark.parametrize("n,sizes", [(1, (1,)), (1, (0,)), (513, (513,)), (512, (512,)), (513, (0, 0, 0))])
def test_row_sum_edges_of_the_chunk(n, sizes):
    for width in (10, 40):
        _check_row_sum(n, sizes, width, seed=n)


# ---- the generated chain cases (checks 2 - 4) -----------------------------------------------------------------------------------------------------------
_POINTS = {"chain": (1, 2, 1025, 8193), "many": (3,) * 33}
_SHAPES = [(4, 32, "chain"), (8, 56, "chain"), (1, 2, "chain"), (4, 32, "many")]
# (frame, step, frame / step on the device): step 0 at t = 0 (k_fine = k_coarse = 30: both levels hit the same rows, t on a row boundary), step 0 at
# t = 0.5 from the device, a step past c2f_temporal_iter (k_fine = the table's 40 rows), and t = 1 (the second row lies past the end) from the device
_TIMES = [(0, 0, False), (1, 0, True), (1, 30000, False), (2, 30000, True)]
F_, ROWS = 3, 40


@functools.lru_cache(maxsize=None)
def _inputs(edim, fdim, tag):
    pts = _POINTS[tag]
    A = len(pts)
    g = torch.Generator().manual_seed(1000 * edim + fdim + A)
    heads = motion.TrackOffsetHeads(A, temporal_embedding_dim=fdim, gaussian_embedding_dim=edim, max_embeddings=ROWS)
    with torch.no_grad():
        for n in NAMES:
            lin = getattr(heads, n)
            lin.weight.copy_(0.3 * torch.randn(lin.weight.shape, generator=g))
            lin.bias.copy_(0.1 * torch.randn(lin.bias.shape, generator=g))
        heads.weight.copy_(0.5 * torch.randn(heads.weight.shape, generator=g))
    ids = torch.repeat_interleave(torch.arange(A), torch.tensor(pts))
    return types.SimpleNamespace(A=A, edim=edim, fdim=fdim, heads=heads, ids=ids, emb=torch.randn(ids.numel(), edim, generator=g),
                                 gt=torch.randn(A, 3, generator=g), gr=torch.randn(A, 4, generator=g), iq=torch.randn(F_, A, 4, generator=g) * 1.3,
                                 it=torch.randn(F_, A, 3, generator=g), fv=torch.rand(F_, A, generator=g) > 0.2, w=torch.randn(A, 12, generator=g))


class _Guarded:
    """Allocators for motion._alloc_det_ws / _alloc_det_grads: NaN-filled buffers between guard bands."""
    BAND = 1024

    def __init__(self):
        self.made = []

    def _alloc(self, nbytes, dev):
        raw = torch.empty(nbytes + 2 * self.BAND, dtype=torch.uint8, device=dev)
        raw.fill_(0x5A)
        raw[self.BAND:self.BAND + nbytes].fill_(0xFF)            # every float a NaN
        self.made.append((raw, nbytes))
        return raw[self.BAND:self.BAND + nbytes]

    def ws(self, nbytes, dev):
        return self._alloc(nbytes, dev)

    def grads(self, numel, dev):
        return self._alloc(4 * numel, dev).view(torch.float32)

    def check(self):
        assert self.made
        for raw, nbytes in self.made:
            assert bool((raw[:self.BAND] == 0x5A).all()) and bool((raw[self.BAND + nbytes:] == 0x5A).all()), "a guard band was written"


def _run(c, form, det, frame, step, on_device, ids=None, guarded=None):
    """One forward + backward of a launch form ("pose": pose_table, "heads": forward + actor_pose_table) -> dict of numpy arrays."""
    hd = motion.TrackOffsetHeads(c.A, temporal_embedding_dim=c.fdim, gaussian_embedding_dim=c.edim, max_embeddings=ROWS, deterministic=det)
    hd.load_state_dict(c.heads.state_dict())
    hd = hd.to(DEV)
    sorted_form = ids is None                                    # (pose_table takes the three-launch path for ids that are not sorted by actor)
    ids = (c.ids if ids is None else ids).to(DEV)
    e = c.emb.to(DEV).requires_grad_(True)
    iq, it = c.iq.to(DEV).requires_grad_(True), c.it.to(DEV).requires_grad_(True)
    fr = torch.tensor([frame], dtype=torch.int32, device=DEV) if on_device else frame
    st = torch.tensor([step], dtype=torch.int64, device=DEV) if on_device else step
    params = [hd.weight] + [p for n in NAMES for p in (getattr(hd, n).weight, getattr(hd, n).bias)]
    motion.DET_TRACE = [] if det else None
    old = (motion._alloc_det_ws, motion._alloc_det_grads)
    if guarded is not None:
        motion._alloc_det_ws, motion._alloc_det_grads = guarded.ws, guarded.grads
    try:
        if form == "pose":
            out = hd.pose_table(iq, it, c.fv.to(DEV), fr, e, ids, st)
            (out * c.w.to(DEV)).sum().backward()
            res = dict(out=out, d_q=iq.grad, d_t=it.grad)
        else:
            tt, rr = hd(fr, F_, e, ids, st)
            ((tt * c.gt.to(DEV)).sum() + (rr * c.gr.to(DEV)).sum()).backward()
            res = dict(out=torch.cat([tt, rr], 1))
        torch.cuda.synchronize()
        trace = motion.DET_TRACE
    finally:
        motion.DET_TRACE = None
        motion._alloc_det_ws, motion._alloc_det_grads = old
    res.update(table=params[0].grad, emb=e.grad, heads=torch.cat([p.grad.reshape(-1) for p in params[1:]]))
    res = {k: v.detach().cpu().numpy() for k, v in res.items()}
    if det:
        assert len(trace) == 1 and trace[0]["form"] == (form if sorted_form else "heads")
        width = c.fdim + c.edim
        lay = L.track_det_layout(c.A, width)
        raw = trace[0]["ws"].cpu().numpy()
        res["slab"] = raw[lay["slab"]:lay["slab"] + 4 * c.A * lay["pitch"]].view(np.float32).reshape(c.A, lay["pitch"])[:, :8 * width + 8].copy()
        res["dh"] = raw[lay["dh"]:lay["dh"] + 4 * c.A * 128].view(np.float32).reshape(c.A, 2, 64).copy()
    return res


@functools.lru_cache(maxsize=None)
def _det(edim, fdim, tag, frame, step, on_device, form):
    c = _inputs(edim, fdim, tag)
    guarded = _Guarded()
    res = _run(c, form, True, frame, step, on_device, guarded=guarded)
    guarded.check()
    return res


@functools.lru_cache(maxsize=None)
def _default(edim, fdim, tag, frame, step, on_device, form):
    return _run(_inputs(edim, fdim, tag), form, False, frame, step, on_device)


def _chain_cases(f):
    f = pytest.mark.parametrize("edim,fdim,tag", _SHAPES)(f)
    f = pytest.mark.parametrize("frame,step,on_device", _TIMES)(f)
    return pytest.mark.parametrize("form", ["pose", "heads"])(f)


# ---- 2. the head reduction --------------------------------------------------------------------------------------------------------------------------------
@_chain_cases
def test_head_gradients_are_the_ascending_fp64_sum_of_the_slab(edim, fdim, tag, frame, step, on_device, form):
    """The eight head gradients, back to back as the slot lays them out, against the slab the call left: per element the slots in ascending actor index
    in fp64 from 0.0, one rounding.  Gradient buffers, slab and dL/dh rows were NaN-filled between guard bands (_det checks the bands)."""
    got = _det(edim, fdim, tag, frame, step, on_device, form)
    slab = got["slab"]
    assert np.isfinite(slab).all()                               # every element of every slot was written
    acc = np.zeros(slab.shape[1], np.float64)
    for a in range(slab.shape[0]):
        acc = acc + slab[a].astype(np.float64)
    assert np.array_equal(got["heads"].view(np.uint32), acc.astype(np.float32).view(np.uint32))
    assert np.abs(got["heads"]).max() > 0


# ---- 3. the table gather ----------------------------------------------------------------------------------------------------------------------------------
def _sample(t, k, rows):
    iy = _reflect((_f(t) - _f(0.5)) * _f(2), k)
    y0f = np.floor(iy)
    y0 = int(y0f)
    wy1 = iy - y0f
    return dict(wy=(_f(1) - wy1, wy1), row=[_resized_row(min(y0, k - 1), k, rows), _resized_row(min(y0 + 1, k - 1), k, rows)], in1=y0 + 1 <= k - 1)


def _table_restated(rows, dim, k_c, k_f, t, dhc, dhf):
    """tests/test_mlp_det_gpu._te_restated over the two levels: column j ascending, coarse before fine, r = 0, 1, then (ha, x0), (hb, x0), (ha, x1),
    (hb, x1); each product left to right in float32, added in float64 from 0.0, rounded once."""
    levels = [(_sample(t, k_c, rows), dhc), (_sample(t, k_f, rows), dhf)]
    G = np.zeros((rows, dim), dtype=np.float64)
    touched = set()
    for j in range(dim):
        gx = (_f(j) / _f(dim - 1) - _f(0.5)) * _f(2) if dim > 1 else _f(-1)
        ix = _reflect(gx, dim)
        x0f = np.floor(ix)
        x0 = int(x0f)
        wx1 = ix - x0f
        wx0 = _f(1) - wx1
        for s, g in levels:
            for r in range(2):
                if r == 1 and not s["in1"]:
                    continue
                ha, hb, la, lb = s["row"][r]
                touched.update((ha, hb))
                G[ha, x0] += np.float64(_f(g[j]) * wx0 * s["wy"][r] * la)
                G[hb, x0] += np.float64(_f(g[j]) * wx0 * s["wy"][r] * lb)
                if x0 + 1 <= dim - 1:
                    G[ha, x0 + 1] += np.float64(_f(g[j]) * wx1 * s["wy"][r] * la)
                    G[hb, x0 + 1] += np.float64(_f(g[j]) * wx1 * s["wy"][r] * lb)
    return G.astype(np.float32), touched


@_chain_cases
def test_table_gradient_is_the_enumeration_over_the_dh_rows(edim, fdim, tag, frame, step, on_device, form):
    got = _det(edim, fdim, tag, frame, step, on_device, form)
    c = _inputs(edim, fdim, tag)
    t = frame / (F_ - 1)
    k_f = c.heads.int_lininterp(step, c.heads.min_embeddings, ROWS, c.heads.c2f_temporal_iter)
    assert k_f == (30 if step == 0 else ROWS)
    for a in range(c.A):
        want, touched = _table_restated(ROWS, fdim, c.heads.min_embeddings, k_f, t, got["dh"][a, 0], got["dh"][a, 1])
        assert np.array_equal(got["table"][a].view(np.uint32), want.view(np.uint32)), a
        untouched = np.array([r not in touched for r in range(ROWS)])
        assert (got["table"][a][untouched].view(np.uint32) == 0).all()       # +0.0
        assert len(touched) <= 8 and (np.abs(got["table"][a]).max(axis=1) > 0).sum() <= 8
    assert np.abs(got["table"]).max() > 0


# ---- 4. against the checker and the default ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _checker(edim, fdim, tag, frame, step, form, ids_key=None):
    c = _inputs(edim, fdim, tag)
    ids = c.ids if ids_key is None else _interleaved(c)
    w0 = c.heads.weight.detach().double().requires_grad_(True)
    e0 = c.emb.double().requires_grad_(True)
    hp = {n: (getattr(c.heads, n).weight.detach().double().requires_grad_(True), getattr(c.heads, n).bias.detach().double().requires_grad_(True)) for n in NAMES}
    t0, r0 = tr.track_offsets(w0, hp, frame, F_, e0, ids, step, min_embeddings=c.heads.min_embeddings, max_embeddings=ROWS,
                              c2f_temporal_iter=c.heads.c2f_temporal_iter)
    if form == "pose":
        pose = motion.build_actor_pose(c.iq.double(), c.it.double(), c.fv, frame, t0, r0)
        (pose * c.w.double()).sum().backward()
    else:
        ((t0 * c.gt.double()).sum() + (r0 * c.gr.double()).sum()).backward()
    heads = torch.cat([p.grad.reshape(-1) for n in NAMES for p in hp[n]])
    return dict(table=w0.grad.numpy(), emb=e0.grad.numpy(), heads=heads.numpy(), offsets=torch.cat([t0, r0], 1).detach().numpy())


def _head_parts(width):
    """(name, slice) of the eight tensors inside the back-to-back head gradients."""
    sizes = [3 * width, 3, 3 * width, 3, width, 1, width, 1]
    names = [f"{n}.{k}" for n in NAMES for k in ("weight", "bias")]
    starts = np.concatenate(([0], np.cumsum(sizes)))
    return [(names[i], slice(starts[i], starts[i + 1])) for i in range(8)]


@_chain_cases
def test_gradients_against_the_checker_and_the_default_mode(edim, fdim, tag, frame, step, on_device, form):
    got, default = _det(edim, fdim, tag, frame, step, on_device, form), _default(edim, fdim, tag, frame, step, on_device, form)
    ref = _checker(edim, fdim, tag, frame, step, form)
    width = edim + fdim
    # the checker in fp64: the bar of test_fused_track_heads_match_the_checker_forward_and_backward
    pairs = [("temporal tables", got["table"], ref["table"]), ("embeddings", got["emb"], ref["emb"])]
    pairs += [(name, got["heads"][sl], ref["heads"][sl]) for name, sl in _head_parts(width)]
    for what, a, b in pairs:
        d, m = np.abs(a - b).max(), np.abs(b).max()
        print(f"{what} gradient vs checker: max |err| {d:.3e}, max |ref| {m:.3e}")
        assert d <= 1e-4 * m + 1e-7, (what, d, m)
    # the default mode: sorted ids -> the same forward launch, bit for bit
    assert np.array_equal(got["out"].view(np.uint32), default["out"].view(np.uint32))
    for k in ("table", "emb") + (("d_q", "d_t") if form == "pose" else ()):
        d, m = np.abs(got[k] - default[k]).max(), np.abs(default[k]).max()
        print(f"{k} vs the default mode: max |err| {d:.3e}, max |ref| {m:.3e}")
        assert d <= 2e-5 * m + 1e-7, (k, d, m)
    A = got["slab"].shape[0]
    bound = 2 * A * 2.0 ** -24 * np.abs(got["slab"].astype(np.float64)).sum(axis=0)
    err = np.abs(got["heads"].astype(np.float64) - default["heads"])
    print(f"head gradients vs the default mode: worst |err| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()


def _interleaved(c):
    g = torch.Generator().manual_seed(5)
    return c.ids[torch.randperm(c.ids.numel(), generator=g)]


@pytest.mark.parametrize("form", ["pose", "heads"])
@pytest.mark.parametrize("edim,fdim", [(4, 32), (8, 56)])
def test_interleaved_ids_take_the_row_sum_in_the_forward(edim, fdim, form, monkeypatch):
    """Ids that are not sorted by actor: the embedding mean comes from emd_actor_row_sum_det (another association than the sorted form's), the chain
    runs in the three-launch form.  Offsets against the checker within the existing rtol = atol = 1e-5, gradients within 1e-4 max|ref| + 1e-7."""
    _refuse_defaults(monkeypatch)
    c = _inputs(edim, fdim, "chain")
    frame, step = 1, 30000
    got = _run(c, form, True, frame, step, False, ids=_interleaved(c))
    ref = _checker(edim, fdim, "chain", frame, step, form, ids_key="interleaved")
    if form == "heads":
        np.testing.assert_allclose(got["out"], ref["offsets"], rtol=1e-5, atol=1e-5)
    pairs = [("temporal tables", got["table"], ref["table"]), ("embeddings", got["emb"], ref["emb"])]
    pairs += [(name, got["heads"][sl], ref["heads"][sl]) for name, sl in _head_parts(edim + fdim)]
    for what, a, b in pairs:
        d, m = np.abs(a - b).max(), np.abs(b).max()
        assert d <= 1e-4 * m + 1e-7, (what, d, m)


@pytest.mark.parametrize("order", ["sorted", "interleaved"])
def test_embedding_gradient_of_the_heads_form_has_the_default_entrys_bits(order):
    """emd_track_heads_backward_det against emd_track_heads_backward through ctypes on the same inputs (A = 3, dim = 4, E = 4, 130 points in more
    than one workgroup of the per-point launch; the same forward sums): dL/d embeddings is per point, d_mean[id] / count[id] by embed.hip's own
    k_track_embed_bwd in both, and d_mean is the same expressions in both units -- bit for bit."""
    A, dim, E, n, rows = 3, 4, 4, 130, ROWS
    g = torch.Generator().manual_seed(130)
    ids = torch.repeat_interleave(torch.arange(A), torch.tensor([70, 1, 59]))
    if order == "interleaved":
        ids = ids[torch.randperm(n, generator=g)]
        assert bool((ids[1:] < ids[:-1]).any())
    width = dim + E
    r = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=g)).to(DEV)
    weight, emb = r(A, rows, dim, s=0.5), r(n, E)
    heads = [r(3, width, s=0.3), r(3, s=0.1), r(3, width, s=0.3), r(3, s=0.1), r(1, width, s=0.3), r(1, s=0.1), r(1, width, s=0.3), r(1, s=0.1)]
    g_trans, g_rot = r(A, 3), r(A, 4)
    ids32 = ids.to(torch.int32).to(DEV)
    cnt = torch.bincount(ids, minlength=A).float().to(DEV)
    emb_sum = torch.zeros(A, E, device=DEV).index_add_(0, ids.to(DEV), emb)
    a = motion._TrackHeads._args(weight, emb, heads, ids32, cnt, None, 0.5, 30, ROWS, emb_sum, None, None)
    got = {}
    for det in (False, True):
        bufs = dict(d_weight=torch.zeros(A, rows, dim, device=DEV), d_emb=torch.full((n, E), float("nan"), device=DEV), d_mean=torch.empty(A, E, device=DEV),
                    d_heads=[torch.zeros_like(h) for h in heads])
        gr = L.EmdTrackGrads()
        gr.g_trans, gr.g_rot, gr.d_weight = g_trans.data_ptr(), g_rot.data_ptr(), bufs["d_weight"].data_ptr()
        gr.d_embeddings, gr.d_mean = bufs["d_emb"].data_ptr(), bufs["d_mean"].data_ptr()
        for h in range(4):
            gr.d_head_w[h], gr.d_head_b[h] = bufs["d_heads"][2 * h].data_ptr(), bufs["d_heads"][2 * h + 1].data_ptr()
        if det:
            ws = torch.empty(L.track_det_workspace_size(A, width), dtype=torch.uint8, device=DEV)
            L.check(L.load().emd_track_heads_backward_det(C.byref(a), C.byref(gr), ws.data_ptr(), ws.numel(), L.stream()), "emd_track_heads_backward_det")
        else:
            L.check(L.load().emd_track_heads_backward(C.byref(a), C.byref(gr), L.stream()), "emd_track_heads_backward")
        torch.cuda.synchronize()
        got[det] = bufs["d_emb"]
    assert bool(torch.isfinite(got[True]).all()) and float(got[True].abs().min()) > 0
    assert torch.equal(got[True], got[False])
    assert torch.equal(got[True].view(torch.int32), got[False].view(torch.int32))


# ---- 5. the same bits in every setting ----------------------------------------------------------------------------------------------------------------------
def _same_bits_everywhere(step):
    """step() -> list of gradients: two eager runs, a run on a side stream behind a busy main stream, two replays of a captured graph."""
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    first = [g.clone() for g in step()]
    for i, g in enumerate(first):
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, f"gradient {i} is not finite or all zero"
    assert same(first, step())
    busy = torch.randn(2048, 2048, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(8):
        busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        on_side = [g.clone() for g in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert same(first, on_side)
    with torch.cuda.stream(side):
        step()                                                   # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same(first, captured)


@pytest.mark.parametrize("form,sorted_ids", [("pose", True), ("heads", True), ("heads", False)])
def test_chain_has_identical_bits_across_runs_streams_and_graph_replay(form, sorted_ids, monkeypatch):
    _refuse_defaults(monkeypatch)
    c = _inputs(4, 32, "chain")
    hd = motion.TrackOffsetHeads(c.A, temporal_embedding_dim=32, gaussian_embedding_dim=4, max_embeddings=ROWS, deterministic=True)
    hd.load_state_dict(c.heads.state_dict())
    hd = hd.to(DEV)
    ids = (c.ids if sorted_ids else _interleaved(c)).to(DEV)
    e = c.emb.to(DEV).requires_grad_(True)
    iq, it, fv, w = c.iq.to(DEV).requires_grad_(True), c.it.to(DEV).requires_grad_(True), c.fv.to(DEV), c.w.to(DEV)
    fr, st = torch.tensor([1], dtype=torch.int32, device=DEV), torch.tensor([12000], dtype=torch.int64, device=DEV)
    params = [hd.weight] + [p for n in NAMES for p in (getattr(hd, n).weight, getattr(hd, n).bias)]

    def step():
        if form == "pose":
            pose = hd.pose_table(iq, it, fv, fr, e, ids, st)
        else:
            tt, rr = hd(fr, F_, e, ids, st)
            pose = motion.actor_pose_table(iq, it, fv, fr, tt, rr)
        return torch.autograd.grad((pose * w).sum(), [e, iq, it] + params)
    _same_bits_everywhere(step)


def _deform_case(E, seed=3):
    from emd_amd.deformation import ConditionalDeformNetwork
    g = torch.Generator().manual_seed(seed)
    N, A = 3001, 5
    torch.manual_seed(seed)
    net = ConditionalDeformNetwork(D=4, W=64, embed_dim=E, x_multires=4, t_multires=4).to(DEV)
    ids = torch.randint(0, A, (N,), generator=g)
    return types.SimpleNamespace(net=net, N=N, A=A, E=E, ids=ids.to(DEV), means=torch.randn(N, 3, generator=g).to(DEV),
                                 size=(torch.rand(A, 3, generator=g) + 0.5).to(DEV), emb=torch.randn(A, E, generator=g).to(DEV).requires_grad_(True),
                                 t=torch.tensor([0.35], device=DEV), gx=torch.randn(N, 3, generator=g).to(DEV), gq=torch.randn(N, 4, generator=g).to(DEV))


def test_nonrigid_deformation_has_identical_bits_across_runs_streams_and_graph_replay(monkeypatch):
    from emd_amd.deformation import nonrigid_deformation
    _refuse_defaults(monkeypatch)
    d = _deform_case(10)

    def step():
        dx, dq, _ = nonrigid_deformation(d.net, d.means, d.ids, d.size, d.emb, d.t, deterministic=True)
        return torch.autograd.grad((dx * d.gx).sum() + (dq * d.gq).sum(), [d.emb])
    _same_bits_everywhere(step)


def test_street_gaussians_step_has_identical_bits_across_runs_streams_and_graph_replay(monkeypatch):
    """A small StreetGaussians(track_heads=True) step -- actor chain -> rasterizer with fused actor motion -> a scalar loss on the image -- with the
    rasterizer's deterministic=True and model.track_heads.deterministic = True."""
    from emd_amd import RasterOptions, scenes
    from emd_amd.model import StreetGaussians, render
    _refuse_defaults(monkeypatch)
    dev = torch.device("cuda", 0)
    N, H, W = 30000, 96, 160                                     # the scene of tests/test_det_step_gpu.py: its three actors are in view of this camera
    scene = scenes.add_actors(scenes.make_static_scene(N, seed=0), num_actors=3, pts_per_actor=2000, num_frames=5, seed=1)
    model = StreetGaussians(scene, dev, track_heads=True)
    model.track_heads.deterministic = True
    cam = scenes.rig_camera(2, 0, H, W)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(9)).to(dev)
    opts = RasterOptions(deterministic=True, no_sync=True, capacity_hint=1 << 20)
    heads = model.track_heads
    leaves = [model._xyz, model._scaling, model._rotation, model._opacity, model._features, model.instances_quats, model.instances_trans, model._embeddings, heads.weight]
    leaves += [p for n in NAMES for p in (getattr(heads, n).weight, getattr(heads, n).bias)]
    bg = torch.zeros(3)

    def step():
        out = render(model, cam, bg, frame=2, options=opts)
        return torch.autograd.grad((out["render"] - gt).abs().mean(), leaves)
    _same_bits_everywhere(step)


# ---- 6. the encoder input ---------------------------------------------------------------------------------------------------------------------------------------
def test_golden_holds_with_the_switch_on(monkeypatch):
    """tests/test_deform_gpu.test_nonrigid_deformation_matches_reference_golden as it stands, its bars, with the switch on."""
    from emd_amd import deformation
    monkeypatch.setattr(L.load(), "emd_deform_input_backward", _refuse("emd_deform_input_backward"))
    monkeypatch.setattr(deformation, "nonrigid_deformation", functools.partial(deformation.nonrigid_deformation, deterministic=True))
    deform_base.test_nonrigid_deformation_matches_reference_golden()


@pytest.mark.parametrize("E", [10, 40])
def test_embedding_gradient_is_the_pinned_sum(E):
    """dL/d instances_embedding = the pinned sum of g[:, col0 : col0 + E] per actor: ids interleaved and containing -1, ld > col0 + E."""
    rng = np.random.default_rng(E)
    n, A, col0, ld = 3001, 7, 5, 5 + E + 6
    ids = rng.integers(-1, A, n).astype(np.int32)
    ids[ids == 3] = -1                                           # an actor without a point
    g = rng.standard_normal((n, ld)).astype(np.float32)
    got = L.actor_row_sum_det(torch.from_numpy(g).to(DEV), E, torch.from_numpy(ids).to(DEV), A, col0=col0).cpu().numpy()
    want = _pinned(ids, np.ascontiguousarray(g[:, col0:col0 + E]), E, A)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[3].view(np.uint32) == 0).all() and (ids < 0).sum() > 100


def test_embedding_gradient_through_the_encoder_input(monkeypatch):
    """The same through _DeformInput's backward (E = 10, ids interleaved): the pinned sum of the incoming gradient's embedding columns, bit for bit, and
    identical bits across runs, on a side stream and in a graph replay."""
    from emd_amd.deformation import _DeformInput
    _refuse_defaults(monkeypatch)
    d = _deform_case(10)
    width = L.load().emd_deform_input_width(4, 4, 10)
    gout = torch.randn(d.N, width, generator=torch.Generator().manual_seed(1)).to(DEV)

    def step():
        h0 = _DeformInput.apply(d.means, d.ids, d.size, d.emb, d.t, 4, 4, True)
        return torch.autograd.grad((h0 * gout).sum(), [d.emb])
    got = step()[0].cpu().numpy()
    want = _pinned(d.ids.cpu().numpy().astype(np.int32), np.ascontiguousarray(gout.cpu().numpy()[:, width - 10:]), 10, d.A)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    _same_bits_everywhere(step)
