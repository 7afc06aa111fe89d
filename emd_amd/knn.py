"""Exact k nearest neighbours on the device, and what the training loop builds on them (include/emd_raster.h, ABI 28; csrc/knn.hip).

    from emd_amd.knn import distCUDA2           # was: from simple_knn._C import distCUDA2   (S3Gaussian/scene/gaussian_model.py:152-181)
    table = KnnTable(gaussians.get_xyz, k=20)   # was: o3d_knn(xyz, 20): open3d + a Python loop over the points   (train.py:326-337)
    loss = loss + lambda_reg * embedding_reg(gaussians.get_embedding, table)        # was: weighted_l2_loss_v2(emb[:, None], emb[idx], w)

`knn` / `distCUDA2` are one call of `emd_knn` (a Z-order sort and a pruned, exact search: no host synchronisation); `embedding_reg` is a
`torch.autograd.Function` on `emd_embed_reg_forward` / `emd_embed_reg_backward`: one launch each, no host read, no allocation that depends on
device data, so it records into a hipGraph like the image loss.  Its gradient is formed by gathers over the table and its transposed adjacency
(built once per table by `emd_knn_reverse`) in a fixed order: bit-identical from run to run.  No CPU path.

For OmniRe's SMPLNodes: `knn_segments` / `KnnTable(..., segment_start=)` keep a point's neighbours inside its own segment
(one `emd_knn_segments` launch instead of `pytorch3d.knn_points` in a loop over people), and `neighbour_std` is the k-NN regulariser over such a
table, `act(x)[cat(self, idx)].std(dim=1).mean() * w` for up to eight blocks in one launch each way (csrc/neighbour_reg.hip)."""
import ctypes as C

import torch

from . import _lib as L

MAX_K = L.KNN_MAX_K
EMBED_DIMS = (4, 8, 16, 32)


def _points(points):
    L.need_device("knn", points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"knn: points must be [N, 3], got {tuple(points.shape)}")
    return points.detach().contiguous().float()


def _check_k(k):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"knn: k must be in 1 .. {MAX_K}, got {k}")
    return k


def _knn_into(pts, k, idx, d2, mean, ws):
    n = pts.shape[0]
    if n == 0:
        return None
    need = L.load().emd_knn_workspace(n, k)
    if need == 0:
        raise ValueError(f"knn: {n} points x {k} neighbours is outside the supported range")
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=pts.device)
    L.launch("emd_knn", n, k, pts.data_ptr(), L.ptr(idx), L.ptr(d2), L.ptr(mean), ws.data_ptr(), ws.numel())
    return ws


def knn(points, k):
    """-> (idx [N,k] int32, d2 [N,k] fp32): for every point the k nearest OTHER points, rows ascending in the squared distance.  Exact; self is
    excluded by index (coincident points are neighbours at distance 0); with fewer than k other points the missing slots hold -1 / +inf; a point
    with a NaN or infinite coordinate gets a row of -1 / +inf and is nobody's neighbour.  Which of several equidistant points is returned is
    unspecified, but the call is deterministic."""
    pts, k = _points(points), _check_k(k)
    n = pts.shape[0]
    idx = torch.empty(n, k, dtype=torch.int32, device=pts.device)
    d2 = torch.empty(n, k, dtype=torch.float32, device=pts.device)
    _knn_into(pts, k, idx, d2, None, None)
    return idx, d2


def distCUDA2(points):
    """-> [N]: the mean squared distance of every point to its 3 nearest neighbours (simple_knn._C.distCUDA2)."""
    pts = _points(points)
    out = torch.empty(pts.shape[0], dtype=torch.float32, device=pts.device)
    _knn_into(pts, 3, None, None, out, None)
    return out


def _segments(segment_start, pts):
    if not isinstance(segment_start, torch.Tensor) or segment_start.device != pts.device:
        raise L.EmdError("knn_segments: segment_start must be a tensor on the points' ROCm device (it is read there); there is no CPU path")
    if segment_start.dim() != 1 or segment_start.numel() < 1 or segment_start.dtype not in (torch.int32, torch.int64):
        raise ValueError("knn_segments: segment_start must be an integer tensor [S + 1]")
    return segment_start.to(torch.int32).contiguous()


def _knn_segments_into(pts, seg, k, idx, d2):
    L.launch("emd_knn_segments", pts.shape[0], seg.numel() - 1, k, pts.data_ptr(), seg.data_ptr(), L.ptr(idx), L.ptr(d2))


def knn_segments(points, segment_start, k):
    """`knn` inside segments: segment s owns the rows [segment_start[s], segment_start[s+1]) (an ascending device table [S+1], read on the
    device) and a row's neighbours are the k nearest OTHER rows of its own segment, as global row numbers.  Rows outside every segment, rows with
    a non-finite coordinate and the slots a small segment cannot fill hold -1 / +inf.  Among equidistant candidates the lower row comes first.
    One launch, no workspace (emd_knn_segments)."""
    pts, k = _points(points), _check_k(k)
    seg = _segments(segment_start, pts)
    n = pts.shape[0]
    idx = torch.empty(n, k, dtype=torch.int32, device=pts.device)
    d2 = torch.empty(n, k, dtype=torch.float32, device=pts.device)
    _knn_segments_into(pts, seg, k, idx, d2)
    return idx, d2


class KnnTable:
    """The neighbour table of the embedding regulariser: `idx`, `d2` [N,k], the pair weights `w` [N,k], the transposed adjacency
    (`rev_start` [N+1], `rev_slot` [N*k]: see emd_knn_reverse) and the workspaces.  Built once, and again after the trainer's density control
    changed the points: `refresh(points)` rebuilds in place when N is unchanged and reallocates otherwise.

    `w` is all ones unless `weight_fn(d2) -> w` is given (slots without a neighbour have d2 = +inf and idx = -1; they never contribute).  The
    reference derives its weights from the squared distances in train.py:326-337; that rule was not available when this was written, so the
    trainer passes it as `weight_fn`, e.g. `lambda d2: torch.exp(-2000 * d2)`.
    `store_factors`: keep the per-pair factor w / sqrt(w |e_n - e_m|^2 + 1e-20) of the forward for the backward instead of recomputing it
    there (the backward reads either that factor or the weight, so recomputing saves the forward's write; profiles/knn_microbench.json).
    `segment_start` [S+1] (a device table, see `knn_segments`): the neighbours of a row are rows of its own segment -- the table of
    `neighbour_std` over SMPL instances; `refresh(points, segment_start=...)` installs another table, otherwise the last one is kept."""

    def __init__(self, points, k=20, weight_fn=None, store_factors=False, segment_start=None):
        self.k = _check_k(k)
        self.segment_start = segment_start
        self._nstd_ws = None
        self.weight_fn = weight_fn
        self.store_factors = bool(store_factors)
        self.N = -1
        self._ws = self._rev_ws = None
        self.refresh(points)

    def refresh(self, points, segment_start=None):
        pts = _points(points)
        if segment_start is not None:
            self.segment_start = segment_start
        n, k, dev = pts.shape[0], self.k, pts.device
        if n != self.N or self.idx.device != dev:
            self.idx = torch.empty(n, k, dtype=torch.int32, device=dev)
            self.d2 = torch.empty(n, k, dtype=torch.float32, device=dev)
            self.rev_start = torch.empty(n + 1, dtype=torch.int32, device=dev)
            self.rev_slot = torch.empty(n * k, dtype=torch.int32, device=dev)
            self.factors = torch.empty(n, k, dtype=torch.float32, device=dev) if self.store_factors else None
            # granule table of the forward's reduction: zero between calls; a hipGraph recorded with this table has its address baked in
            self._scratch = torch.zeros(L.EMBED_REG_SCRATCH_WORDS, dtype=torch.int32, device=dev)
            self._ws = self._rev_ws = None
            self.N = n
        if self.segment_start is None:
            self._ws = _knn_into(pts, k, self.idx, self.d2, None, self._ws)
        else:
            _knn_segments_into(pts, _segments(self.segment_start, pts), k, self.idx, self.d2)
        need = L.load().emd_knn_reverse_workspace(n, k)
        if self._rev_ws is None or self._rev_ws.numel() < need:
            self._rev_ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        L.launch("emd_knn_reverse", n, k, self.idx.data_ptr(), self.rev_start.data_ptr(), self.rev_slot.data_ptr(), self._rev_ws.data_ptr(),
                 self._rev_ws.numel())
        if self.weight_fn is None:
            self.w, self._unit = torch.ones(n, k, dtype=torch.float32, device=dev), True
        else:
            self.set_weights(self.weight_fn(self.d2))
        return self

    def set_weights(self, w):
        """Install pair weights [N,k] (no gradient flows to them)."""
        w = w.detach().to(self.idx.device).float().contiguous()
        if tuple(w.shape) != (self.N, self.k):
            raise ValueError(f"KnnTable: weights must be [{self.N}, {self.k}], got {tuple(w.shape)}")
        self.w, self._unit = w, False

    def _w_ptr(self):
        return None if self._unit else self.w.data_ptr()       # (NULL = ones: the kernels skip the read)


def _check_table(e, table):
    L.need_device("embedding_reg", e)
    if e.dim() != 2 or e.shape[1] not in EMBED_DIMS:
        raise ValueError(f"embedding_reg: the embedding must be [N, E] with E in {EMBED_DIMS}, got {tuple(e.shape)}")
    if e.shape[0] != table.N:
        raise ValueError(f"embedding_reg: the table was built for {table.N} points, the embedding has {e.shape[0]} rows "
                         "(stale table: rebuild it after density control with KnnTable.refresh / GaussianModel.knn_table)")
    if e.device != table.idx.device:
        raise ValueError("embedding_reg: the embedding and the table live on different devices")


def embed_reg_forward(e, table):
    """-> [2] device tensor: (loss, 1 / number of pairs).  `e` fp32 contiguous [N,E]."""
    out = torch.empty(2, dtype=torch.float32, device=e.device)
    L.launch("emd_embed_reg_forward", table.N, table.k, e.shape[1], e.data_ptr(), table.idx.data_ptr(), table._w_ptr(), L.ptr(table.factors),
             out.data_ptr(), table._scratch.data_ptr())
    return out


def embed_reg_backward(e, table, fwd, g, grad_e, accumulate=False):
    """grad_e (+)= g * dloss/de with `fwd` the forward's result for the same `e` and `g` a one-element device tensor; `accumulate=True` adds
    into `grad_e` (e.g. the buffer the rasterizer's gradients land in) instead of overwriting it."""
    L.launch("emd_embed_reg_backward", table.N, table.k, e.shape[1], e.data_ptr(), table.idx.data_ptr(), table._w_ptr(), L.ptr(table.factors),
             table.rev_start.data_ptr(), table.rev_slot.data_ptr(), g.data_ptr(), fwd.data_ptr() + 4, grad_e.data_ptr(),
             1 if accumulate else 0)
    return grad_e


class _EmbeddingReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, embedding, table):
        e = embedding.detach().contiguous().float()
        fwd = embed_reg_forward(e, table)
        ctx.save_for_backward(e, fwd)
        ctx.table = table
        return fwd[0].clone()

    @staticmethod
    def backward(ctx, g):
        e, fwd = ctx.saved_tensors
        if ctx.table.N != e.shape[0]:
            raise ValueError("embedding_reg: the table was rebuilt for another point count between forward and backward")
        grad = torch.empty_like(e)
        embed_reg_backward(e, ctx.table, fwd, g.contiguous().float(), grad, accumulate=False)
        return grad, None


def embedding_reg(embedding, table):
    """-> scalar: mean over the table's pairs of sqrt(w[n,j] * |e[n] - e[idx[n,j]]|^2 + 1e-20), the reference's
    weighted_l2_loss_v2(e[:, None, :], e[idx], w); differentiable with respect to `embedding` only."""
    _check_table(embedding, table)
    return _EmbeddingReg.apply(embedding, table)


# ---- the neighbour-std regulariser of SMPLNodes (csrc/neighbour_reg.hip) --------------------------------------------------------------------------
def _nstd_args(table, xs, acts, weights):
    a = L.EmdNeighbourStdArgs()
    a.num_points, a.k, a.num_blocks = table.N, table.k, len(xs)
    a.idx, a.rev_start, a.rev_slot = table.idx.data_ptr(), table.rev_start.data_ptr(), table.rev_slot.data_ptr()
    for b, (x, act, w) in enumerate(zip(xs, acts, weights)):
        a.x[b], a.cols[b], a.act[b], a.weight[b] = x.data_ptr(), x.shape[1], act, w
    return a


def _cols(x):
    return int(torch.Size(x.shape[1:]).numel())              # ([N] -> 1)


class _NeighbourStd(torch.autograd.Function):
    """One autograd node: `emd_neighbour_std_forward` and `emd_neighbour_std_backward`, one launch each."""

    @staticmethod
    def forward(ctx, table, acts, weights, *blocks):
        dev = table.idx.device
        xs = [x.detach().reshape(x.shape[0], _cols(x)).contiguous().float() for x in blocks]
        a = _nstd_args(table, xs, acts, weights)
        active = sum(x.shape[1] for x, w in zip(xs, weights) if w != 0.0)
        stash = torch.empty(table.N * active * 2 + 2, dtype=torch.float32, device=dev)
        terms = torch.empty(len(xs), dtype=torch.float32, device=dev)
        if table._nstd_ws is None or table._nstd_ws.device != dev:
            # the ticket at its head is zero between calls; a hipGraph recorded with this table has the address baked in
            table._nstd_ws = torch.zeros(int(L.load().emd_neighbour_std_workspace_size()), dtype=torch.uint8, device=dev)
        a.stash, a.terms = stash.data_ptr(), terms.data_ptr()
        L.launch("emd_neighbour_std_forward", C.byref(a), table._nstd_ws.data_ptr(), table._nstd_ws.numel())
        ctx.save_for_backward(stash, *xs)
        ctx.table, ctx.acts, ctx.weights, ctx.shapes = table, acts, weights, [x.shape for x in blocks]
        return terms

    @staticmethod
    def backward(ctx, g):
        stash, *xs = ctx.saved_tensors
        table = ctx.table
        if table.N != xs[0].shape[0]:
            raise ValueError("neighbour_std: the table was rebuilt for another point count between forward and backward")
        a = _nstd_args(table, xs, ctx.acts, ctx.weights)
        g = g.contiguous().float()
        grads = [torch.empty_like(x) if w != 0.0 else None for x, w in zip(xs, ctx.weights)]
        for b, d in enumerate(grads):
            a.dx[b] = L.ptr(d)
        a.stash, a.g_terms = stash.data_ptr(), g.data_ptr()
        L.launch("emd_neighbour_std_backward", C.byref(a))
        return (None, None, None) + tuple(None if d is None else d.reshape(s) for d, s in zip(grads, ctx.shapes))


def neighbour_std(blocks, table, weights, activations):
    """-> terms [B]: terms[b] = weights[b] * act_b(blocks[b])[cat(self, table.idx)].std(dim=1).mean(), the k-NN regulariser of SMPLNodes over the
    groups {n} + table.idx[n] (so the table holds K - 1 neighbours for the reference's `knn_neighbors` = K).  blocks: up to 8 tensors [N, ...]
    with 1 .. 64 columns after flattening; activations: "identity" | "exp" | "sigmoid" per block; weights: Python numbers, a block whose weight
    is 0 is skipped (value 0, no gradient).  One autograd node, one launch each way, no host read, no allocation that depends on device data: it
    records into a hipGraph.  Values and gradients are bit-identical from run to run (the contract: EmdNeighbourStdArgs, include/emd_raster.h).
    No gradient flows to the table or the positions."""
    blocks = list(blocks)
    L.need_device("neighbour_std (the checker's restatement is tests/neighbour_std_ref.py)", *blocks)
    if not 1 <= len(blocks) <= L.NSTD_MAX_BLOCKS:
        raise ValueError(f"neighbour_std: 1 .. {L.NSTD_MAX_BLOCKS} blocks, got {len(blocks)}")
    if len(weights) != len(blocks) or len(activations) != len(blocks):
        raise ValueError("neighbour_std: one weight and one activation per block")
    for x in blocks:
        if x.dim() < 1 or x.shape[0] != table.N:
            raise ValueError(f"neighbour_std: the table was built for {table.N} points, a block has shape {tuple(x.shape)} "
                             "(stale table: refresh it after the point set changed)")
        cols = _cols(x)
        if not 1 <= cols <= L.NSTD_MAX_COLS:
            raise ValueError(f"neighbour_std: a block must have 1 .. {L.NSTD_MAX_COLS} columns, got {cols}")
        if x.device != table.idx.device:
            raise ValueError("neighbour_std: a block and the table live on different devices")
    try:
        acts = tuple(L.NSTD_ACT[a] for a in activations)
    except KeyError as e:
        raise ValueError(f"neighbour_std: unknown activation {e.args[0]!r}; one of {sorted(L.NSTD_ACT)}") from None
    return _NeighbourStd.apply(table, acts, tuple(float(w) for w in weights), *blocks)
