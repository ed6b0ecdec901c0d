"""k-nearest-neighbour hypergraph construction (include/hg_aggr.h, hg_knn_f32): the hyperedges of HGNN's ModelNet40 /
NTU2012 hypergraphs and of DHGNN's layers, "each vertex and its k nearest neighbours in feature space", found on the
device without the N x N distance matrix.

`knn` and `knn_incidence_weights` are exported as `ops.knn` / `ops.knn_incidence_weights`; `incidence_from_knn` is the
host-side layout step of `HyperGraph.from_knn`.

`knn_transpose` and `knn_aggr` (`ops.knn_transpose` / `ops.knn_aggr`; hg_table_* in include/hg_aggr.h) aggregate over the
neighbour table itself, with no plan and no host step, and `KnnHypergraph` is the device-only hypergraph they serve.
`knn_dist` (`ops.knn_dist`) gives a table's distances with a gradient, and `knn_aggr(weight_grad=True)` the gradient of its
weights: together they train through the weights of a probabilistic kNN hypergraph.
"""
import ctypes
import numbers

import numpy as np
import torch

from . import _lib
from .plan import _check_feat, _ptr, _stream_handle
from .synth import Incidence

K_MAX = 64        # include/hg_aggr.h: k in 1 .. 64
SLICES_MAX = 32   # cand_slices in 0 .. 32
FORMS = ("difference", "dot")
DOT_F_MAX = 65536  # form="dot": the widest rows the error bound is derived for (hg_knn.h, kDotMaxF)


_NO_FORM = " (%s has no bfloat16 / float16 / float64 form)"
_KNN_NO_FORM = ' (knn has no float16 / float64 form; form="dot" takes bfloat16 rows, X and queries alike)'


def _check_dtype(t, label, dtype, note=""):
    """TypeError unless t is a tensor of `dtype`, torch.float32 or torch.int32; `note` follows "tensor" in the text."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError("%s must be %s tensor%s, got %s" % (label, "a float32" if dtype == torch.float32 else "an int32", note,
                                                            getattr(t, "dtype", type(t))))


def _check_transpose_types(transpose):
    """The first phase of the check of a `transpose` argument, with the caller's other TypeErrors: None, or the pair
    (ptr_v, pos_v) of int32 tensors."""
    if transpose is None:
        return
    if not isinstance(transpose, (tuple, list)) or len(transpose) != 2:
        raise TypeError("transpose must be the pair (ptr_v, pos_v) of knn_transpose")
    for name, t in zip(("ptr_v", "pos_v"), transpose):
        _check_dtype(t, "transpose's " + name, torch.int32)


def _check_transpose_shapes(transpose, n, entries):
    """The second phase, with the caller's other ValueErrors: ptr_v [n + 1] and pos_v [entries]."""
    if transpose is not None and (tuple(transpose[0].shape) != (n + 1,) or tuple(transpose[1].shape) != (entries,)):
        raise ValueError("transpose must be (ptr_v [%d], pos_v [%d]), got %s and %s"
                         % (n + 1, entries, tuple(transpose[0].shape), tuple(transpose[1].shape)))


def _segment_offsets(segments, n, k):
    """The host offsets [B + 1] of `segments` as int32, checked: 0 first, n last, ascending, every segment of at least k rows."""
    if isinstance(segments, torch.Tensor):
        segments = segments.detach().cpu().numpy()
    seg = np.ascontiguousarray(np.asarray(segments).reshape(-1), dtype=np.int64)
    if seg.shape[0] < 2 or seg[0] != 0 or seg[-1] != n:
        raise ValueError("segments must be offsets [B + 1] with segments[0] = 0 and segments[B] = %d rows" % n)
    length = np.diff(seg)
    if (length < 0).any():
        raise ValueError("segments must ascend")
    if (length < k).any():
        b = int(np.argmax(length < k))
        raise ValueError("segment %d has %d rows, fewer than k = %d" % (b, int(length[b]), k))
    return seg.astype(np.int32)


def knn(X, k, queries=None, segments=None, self_first=None, return_mean=False, cand_slices=0, form="difference",
        return_fallback=False):
    """The k nearest rows of X [n, F] for every row of `queries` [nq, F] (None: for every row of X itself), by the squared
    Euclidean distance d2(i, j) = sum_c (Q[i, c] - X[j, c])^2 in float32 -- the difference form, so identical rows are at
    exactly 0 and integer-valued rows give exact distances.  Returns (idx int32 [nq, k], dist float32 [nq, k]) and, with
    return_mean, mean float32 [nq]: row i lists its k smallest candidates under the total order (d2, j) -- the smaller
    distance first, the smaller index among equal distances -- ascending; mean[i] is the mean of sqrt(d2(i, j)) over every
    candidate of row i, itself included (HGNN's avg_dis).  One bit pattern on every call and for every cand_slices (mean:
    for a given cand_slices).  The N x N matrix is never formed: the peak allocation is the outputs and
    hg_knn_workspace_bytes, O(nq k).

    self_first (default: queries is None): row i's own index comes first, (i, 0.0), even where a duplicate row has a
    smaller index -- HGNN's "the centre is always in its own hyperedge".  segments: host offsets [B + 1] into the rows
    (0 first, n last, ascending): row i competes with the rows of its own segment only -- many point sets in one tensor;
    the call then waits for the stream once.  cand_slices: 0 (1 or 2, picked from nq and n) or 1 .. 32 slices of the
    candidates per query tile, merged by a second kernel; more slices fill the device when nq is small.

    form: "difference" (the default) is the search above.  "dot" (hg_knn_dot_f32, for wide rows) returns the same idx and
    dist, bit for bit, for the same arguments: the dot form |q|^2 + |x|^2 - 2 q.x on the f32 matrix unit only shortlists
    32 ceil((k + 16) / 32) candidates per row, the difference form ranks them, an error bound certifies row by row that
    nothing outside the shortlist could have entered the top k, and a row that is not certified is searched exhaustively
    in the difference form (include/hg_aggr.h has the bound).  dist never holds a dot-form estimate.  Under "dot" the
    mean is another number: mean[i] = the float32 mean over all candidates of sqrt(max(d~(i, j), 0)) with d~ the dot-form
    estimate and the self pair exactly 0 when queries is None -- within mean_j sqrt(E1(i)) + the float32 summation error
    of the float64 mean, E1 = hg_aggr.h's bound on |d~ - d2|; one bit pattern per (form, cand_slices).  "dot" takes no
    segments and rows of at most 65536 columns, and neither waits nor reads back.  return_fallback: one more result,
    int32 [nq], 1 where the row was not certified and took the exhaustive path, else 0 (all 0 under "difference").

    bfloat16 rows: form="dot" takes a bfloat16 X (queries, where given, bfloat16 too; hg_knn_dot_bf16).  idx and dist
    (float32, never an estimate, never rounded) are what knn(X.float(), ..., form="difference") returns, bit for bit, for
    the same arguments; the prefilter runs on the bf16 matrix unit under its own bound E1b (include/hg_aggr.h), mean is
    the mean of those estimates, and everything else above holds.  Under every other form bfloat16 is refused.

    Not differentiable: raises if X (or queries) requires a gradient while grad mode is on; call it under
    torch.no_grad() or on X.detach().  Refusals, in this order and before a device is touched: TypeError for anything
    but float32 (or, under form="dot", bfloat16 for X and queries alike); ValueError for an unknown form, for k outside
    1 .. min(64, n), for segments or self_first together with queries, for form="dot" with segments or with F above
    65536, for a segment shorter than k; RuntimeError for CPU tensors."""
    bf16 = form == "dot" and isinstance(X, torch.Tensor) and X.dtype == torch.bfloat16
    if bf16:
        if queries is not None and not (isinstance(queries, torch.Tensor) and queries.dtype == torch.bfloat16):
            raise TypeError("queries must be a bfloat16 tensor where X is one (X and queries are both float32 or both "
                            "bfloat16), got %s" % getattr(queries, "dtype", type(queries)))
    else:
        _check_dtype(X, "X", torch.float32, _KNN_NO_FORM)
        if queries is not None:
            _check_dtype(queries, "queries", torch.float32, _KNN_NO_FORM)
    if X.dim() != 2 or X.shape[1] < 1:
        raise ValueError("X must be [n, F] with F >= 1, got %s" % (tuple(X.shape),))
    n, F = X.shape
    if form not in FORMS:
        raise ValueError("form must be one of %s, got %r" % (", ".join(repr(f) for f in FORMS), form))
    if not isinstance(k, numbers.Integral) or isinstance(k, bool) or not 1 <= k <= K_MAX:
        raise ValueError("k must be an integer in 1 .. %d, got %r" % (K_MAX, k))
    if k > n:
        raise ValueError("k = %d exceeds the %d rows of X" % (k, n))
    if queries is not None:
        if segments is not None:
            raise ValueError("segments cannot be combined with queries (a segment is a range of rows of X itself)")
        if self_first:
            raise ValueError("self_first cannot be combined with queries (a query row is no candidate)")
        if queries.dim() != 2 or queries.shape[1] != F or queries.shape[0] < 1:
            raise ValueError("queries must be [nq >= 1, F = %d], got %s" % (F, tuple(queries.shape)))
    if form == "dot":
        if segments is not None:
            raise ValueError('form="dot" cannot be combined with segments (batches of point sets have narrow rows: use '
                             'form="difference")')
        if F > DOT_F_MAX:
            raise ValueError('form="dot" takes rows of at most %d columns (the width its error bound is derived for), got '
                             "F = %d" % (DOT_F_MAX, F))
    seg = None if segments is None else _segment_offsets(segments, n, k)
    if not isinstance(cand_slices, numbers.Integral) or isinstance(cand_slices, bool) or not 0 <= cand_slices <= SLICES_MAX:
        raise ValueError("cand_slices must be 0 (auto) or 1 .. %d, got %r" % (SLICES_MAX, cand_slices))
    if torch.is_grad_enabled() and (X.requires_grad or (queries is not None and queries.requires_grad)):
        raise RuntimeError("knn is not differentiable: call it under torch.no_grad() or on X.detach()")
    _check_feat(X, "X", bf16_ok=bf16)
    if queries is not None:
        _check_feat(queries, "queries", device=X.device, bf16_ok=bf16)
    if self_first is None:
        self_first = queries is None
    Q = X if queries is None else queries
    nq, k, cand_slices = Q.shape[0], int(k), int(cand_slices)
    dev = X.device
    L = _lib.lib()
    idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
    dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
    mean = torch.empty(nq, dtype=torch.float32, device=dev) if return_mean else None
    if form == "dot":
        fallback = torch.empty(nq, dtype=torch.int32, device=dev) if return_fallback else None
        if bf16 and not hasattr(L, "hg_knn_dot_bf16"):
            raise RuntimeError("this build of libhgaggr has no hg_knn_dot_bf16 (bfloat16 rows under form=\"dot\")")
        entry, sizes = ((L.hg_knn_dot_bf16, L.hg_knn_dot_bf16_workspace_bytes) if bf16 else
                        (L.hg_knn_dot_f32, L.hg_knn_dot_workspace_bytes))
        ws_bytes = sizes(nq, n, F, k, cand_slices)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(entry(_ptr(Q), nq, _ptr(X), n, F, k, 1 if self_first else 0, cand_slices, _ptr(idx), _ptr(dist),
                             _ptr(mean), _ptr(fallback), _ptr(ws), ws_bytes, _stream_handle(dev)))
    else:
        ws_bytes = L.hg_knn_workspace_bytes(nq, n, F, k, cand_slices)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        seg_ptr = None if seg is None else seg.ctypes.data_as(ctypes.c_void_p)
        with torch.cuda.device(dev):
            _lib.check(L.hg_knn_f32(_ptr(Q), nq, _ptr(X), n, F, k, seg_ptr, 0 if seg is None else seg.shape[0] - 1,
                                    1 if self_first else 0, cand_slices, _ptr(idx), _ptr(dist), _ptr(mean), _ptr(ws), ws_bytes,
                                    _stream_handle(dev)))
        fallback = torch.zeros(nq, dtype=torch.int32, device=dev) if return_fallback else None
    out = (idx, dist) + ((mean,) if return_mean else ()) + ((fallback,) if return_fallback else ())
    return out


def knn_incidence_weights(dist, mean, m_prob=1.0):
    """HGNN's probabilistic incidence entries exp(-dist / (m_prob * mean[:, None])^2) of knn's (dist [nq, k], already
    squared; mean [nq]), flattened to [nq * k]: aligned with the H_T positions of HyperGraph.from_knn, so it is what
    incidence_aggr takes as v2e_weight and e2v_weight.  Plain torch."""
    if dist.dim() != 2 or mean.dim() != 1 or mean.shape[0] != dist.shape[0]:
        raise ValueError("dist must be [nq, k] and mean [nq], got %s and %s" % (tuple(dist.shape), tuple(mean.shape)))
    return torch.exp(-dist / (m_prob * mean[:, None]) ** 2).reshape(-1)


def incidence_from_knn(idx, name="knn"):
    """The hypergraph of a neighbour table idx [N, k] (host, integer): hyperedge i = the k neighbours of vertex i, so
    M = N, csrptr = arange(0, N k + 1, k) and colind = idx flattened, in idx's order."""
    idx = np.asarray(idx)
    if idx.ndim != 2 or idx.shape[1] < 1:
        raise ValueError("idx must be [N, k], got %s" % (idx.shape,))
    N, k = idx.shape
    if idx.size and (idx.min() < 0 or idx.max() >= N):
        raise ValueError("idx must hold row numbers in 0 .. %d" % (N - 1))
    return Incidence(N, N, np.arange(0, N * k + 1, k, dtype=np.int64), idx.reshape(-1), name)


# ---- aggregation over the neighbour table itself, no plan (include/hg_aggr.h, hg_table_*) ---------------------------------

def _table_shape(idx):
    """The first phase of a neighbour table's check, with the caller's other TypeErrors: the dtype."""
    _check_dtype(idx, "idx", torch.int32, " [rows, k] (ops.knn's table)")


def _table_shape_values(idx):
    """The second phase: (rows, k), with the shape and k checked (ValueError)."""
    if idx.dim() != 2 or idx.shape[0] < 1:
        raise ValueError("idx must be [rows >= 1, k], got %s" % (tuple(idx.shape),))
    rows, k = idx.shape
    if not 1 <= k <= K_MAX:
        raise ValueError("k must be in 1 .. %d, got idx of %s" % (K_MAX, tuple(idx.shape)))
    if rows * k >= 2 ** 31:
        raise ValueError("rows * k must be below 2^31, got %d x %d" % (rows, k))
    return rows, k


def _check_table_index(t, name):
    if not t.is_cuda:
        raise RuntimeError("%s must be on a GPU (no CPU fallback in this backend)" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)


def knn_transpose(idx, n=None):
    """The transpose of a neighbour table idx [rows, k] (int32, ops.knn's) over n vertices (default: rows), on the device:
    (ptr_v int32 [n + 1], pos_v int32 [rows * k]).  pos_v[ptr_v[v] : ptr_v[v + 1]] are the positions p = i * k + s with
    idx[i, s] == v in ascending p -- the stable sort of the positions by vertex, so hyperedge p // k and slot p % k come
    from the position and pos_v indexes a weight [rows * k] directly.  An entry outside 0 .. n - 1 is ignored: ptr_v[n] is
    the number of valid entries and pos_v is unspecified from there on.  Nothing is read back and nothing waits.
    Refusals, before a device is touched: TypeError for anything but int32, ValueError for the shape, k or n, RuntimeError
    for a CPU tensor."""
    _table_shape(idx)
    rows, k = _table_shape_values(idx)
    if n is None:
        n = rows
    if not isinstance(n, numbers.Integral) or isinstance(n, bool) or not 1 <= n < 2 ** 31 - 1:
        raise ValueError("n must be a positive integer, got %r" % (n,))
    _check_table_index(idx, "idx")
    n = int(n)
    dev = idx.device
    L = _lib.lib()
    ptr_v = torch.empty(n + 1, dtype=torch.int32, device=dev)
    pos_v = torch.empty(rows * k, dtype=torch.int32, device=dev)
    ws_bytes = L.hg_table_transpose_workspace_bytes(rows, k, n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.hg_table_transpose(_ptr(idx), rows, k, n, _ptr(ptr_v), _ptr(pos_v), _ptr(ws), ws_bytes,
                                        _stream_handle(dev)))
    return ptr_v, pos_v


def _flat_or_none(t, name, count, dev):
    """A float32 device tensor of `count` elements (any shape) as the kernels take it, or None."""
    if t is None:
        return None
    _check_feat(t, name, device=dev)
    if t.numel() != count:
        raise ValueError("%s must have %d elements, got %s" % (name, count, tuple(t.shape)))
    return t


def table_gather(idx, src, w=None, src_scale=None, dst_scale=None, ctr=None):
    """dst[i] = dst_scale[i] * sum_s (src[idx[i, s]] * src_scale[idx[i, s]]) * w[i * k + s] over a table idx [rows, k] and rows
    src [n, F]: hg_table_gather_f32, every row summed in ascending s.  Any of w [rows * k], src_scale [n], dst_scale [rows]
    may be None (no multiplication).  An entry outside 0 .. n - 1 adds nothing.  No gradient.
    ctr [rows, F]: the difference gather hg_table_gather_diff_f32 -- the term starts from ctr[i] - src[idx[i, s]]."""
    _table_shape(idx)
    rows, k = _table_shape_values(idx)
    _check_table_index(idx, "idx")
    _check_feat(src, "src", device=idx.device)
    if src.dim() != 2 or src.shape[0] < 1 or src.shape[1] < 1:
        raise ValueError("src must be [n >= 1, F >= 1], got %s" % (tuple(src.shape),))
    n, F = src.shape
    dev = idx.device
    w = _flat_or_none(w, "w", rows * k, dev)
    src_scale = _flat_or_none(src_scale, "src_scale", n, dev)
    dst_scale = _flat_or_none(dst_scale, "dst_scale", rows, dev)
    ctr = _flat_or_none(ctr, "ctr", rows * F, dev)
    dst = torch.empty((rows, F), dtype=torch.float32, device=dev)
    L = _lib.lib()
    entry, centre = (L.hg_table_gather_f32, ()) if ctr is None else (L.hg_table_gather_diff_f32, (_ptr(ctr),))
    with torch.cuda.device(dev):
        _lib.check(entry(_ptr(idx), rows, k, n, F, _ptr(src), _ptr(w), _ptr(src_scale), _ptr(dst_scale), *centre, _ptr(dst),
                         _stream_handle(dev)))
    return dst


def table_gather_t(ptr_v, pos_v, k, src, w=None, src_scale=None, dst_scale=None, ctr=None):
    """dst[v] = dst_scale[v] * sum_q (src[pos_v[q] // k] * src_scale[pos_v[q] // k]) * w[pos_v[q]], q over ptr_v[v] ..
    ptr_v[v + 1] - 1, for the transpose (ptr_v [n + 1], pos_v [rows * k]) of a table of k columns and rows src [rows, F]:
    hg_table_gather_t_f32.  A row of at most TABLE_SEQ_MAX entries is summed in ascending q; a longer one by its whole
    workgroup in an order fixed by its length and F.  A vertex with no entry is +0.0 whatever dst_scale.  No gradient.
    ctr [n, F]: the difference gather hg_table_gather_t_diff_f32 -- the term starts from ctr[v] - src[pos_v[q] // k]."""
    _check_dtype(ptr_v, "ptr_v", torch.int32)
    _check_dtype(pos_v, "pos_v", torch.int32)
    if not isinstance(k, numbers.Integral) or isinstance(k, bool) or not 1 <= k <= K_MAX:
        raise ValueError("k must be an integer in 1 .. %d, got %r" % (K_MAX, k))
    if ptr_v.dim() != 1 or ptr_v.shape[0] < 2 or pos_v.dim() != 1:
        raise ValueError("ptr_v must be [n + 1] and pos_v [rows * k], got %s and %s" % (tuple(ptr_v.shape), tuple(pos_v.shape)))
    _check_table_index(ptr_v, "ptr_v")
    _check_table_index(pos_v, "pos_v")
    dev = ptr_v.device
    _check_feat(src, "src", device=dev)
    if src.dim() != 2 or src.shape[0] < 1 or src.shape[1] < 1 or src.shape[0] * int(k) != pos_v.shape[0]:
        raise ValueError("src must be [rows, F >= 1] with rows * k = %d positions, got %s" % (pos_v.shape[0], tuple(src.shape)))
    rows, F = src.shape
    n = ptr_v.shape[0] - 1
    w = _flat_or_none(w, "w", rows * int(k), dev)
    src_scale = _flat_or_none(src_scale, "src_scale", rows, dev)
    dst_scale = _flat_or_none(dst_scale, "dst_scale", n, dev)
    ctr = _flat_or_none(ctr, "ctr", n * F, dev)
    dst = torch.empty((n, F), dtype=torch.float32, device=dev)
    L = _lib.lib()
    entry, centre = (L.hg_table_gather_t_f32, ()) if ctr is None else (L.hg_table_gather_t_diff_f32, (_ptr(ctr),))
    with torch.cuda.device(dev):
        _lib.check(entry(_ptr(ptr_v), _ptr(pos_v), rows, int(k), n, F, _ptr(src), _ptr(w), _ptr(src_scale), _ptr(dst_scale),
                         *centre, _ptr(dst), _stream_handle(dev)))
    return dst


def table_dot(idx, A, B, a_scale=None, C=None, D=None):
    """out[i * k + s] = a_scale[j] * <A[j], B[i]> + <C[j], D[i]>, j = idx[i, s], over a table idx [rows, k]: hg_table_dot_f32,
    one launch and no [rows * k, F] array.  A, C [n, F]; B, D [rows, F]; a_scale [n] or None; C and D both or neither.  An
    entry outside 0 .. n - 1 gives +0.0.  The order of the sum is include/hg_aggr.h's DOT ORDER.  No gradient."""
    _table_shape(idx)
    rows, k = _table_shape_values(idx)
    _check_table_index(idx, "idx")
    dev = idx.device
    if (C is None) != (D is None):
        raise ValueError("C and D must both be given or both be None")
    _check_feat(A, "A", device=dev)
    if A.dim() != 2 or A.shape[0] < 1 or A.shape[1] < 1:
        raise ValueError("A must be [n >= 1, F >= 1], got %s" % (tuple(A.shape),))
    n, F = A.shape
    for name, t, shape in (("B", B, (rows, F)), ("C", C, (n, F)), ("D", D, (rows, F))):
        if t is not None:
            _check_feat(t, name, device=dev)
            if tuple(t.shape) != shape:
                raise ValueError("%s must be [%d, %d], got %s" % (name, shape[0], shape[1], tuple(t.shape)))
    a_scale = _flat_or_none(a_scale, "a_scale", n, dev)
    out = torch.empty(rows * k, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().hg_table_dot_f32(_ptr(idx), rows, k, n, F, _ptr(A), _ptr(a_scale), _ptr(B), _ptr(C), _ptr(D),
                                               _ptr(out), _stream_handle(dev)))
    return out


class _KnnDist(torch.autograd.Function):
    """dist[i, s] = |Q[i] - X[idx[i, s]]|^2 over a fixed table; the gradients are the two difference gathers with g = 2 dDist.
    Saves the table, its transpose and the inputs X and Q -- nothing new of rows * k * F elements."""

    @staticmethod
    def forward(ctx, X, Q, idx, ptr_v, pos_v):
        rows, k = idx.shape
        n, F = X.shape
        Qr = X if Q is None else Q
        dist = torch.empty((rows, k), dtype=torch.float32, device=X.device)
        with torch.cuda.device(X.device):
            _lib.check(_lib.lib().hg_table_dist_f32(_ptr(idx), rows, k, n, F, _ptr(Qr), _ptr(X), _ptr(dist),
                                                    _stream_handle(X.device)))
        ctx.same = Q is None
        ctx.save_for_backward(X, Qr, idx, ptr_v, pos_v)
        return dist

    @staticmethod
    def backward(ctx, dDist):
        X, Q, idx, ptr_v, pos_v = ctx.saved_tensors
        g = (dDist * 2.0).contiguous()  # exact: the factor of d (q - x)^2 folded into the weight
        dX = dQ = None
        if ctx.needs_input_grad[0]:
            dX = table_gather_t(ptr_v, pos_v, idx.shape[1], Q, g, ctr=X)
        if ctx.same:
            if ctx.needs_input_grad[0]:
                dX = dX + table_gather(idx, X, g, ctr=X)
        elif ctx.needs_input_grad[1]:
            dQ = table_gather(idx, X, g, ctr=Q)
        return dX, dQ, None, None, None


def knn_dist(idx, X, queries=None, transpose=None):
    """The squared distances of a GIVEN neighbour table, differentiable: dist float32 [rows, k] with dist[i, s] =
    sum_c (Q[i, c] - X[idx[i, s], c])^2, Q = `queries` [rows, F] or X itself (None; then rows = n).  The sum runs in ops.knn's
    order (include/hg_aggr.h, hg_table_dist_f32), so for the idx that ops.knn(X, k) returned -- under either form, with
    self_first, with queries -- it is the dist ops.knn returned, bit for bit.  An entry of idx outside 0 .. n - 1 gives +0.0.
    The search stays non-differentiable; over a fixed table this is the true gradient wherever the selection does not
    change (almost everywhere):  with g = 2 dDist, dQ[i] = sum_s (Q[i] - X[idx[i, s]]) g[i, s] and dX[j] =
    sum_{(i, s): idx[i, s] = j} (X[j] - Q[i]) g[i, s] -- the difference gathers hg_table_gather_diff_f32 /
    hg_table_gather_t_diff_f32, in the gathers' documented order, no atomics: two calls give the same bits, and identical
    rows (every self_first entry) contribute exactly 0.  With queries None the two are added with one torch add.
    transpose: the (ptr_v, pos_v) of ops.knn_transpose(idx, n) to reuse; computed when X needs a gradient and it is None.
    float32 only.  Refusals, in this order and before a device is touched: TypeError for an idx (ptr_v, pos_v) that is not
    int32 and an X or queries that is not float32; ValueError for the shapes and k; RuntimeError for CPU tensors."""
    _table_shape(idx)
    _check_dtype(X, "X", torch.float32, _NO_FORM % "knn_dist")
    if queries is not None:
        _check_dtype(queries, "queries", torch.float32, _NO_FORM % "knn_dist")
    _check_transpose_types(transpose)
    rows, k = _table_shape_values(idx)
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be [n >= 1, F >= 1], got %s" % (tuple(X.shape),))
    n, F = X.shape
    if queries is None:
        if rows != n:
            raise ValueError("without queries idx must have one row per row of X: %d rows, X has %d" % (rows, n))
    elif tuple(queries.shape) != (rows, F):
        raise ValueError("queries must be [rows, F] = [%d, %d], got %s" % (rows, F, tuple(queries.shape)))
    _check_transpose_shapes(transpose, n, rows * k)
    _check_table_index(idx, "idx")
    _check_feat(X, "X", device=idx.device)
    if queries is not None:
        _check_feat(queries, "queries", device=idx.device)
    ptr_v = pos_v = None
    if torch.is_grad_enabled() and X.requires_grad:
        if transpose is None:
            transpose = knn_transpose(idx, n)
        ptr_v, pos_v = transpose
        _check_table_index(ptr_v, "ptr_v")
        _check_table_index(pos_v, "pos_v")
    return _KnnDist.apply(X, queries, idx, ptr_v, pos_v)


class _KnnAggr(torch.autograd.Function):
    """Y = degV . H_w (degE . (H_w^T X)) over a neighbour table; the gradient of X is the same two gathers swapped.  Saves the
    table, its transpose, the weight and the scales -- nothing of rows * F elements.  Where the weight asks for its gradient,
    dw[p = (i, s)] = degV[v] <dY[v], Xe[i]> + <X[v], G[i]>, v = idx[i, s], one launch of hg_table_dot_f32: Xe is computed
    again in the backward, and the input X is saved as well."""

    @staticmethod
    def forward(ctx, X, w, idx, ptr_v, pos_v, degE, degV):
        Xe = table_gather(idx, X, w, None, degE)
        Y = table_gather_t(ptr_v, pos_v, idx.shape[1], Xe, w, None, degV)
        ctx.save_for_backward(idx, ptr_v, pos_v, w, degE, degV, *((X,) if ctx.needs_input_grad[1] else ()))
        return Y

    @staticmethod
    def backward(ctx, dY):
        idx, ptr_v, pos_v, w, degE, degV = ctx.saved_tensors[:6]
        dY = dY.contiguous()
        G = table_gather(idx, dY, w, degV, degE)
        dX = table_gather_t(ptr_v, pos_v, idx.shape[1], G, w) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            X = ctx.saved_tensors[6]
            Xe = table_gather(idx, X, w, None, degE)
            dw = table_dot(idx, dY, Xe, degV, X, G).view(w.shape)
        return dX, dw, None, None, None, None, None


def knn_aggr(idx, X, weight=None, degE=None, degV=None, transpose=None, weight_grad=False):
    """Y = degV . H_w (degE . (H_w^T X)) over the hypergraph of a neighbour table idx [rows, k] (int32, ops.knn's: hyperedge
    i = the vertices idx[i, :]) and features X [n, F] (float32), with no plan and no host step: two launches of the table
    gathers (include/hg_aggr.h, hg_table_gather_f32 / hg_table_gather_t_f32) and, where `transpose` is None, the transpose.
    weight [rows * k] or [rows, k] weights entry (i, s) in both hops, as HGNNAggrIncidence(hyperg, Z, w, w, ..) does for a
    probabilistic kNN hypergraph (ops.knn_incidence_weights); degE [rows] or [rows, 1] scales the hyperedges, degV [n] or
    [n, 1] the vertices; each may be None (no multiplication).  transpose: the (ptr_v, pos_v) of ops.knn_transpose(idx, n)
    to reuse.  The gradient of X is exact: G = table_gather(dY, src_scale=degV, dst_scale=degE, w), dX = table_gather_t(G,
    w).  weight, degE and degV get no gradient -- kNN weights come from detached distances -- and one that requires a
    gradient is refused.  Deterministic: the order of every sum is hg_aggr.h's, two calls give the same bits.
    weight_grad=True: `weight` may require a gradient (degE and degV are still refused), and gets
    dw[p = (i, s)] = degV[v] <dY[v], Xe[i]> + <X[v], G[i]>, v = idx[i, s], Xe = table_gather(X, w, dst_scale=degE) computed
    again in the backward -- one launch of hg_table_dot_f32, no [rows * k, F] array, no atomics.  Y and dX keep the bits of
    the default call; the backward then also keeps X, an input.
    Refusals, in this order and before a device is touched: TypeError for an idx (ptr_v, pos_v) that is not int32 and for
    an X, weight, degE or degV that is not float32; ValueError for the shapes and k; RuntimeError for a weight, degE or
    degV that requires a gradient, and for CPU tensors."""
    _table_shape(idx)
    _check_dtype(X, "X", torch.float32, _NO_FORM % "knn_aggr")
    scales = (("weight", weight), ("degE", degE), ("degV", degV))
    for name, t in scales:
        if t is not None:
            _check_dtype(t, name, torch.float32)
    _check_transpose_types(transpose)
    rows, k = _table_shape_values(idx)
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be [n >= 1, F >= 1], got %s" % (tuple(X.shape),))
    n = X.shape[0]
    if weight is not None and tuple(weight.shape) not in ((rows * k,), (rows, k)):
        raise ValueError("weight must be [rows * k] = [%d] or [rows, k] = [%d, %d], got %s" % (rows * k, rows, k, tuple(weight.shape)))
    for name, t, count in (("degE", degE, rows), ("degV", degV, n)):
        if t is not None and tuple(t.shape) not in ((count,), (count, 1)):
            raise ValueError("%s must be [%d] or [%d, 1], got %s" % (name, count, count, tuple(t.shape)))
    _check_transpose_shapes(transpose, n, rows * k)
    if torch.is_grad_enabled():
        for name, t in scales:
            if t is not None and t.requires_grad and not (weight_grad and name == "weight"):
                raise RuntimeError("%s gets no gradient from knn_aggr: pass %s.detach()" % (name, name))
    _check_table_index(idx, "idx")
    _check_feat(X, "X", device=idx.device)
    for name, t in scales:
        if t is not None:
            _check_feat(t, name, device=idx.device)
    if transpose is None:
        transpose = knn_transpose(idx, n)
    ptr_v, pos_v = transpose
    _check_table_index(ptr_v, "ptr_v")
    _check_table_index(pos_v, "pos_v")
    w, degE, degV = (None if t is None else t.detach() for _, t in scales)
    if weight_grad and weight is not None and weight.requires_grad:
        w = weight  # the one scale whose gradient is wanted
    return _KnnAggr.apply(X, w, idx, ptr_v, pos_v, degE, degV)


class KnnHypergraph:
    """The hypergraph "each vertex and its k - 1 nearest neighbours" as a device-only object: what HyperGraph.from_knn builds,
    without the read-back, the host transpose and the plan.  Nothing here reads a tensor back; with segments=None nothing
    waits for the device either (ops.knn waits once for its segment offsets).
      idx [N, k], dist [N, k] (squared), mean [N]: ops.knn(X, k, self_first=True, return_mean=True)
      ptr_v [N + 1], pos_v [N k]: ops.knn_transpose(idx)
      degE [N, 1] = 1 / k and degV [N, 1] = in-degree^-1/2, 1 where no hyperedge names the vertex (HyperGraph's formulas)
      weights(m_prob, X=None): HGNN's exp(-d2 / (m_prob mean)^2) entries [N k].  With X (the rows the table was built
        from, attached to the graph) d2 is ops.knn_dist(idx, X) -- the same bits as `dist`, with a gradient into X; `mean`
        stays detached: its gradient is an N x N sum and HGNN treats avg_dis as a constant of the construction.
      aggregate(Z, probabilistic=False, m_prob=1.0, X=None): ops.knn_aggr over the table; X goes to weights, and the
        weights then get their gradient (weight_grad=True).
    form: ops.knn's -- "dot" gives the same idx and dist through the matrix-unit prefilter, and its own mean.  Under "dot" X
    may be bfloat16: the table, dist, mean, transpose and degrees are int32 / float32 as always; aggregate, ops.knn_aggr and
    ops.knn_dist stay float32 only."""

    @classmethod
    def build(cls, X, k, segments=None, form="difference"):
        self = cls.__new__(cls)
        if isinstance(X, torch.Tensor):  # anything else is ops.knn's refusal
            X = X.detach().contiguous()
        self.idx, self.dist, self.mean = knn(X, k, segments=segments, self_first=True, return_mean=True, form=form)
        N = self.idx.shape[0]
        self.k, self.num_nodes, self.num_edges, self.nnz = int(k), N, N, N * int(k)
        self.device = self.idx.device
        self.ptr_v, self.pos_v = knn_transpose(self.idx, N)
        self.degE = torch.full((N, 1), 1.0 / int(k), dtype=torch.float32, device=self.device)
        deg = (self.ptr_v[1:] - self.ptr_v[:-1]).to(torch.float32).reshape(N, 1)
        self.degV = torch.where(deg > 0, deg.pow(-0.5), torch.ones_like(deg))
        return self

    def weights(self, m_prob=1.0, X=None):
        if X is None:
            return knn_incidence_weights(self.dist, self.mean, m_prob)
        return knn_incidence_weights(knn_dist(self.idx, X, transpose=(self.ptr_v, self.pos_v)), self.mean, m_prob)

    def aggregate(self, Z, probabilistic=False, m_prob=1.0, X=None):
        w = self.weights(m_prob, X) if probabilistic else None
        return knn_aggr(self.idx, Z, w, self.degE, self.degV, transpose=(self.ptr_v, self.pos_v), weight_grad=X is not None)


def table_seq_max():
    """HG_TABLE_SEQ_MAX of the library as built: the longest row one lane group sums in ascending order."""
    return int(_lib.lib().hg_table_seq_max())
