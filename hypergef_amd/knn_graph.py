"""k-nearest-neighbour hypergraph construction (include/hg_aggr.h, hg_knn_f32): the hyperedges of HGNN's ModelNet40 /
NTU2012 hypergraphs and of DHGNN's layers, "each vertex and its k nearest neighbours in feature space", found on the
device without the N x N distance matrix.

`knn` and `knn_incidence_weights` are exported as `ops.knn` / `ops.knn_incidence_weights`; `incidence_from_knn` is the
host-side layout step of `HyperGraph.from_knn`.

`knn_transpose` and `knn_aggr` (`ops.knn_transpose` / `ops.knn_aggr`; hg_table_* in include/hg_aggr.h) aggregate over the
neighbour table itself, with no plan and no host step, and `KnnHypergraph` is the device-only hypergraph they serve.
`knn_gather` (`ops.knn_gather`) is one hop over the table with a choice of sum, mean, max or min (hg_table_reduce_* /
hg_table_select_*: the comparison kernels and their exact gradient), and `knn_aggr(first=, second=)` composes two of them.
`knn_dist` (`ops.knn_dist`) gives a table's distances with a gradient, and `knn_aggr(weight_grad=True)` the gradient of its
weights: together they train through the weights of a probabilistic kNN hypergraph.  Both take bfloat16 rows under
Options.incidence_bf16 = 'rows' (hg_table_*_bf16): the float32 call on the widened rows, bit for bit, rounded once.
`knn_softmax` (`ops.knn_softmax`; hg_table_softmax_*) turns scores into attention coefficients over the table, per hyperedge
or per vertex, with exact gradients: its alpha is `knn_aggr`'s weight.  Several heads (hg_table_*_heads_f32): `knn_softmax(heads=H)` takes
scores with the head as their last dimension, and `knn_aggr` a weight [rows, k, H]; every head in the same launch and with the
single-head call's bits.  `knn_softmax(dropout=p)` drops coefficients inside the softmax launch and its backward
(hg_table_softmax_dropout_*_heads_f32): a Philox mask that is never stored.
`knn_attention_aggr` (`ops.knn_attention_aggr`; hg_table_attention_*) is `knn_aggr` on `knn_softmax`'s alpha in one call, bit
for bit, without alpha: two statistics per segment and head, and every coefficient formed inside the gather that uses it.
`knn_dot_attention_aggr` (`ops.knn_dot_attention_aggr`; hg_table_dot_attention_*) is dot-product attention under the hyperedge
group: logits <query[i], X[j]>, the row softmax and hop 0 in one walk per (row, head), every member row loaded once.
"""
import ctypes
import numbers

import numpy as np
import torch

from . import _lib
from .plan import _check_feat, _ptr, _rng_state_device, _rng_state_dtype, _rng_state_length, _stream_handle
from .synth import Incidence

K_MAX = 64        # include/hg_aggr.h: k in 1 .. 64
SLICES_MAX = 32   # cand_slices in 0 .. 32
FORMS = ("difference", "dot", "dot_split")
DOT_F_MAX = 65536  # form="dot" and "dot_split": the widest rows the error bound is derived for (hg_knn.h, kDotMaxF)


_NO_FORM = " (%s has no float16 / float64 form; bfloat16 rows need Options.incidence_bf16 = 'rows')"
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
        return_fallback=False, set_rows=None):
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

    form="dot_split" (hg_knn_dot_split_f32; float32 rows only): "dot" with the prefilter's sums on the bf16 matrix unit.  Every
    element is split into two bfloat16 parts in registers, q = qh + ql + a remainder below 2^-16 |q|, and the estimate sums
    qh.xh + qh.xl + ql.xh, three bf16 instructions per 16 columns in place of eight f32 ones.  idx and dist are form=
    "difference"'s for the same arguments, bit for bit, on every input, and dist never holds an estimate: the looser estimate
    only shortlists, under its own bound E1s (include/hg_aggr.h).  queries, self_first, cand_slices, return_fallback and
    return_mean behave as under "dot"; mean is this form's own, the float32 mean over all candidates of sqrt(max(d~, 0)) of its
    estimates -- within mean_j sqrt(E1s(i)) + the float32 summation error of the float64 mean, one bit pattern per cand_slices.
    It neither waits nor reads back; it takes no segments, no set_rows and rows of at most 65536 columns.

    set_rows = m: X is B = n / m point sets of exactly m consecutive rows each -- the batch of equal-sized point clouds of
    DGCNN / DHGNN -- and row i competes with rows (i // m) * m .. (i // m) * m + m - 1 only (hg_knn_sets_f32,
    hg_knn_dot_sets_f32 / _bf16).  No offsets exist, on the host or on the device: the call neither waits nor reads back
    under either form and is recorded by torch.cuda.graph.  idx holds row numbers of X, as segments gives them.  idx and
    dist are those of knn(X, k, segments=range(0, n + 1, m), form="difference") bit for bit, for the same self_first
    and cand_slices, under "difference", under "dot" and under "dot" on bfloat16 rows (then: of the call on X.float());
    m = n is the call without set_rows.  mean: under "difference" the segments call's bits; under "dot" the mean over the
    row's own set of sqrt(max(d~, 0)), the number above with n replaced by m.  Under "dot" every set is searched as a
    problem of its own -- kp = min(m, 32 ceil((k + 16) / 32)), the certificate against the largest norm of the row's own
    set, the exhaustive path over the set -- so a set far from the origin costs the others nothing; a set of fewer than
    128 rows still takes a whole 128-row workgroup of the prefilter.

    Not differentiable: raises if X (or queries) requires a gradient while grad mode is on; call it under
    torch.no_grad() or on X.detach().  Refusals, in this order and before a device is touched: TypeError for anything
    but float32 (or, under form="dot", bfloat16 for X and queries alike); ValueError for an unknown form, for k outside
    1 .. min(64, n), for segments or self_first together with queries, for form="dot" or "dot_split" with segments, "dot_split" with
    set_rows, either with F above 65536, for a segment shorter than k, for cand_slices, and then for set_rows: not an integer, k above it, n no
    multiple of it, together with queries or with segments; RuntimeError for CPU tensors."""
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
    if form in ("dot", "dot_split"):
        if segments is not None:
            raise ValueError('form="%s" cannot be combined with segments (batches of point sets have narrow rows: use '
                             'form="difference")' % form)
        if form == "dot_split" and set_rows is not None:
            raise ValueError('form="dot_split" cannot be combined with set_rows (uniform sets are searched under "difference" '
                             'and "dot")')
        if F > DOT_F_MAX:
            raise ValueError('form="%s" takes rows of at most %d columns (the width its error bound is derived for), got '
                             "F = %d" % (form, DOT_F_MAX, F))
    seg = None if segments is None else _segment_offsets(segments, n, k)
    if not isinstance(cand_slices, numbers.Integral) or isinstance(cand_slices, bool) or not 0 <= cand_slices <= SLICES_MAX:
        raise ValueError("cand_slices must be 0 (auto) or 1 .. %d, got %r" % (SLICES_MAX, cand_slices))
    if set_rows is not None:
        if not isinstance(set_rows, numbers.Integral) or isinstance(set_rows, bool):
            raise ValueError("set_rows must be an integer (the rows of every point set), got %r" % (set_rows,))
        if not k <= set_rows:
            raise ValueError("k = %d exceeds the set_rows = %d rows of a set" % (k, set_rows))
        if n % set_rows:
            raise ValueError("the %d rows of X are no multiple of set_rows = %d" % (n, set_rows))
        if queries is not None:
            raise ValueError("set_rows cannot be combined with queries (a set is a range of rows of X itself)")
        if segments is not None:
            raise ValueError("set_rows cannot be combined with segments (uniform sets need no offsets)")
        set_rows = int(set_rows)
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
    if set_rows is not None:  # the sets entries: X alone, no offsets
        if not hasattr(L, "hg_knn_sets_f32"):
            raise RuntimeError("this build of libhgaggr has no hg_knn_sets_f32 (set_rows)")
        if form == "dot":
            fallback = torch.empty(nq, dtype=torch.int32, device=dev) if return_fallback else None
            entry = L.hg_knn_dot_sets_bf16 if bf16 else L.hg_knn_dot_sets_f32
            ws_bytes = L.hg_knn_dot_sets_workspace_bytes(n, F, k, cand_slices, set_rows)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                _lib.check(entry(_ptr(X), n, F, k, set_rows, 1 if self_first else 0, cand_slices, _ptr(idx), _ptr(dist),
                                 _ptr(mean), _ptr(fallback), _ptr(ws), ws_bytes, _stream_handle(dev)))
        else:
            ws_bytes = L.hg_knn_workspace_bytes(n, n, F, k, cand_slices)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
            with torch.cuda.device(dev):
                _lib.check(L.hg_knn_sets_f32(_ptr(X), n, F, k, set_rows, 1 if self_first else 0, cand_slices, _ptr(idx),
                                             _ptr(dist), _ptr(mean), _ptr(ws), ws_bytes, _stream_handle(dev)))
            fallback = torch.zeros(nq, dtype=torch.int32, device=dev) if return_fallback else None
    elif form in ("dot", "dot_split"):
        fallback = torch.empty(nq, dtype=torch.int32, device=dev) if return_fallback else None
        if bf16 and not hasattr(L, "hg_knn_dot_bf16"):
            raise RuntimeError("this build of libhgaggr has no hg_knn_dot_bf16 (bfloat16 rows under form=\"dot\")")
        if form == "dot_split" and not hasattr(L, "hg_knn_dot_split_f32"):
            raise RuntimeError("this build of libhgaggr has no hg_knn_dot_split_f32 (form=\"dot_split\")")
        entry, sizes = ((L.hg_knn_dot_bf16, L.hg_knn_dot_bf16_workspace_bytes) if bf16 else
                        (L.hg_knn_dot_split_f32, L.hg_knn_dot_workspace_bytes) if form == "dot_split" else
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


def _flat_or_none(t, name, count, dev, bf16_ok=False):
    """A float32 device tensor of `count` elements (any shape) as the kernels take it, or None."""
    if t is None:
        return None
    _check_feat(t, name, device=dev, bf16_ok=bf16_ok)
    if t.numel() != count:
        raise ValueError("%s must have %d elements, got %s" % (name, count, tuple(t.shape)))
    return t


BF16 = torch.bfloat16


def _bf16_entry(name):
    """An hg_table_*_bf16 entry of the library; a build without it is an error, never another path."""
    L = _lib.lib()
    if not hasattr(L, name):
        raise RuntimeError("this build of libhgaggr has no %s (bfloat16 rows over a neighbour table)" % name)
    return getattr(L, name)


def _heads_entry(name):
    """An hg_table_*_heads_f32 entry of the library; a build without it is an error, never another path."""
    L = _lib.lib()
    if not hasattr(L, name):
        raise RuntimeError("this build of libhgaggr has no %s (several heads over a neighbour table)" % name)
    return getattr(L, name)


def _heads_value(heads):
    """heads as the kernels take it: an integer >= 1 (ValueError)."""
    if isinstance(heads, bool) or not isinstance(heads, numbers.Integral) or heads < 1:
        raise ValueError("heads must be an integer >= 1, got %r" % (heads,))
    return int(heads)


def _whole_lanes(F, *rows):
    """Whether the hg_table_*_bf16 entries take these row arrays (None: absent): F % 8 == 0 and 16-byte aligned rows
    (include/hg_aggr.h).  Otherwise the caller widens, runs the float32 entry and rounds once: the same bits, torch ops only."""
    return F % 8 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in rows)


def _heads_rows(F, heads, w, io, ctr):
    """What the several-heads gathers refuse beyond the plain ones' refusals."""
    if io or ctr is not None:
        raise TypeError("heads=%d takes float32 rows and no ctr (hg_table_gather_heads_f32 has no bfloat16 or difference form)" % heads)
    if w is None:
        raise ValueError("heads=%d needs w [rows * k, heads] (without weights the heads are the plain gather)" % heads)
    if F % heads:
        raise ValueError("F = %d is no multiple of heads = %d" % (F, heads))


def _gather_io(src, ctr, dst_dtype):
    """The row types of one gather: (the io mask, or 0 for the float32 entry; the result's dtype), with the refusals."""
    if dst_dtype not in (None, torch.float32, BF16):
        raise TypeError("dst_dtype must be torch.float32 or torch.bfloat16, got %s" % (dst_dtype,))
    if ctr is not None and ctr.dtype != src.dtype:
        raise TypeError("ctr must have src's dtype %s, got %s" % (src.dtype, ctr.dtype))
    if src.dtype == BF16:
        if dst_dtype == BF16:
            raise ValueError("bfloat16 src gives a float32 result (the hyperedge rows between the hops stay float32)")
        return _lib.HG_ROWS_SRC_BF16, torch.float32
    if dst_dtype == BF16:
        if ctr is not None:
            raise ValueError("the difference gather has no bfloat16 result: its float32 sums are added before the one rounding")
        return _lib.HG_ROWS_DST_BF16, BF16
    return 0, torch.float32


def _widened(t):
    return t.float() if t is not None and t.dtype == BF16 else t


def table_gather(idx, src, w=None, src_scale=None, dst_scale=None, ctr=None, dst_dtype=None, heads=1):
    """dst[i] = dst_scale[i] * sum_s (src[idx[i, s]] * src_scale[idx[i, s]]) * w[i * k + s] over a table idx [rows, k] and rows
    src [n, F]: hg_table_gather_f32, every row summed in ascending s.  Any of w [rows * k], src_scale [n], dst_scale [rows]
    may be None (no multiplication).  An entry outside 0 .. n - 1 adds nothing.  No gradient.
    ctr [rows, F]: the difference gather hg_table_gather_diff_f32 -- the term starts from ctr[i] - src[idx[i, s]].
    bfloat16 rows (hg_table_gather_bf16): a bfloat16 src (ctr bfloat16 too) gives the float32 result of the call on
    src.float(); dst_dtype=torch.bfloat16 rounds a float32 src's result once (no ctr).  Bit for bit; w and the scales stay
    float32.
    heads = H > 1 (hg_table_gather_heads_f32): w [rows * k, H] (never None) and column c is weighted by w[p, c // (F // H)];
    float32 rows only, no ctr."""
    _table_shape(idx)
    rows, k = _table_shape_values(idx)
    _check_table_index(idx, "idx")
    _check_feat(src, "src", device=idx.device, bf16_ok=True)
    if src.dim() != 2 or src.shape[0] < 1 or src.shape[1] < 1:
        raise ValueError("src must be [n >= 1, F >= 1], got %s" % (tuple(src.shape),))
    n, F = src.shape
    dev = idx.device
    w = _flat_or_none(w, "w", rows * k * heads, dev)
    src_scale = _flat_or_none(src_scale, "src_scale", n, dev)
    dst_scale = _flat_or_none(dst_scale, "dst_scale", rows, dev)
    ctr = _flat_or_none(ctr, "ctr", rows * F, dev, bf16_ok=True)
    io, out_dtype = _gather_io(src, ctr, dst_dtype)
    dst = torch.empty((rows, F), dtype=out_dtype, device=dev)
    if heads > 1:
        _heads_rows(F, heads, w, io, ctr)
        with torch.cuda.device(dev):
            _lib.check(_heads_entry("hg_table_gather_heads_f32")(_ptr(idx), rows, k, n, F, heads, _ptr(src), _ptr(w), _ptr(src_scale),
                                                                 _ptr(dst_scale), _ptr(dst), _stream_handle(dev)))
        return dst
    if io and not _whole_lanes(F, src, ctr, dst):
        return table_gather(idx, _widened(src), w, src_scale, dst_scale, _widened(ctr)).to(out_dtype)
    L = _lib.lib()
    if io:
        entry, tail = _bf16_entry("hg_table_gather_bf16"), (_ptr(ctr), _ptr(dst), io)
    elif ctr is None:
        entry, tail = L.hg_table_gather_f32, (_ptr(dst),)
    else:
        entry, tail = L.hg_table_gather_diff_f32, (_ptr(ctr), _ptr(dst))
    with torch.cuda.device(dev):
        _lib.check(entry(_ptr(idx), rows, k, n, F, _ptr(src), _ptr(w), _ptr(src_scale), _ptr(dst_scale), *tail,
                         _stream_handle(dev)))
    return dst


def table_gather_t(ptr_v, pos_v, k, src, w=None, src_scale=None, dst_scale=None, ctr=None, dst_dtype=None, heads=1):
    """dst[v] = dst_scale[v] * sum_q (src[pos_v[q] // k] * src_scale[pos_v[q] // k]) * w[pos_v[q]], q over ptr_v[v] ..
    ptr_v[v + 1] - 1, for the transpose (ptr_v [n + 1], pos_v [rows * k]) of a table of k columns and rows src [rows, F]:
    hg_table_gather_t_f32.  A row of at most TABLE_SEQ_MAX entries is summed in ascending q; a longer one by its whole
    workgroup in an order fixed by its length and F.  A vertex with no entry is +0.0 whatever dst_scale.  No gradient.
    ctr [n, F]: the difference gather hg_table_gather_t_diff_f32 -- the term starts from ctr[v] - src[pos_v[q] // k].
    bfloat16 rows (hg_table_gather_t_bf16): as table_gather; a long row keeps the float32 call's order, so its bits too.
    heads = H > 1 (hg_table_gather_t_heads_f32): as table_gather; a long row keeps the plain call's order at the same F."""
    _check_dtype(ptr_v, "ptr_v", torch.int32)
    _check_dtype(pos_v, "pos_v", torch.int32)
    if not isinstance(k, numbers.Integral) or isinstance(k, bool) or not 1 <= k <= K_MAX:
        raise ValueError("k must be an integer in 1 .. %d, got %r" % (K_MAX, k))
    if ptr_v.dim() != 1 or ptr_v.shape[0] < 2 or pos_v.dim() != 1:
        raise ValueError("ptr_v must be [n + 1] and pos_v [rows * k], got %s and %s" % (tuple(ptr_v.shape), tuple(pos_v.shape)))
    _check_table_index(ptr_v, "ptr_v")
    _check_table_index(pos_v, "pos_v")
    dev = ptr_v.device
    _check_feat(src, "src", device=dev, bf16_ok=True)
    if src.dim() != 2 or src.shape[0] < 1 or src.shape[1] < 1 or src.shape[0] * int(k) != pos_v.shape[0]:
        raise ValueError("src must be [rows, F >= 1] with rows * k = %d positions, got %s" % (pos_v.shape[0], tuple(src.shape)))
    rows, F = src.shape
    n = ptr_v.shape[0] - 1
    w = _flat_or_none(w, "w", rows * int(k) * heads, dev)
    src_scale = _flat_or_none(src_scale, "src_scale", rows, dev)
    dst_scale = _flat_or_none(dst_scale, "dst_scale", n, dev)
    ctr = _flat_or_none(ctr, "ctr", n * F, dev, bf16_ok=True)
    io, out_dtype = _gather_io(src, ctr, dst_dtype)
    dst = torch.empty((n, F), dtype=out_dtype, device=dev)
    if heads > 1:
        _heads_rows(F, heads, w, io, ctr)
        with torch.cuda.device(dev):
            _lib.check(_heads_entry("hg_table_gather_t_heads_f32")(_ptr(ptr_v), _ptr(pos_v), rows, int(k), n, F, heads, _ptr(src),
                                                                   _ptr(w), _ptr(src_scale), _ptr(dst_scale), _ptr(dst),
                                                                   _stream_handle(dev)))
        return dst
    if io and not _whole_lanes(F, src, ctr, dst):
        return table_gather_t(ptr_v, pos_v, k, _widened(src), w, src_scale, dst_scale, _widened(ctr)).to(out_dtype)
    L = _lib.lib()
    if io:
        entry, tail = _bf16_entry("hg_table_gather_t_bf16"), (_ptr(ctr), _ptr(dst), io)
    elif ctr is None:
        entry, tail = L.hg_table_gather_t_f32, (_ptr(dst),)
    else:
        entry, tail = L.hg_table_gather_t_diff_f32, (_ptr(ctr), _ptr(dst))
    with torch.cuda.device(dev):
        _lib.check(entry(_ptr(ptr_v), _ptr(pos_v), rows, int(k), n, F, _ptr(src), _ptr(w), _ptr(src_scale), _ptr(dst_scale),
                         *tail, _stream_handle(dev)))
    return dst


def table_dot(idx, A, B, a_scale=None, C=None, D=None, heads=1):
    """out[i * k + s] = a_scale[j] * <A[j], B[i]> + <C[j], D[i]>, j = idx[i, s], over a table idx [rows, k]: hg_table_dot_f32,
    one launch and no [rows * k, F] array.  A, C [n, F]; B, D [rows, F]; a_scale [n] or None; C and D both or neither.  An
    entry outside 0 .. n - 1 gives +0.0.  The order of the sum is include/hg_aggr.h's DOT ORDER.  No gradient.
    A (and C with it) may be bfloat16 (hg_table_dot_bf16): out is the float32 call's on A.float() / C.float(), bit for bit;
    B, D and a_scale stay float32.
    heads = H > 1 (hg_table_dot_heads_f32): out [rows * k, H], out[p, h] the call on head h's F // H columns; float32 only."""
    _table_shape(idx)
    rows, k = _table_shape_values(idx)
    _check_table_index(idx, "idx")
    dev = idx.device
    if (C is None) != (D is None):
        raise ValueError("C and D must both be given or both be None")
    _check_feat(A, "A", device=dev, bf16_ok=True)
    if C is not None and isinstance(C, torch.Tensor) and C.dtype != A.dtype:
        raise TypeError("C must have A's dtype %s, got %s" % (A.dtype, C.dtype))
    if A.dim() != 2 or A.shape[0] < 1 or A.shape[1] < 1:
        raise ValueError("A must be [n >= 1, F >= 1], got %s" % (tuple(A.shape),))
    n, F = A.shape
    for name, t, shape in (("B", B, (rows, F)), ("C", C, (n, F)), ("D", D, (rows, F))):
        if t is not None:
            _check_feat(t, name, device=dev, bf16_ok=name == "C")
            if tuple(t.shape) != shape:
                raise ValueError("%s must be [%d, %d], got %s" % (name, shape[0], shape[1], tuple(t.shape)))
    a_scale = _flat_or_none(a_scale, "a_scale", n, dev)
    if heads > 1:
        if A.dtype == BF16:
            raise TypeError("heads=%d takes float32 rows (hg_table_dot_heads_f32 has no bfloat16 form)" % heads)
        if F % heads:
            raise ValueError("F = %d is no multiple of heads = %d" % (F, heads))
        out = torch.empty((rows * k, heads), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_heads_entry("hg_table_dot_heads_f32")(_ptr(idx), rows, k, n, F, heads, _ptr(A), _ptr(a_scale), _ptr(B), _ptr(C),
                                                              _ptr(D), _ptr(out), _stream_handle(dev)))
        return out
    if A.dtype == BF16 and not _whole_lanes(F, A, B, C, D):
        return table_dot(idx, A.float(), B, a_scale, _widened(C), D)
    entry = _bf16_entry("hg_table_dot_bf16") if A.dtype == BF16 else _lib.lib().hg_table_dot_f32
    out = torch.empty(rows * k, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(entry(_ptr(idx), rows, k, n, F, _ptr(A), _ptr(a_scale), _ptr(B), _ptr(C), _ptr(D), _ptr(out),
                         _stream_handle(dev)))
    return out


class _KnnDist(torch.autograd.Function):
    """dist[i, s] = |Q[i] - X[idx[i, s]]|^2 over a fixed table; the gradients are the two difference gathers with g = 2 dDist.
    Saves the table, its transpose and the inputs X and Q -- nothing new of rows * k * F elements.
    bfloat16 X (and Q): dist and both difference gathers are float32 -- those of the widened rows -- and dX (with Q None
    the float32 sum of the two gathers) and dQ are rounded once."""

    @staticmethod
    def forward(ctx, X, Q, idx, ptr_v, pos_v):
        rows, k = idx.shape
        n, F = X.shape
        Qr = X if Q is None else Q
        dist = torch.empty((rows, k), dtype=torch.float32, device=X.device)
        bf16 = X.dtype == BF16
        Xk, Qk = (X.float(), Qr.float()) if bf16 and not _whole_lanes(F, X, Qr) else (X, Qr)
        entry = _bf16_entry("hg_table_dist_bf16") if Xk.dtype == BF16 else _lib.lib().hg_table_dist_f32
        with torch.cuda.device(X.device):
            _lib.check(entry(_ptr(idx), rows, k, n, F, _ptr(Qk), _ptr(Xk), _ptr(dist), _stream_handle(X.device)))
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
            dQ = table_gather(idx, X, g, ctr=Q).to(Q.dtype)
        if dX is not None:
            dX = dX.to(X.dtype)  # bfloat16 rows: the one rounding, after the float32 add
        return dX, dQ, None, None, None


def _rows_bf16(X, options):
    """Whether X is a bfloat16 tensor that the caller's options (Options.incidence_bf16 = 'rows') let through."""
    from . import ops
    return ops._opt(options).incidence_bf16 == "rows" and isinstance(X, torch.Tensor) and X.dtype == BF16


def knn_dist(idx, X, queries=None, transpose=None, options=None):
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
    bfloat16 rows: under Options.incidence_bf16 = 'rows' (options=, resolved as every operator resolves it) X may be
    bfloat16, and queries with it -- both or neither (hg_table_dist_bf16).  dist stays float32 and is knn_dist on X.float(),
    bit for bit, so for the idx of ops.knn(Xb, k, form="dot") it is the dist that call returned; dX and dQ are the float32
    call's, rounded once (with queries None after the one float32 add).  By default bfloat16 is refused.
    Refusals, in this order and before a device is touched: TypeError for an idx (ptr_v, pos_v) that is not int32 and an X
    or queries that is not float32 (or, under the option, bfloat16 for both alike); ValueError for the shapes and k;
    RuntimeError for CPU tensors."""
    bf16 = _rows_bf16(X, options)
    _table_shape(idx)
    if bf16:
        if queries is not None and not (isinstance(queries, torch.Tensor) and queries.dtype == BF16):
            raise TypeError("queries must be a bfloat16 tensor where X is one (X and queries are both float32 or both "
                            "bfloat16), got %s" % getattr(queries, "dtype", type(queries)))
    else:
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
    _check_feat(X, "X", device=idx.device, bf16_ok=bf16)
    if queries is not None:
        _check_feat(queries, "queries", device=idx.device, bf16_ok=bf16)
    ptr_v = pos_v = None
    if torch.is_grad_enabled() and X.requires_grad:
        if transpose is None:
            transpose = knn_transpose(idx, n)
        ptr_v, pos_v = transpose
        _check_table_index(ptr_v, "ptr_v")
        _check_table_index(pos_v, "pos_v")
    return _KnnDist.apply(X, queries, idx, ptr_v, pos_v)


# ---- one hop over the table with a choice of reduction (hg_table_reduce_* / hg_table_select_*) -------------------------------

REDUCES = ("sum", "mean", "max", "min")
HOPS = ("hyperedge", "vertex")
_OPS = {"max": _lib.HG_REDUCE_MAX, "min": _lib.HG_REDUCE_MIN}


def _reduce_entry(name):
    """An hg_table_reduce_* / hg_table_select_* entry of the library; a build without it is an error, never another path."""
    L = _lib.lib()
    if not hasattr(L, name):
        raise RuntimeError("this build of libhgaggr has no %s (max / min over a neighbour table)" % name)
    return getattr(L, name)


def table_reduce(idx, src, op, dst_scale=None, want_arg=True):
    """(dst [rows, F], arg int32 [rows, F] or None): the greatest (op 'max') or smallest ('min') src[idx[i, s], c] over s, times
    dst_scale[i], and the winner's position i k + s -- hg_table_reduce_f32 and its total order.  No checks, no gradient."""
    rows, k = idx.shape
    n, F = src.shape
    dst = torch.empty((rows, F), dtype=torch.float32, device=src.device)
    arg = torch.empty((rows, F), dtype=torch.int32, device=src.device) if want_arg else None
    with torch.cuda.device(src.device):
        _lib.check(_reduce_entry("hg_table_reduce_f32")(_ptr(idx), rows, k, n, F, _OPS[op], _ptr(src), _ptr(dst_scale), _ptr(dst),
                                                        _ptr(arg), _stream_handle(src.device)))
    return dst, arg


def table_reduce_t(ptr_v, pos_v, k, src, op, dst_scale=None, want_arg=True):
    """The same over a vertex's hyperedges, through the transpose: (dst [n, F], arg [n, F] or None) of src [rows, F] --
    hg_table_reduce_t_f32.  A vertex with no entry is +0.0 and arg -1."""
    rows, F = src.shape
    n = ptr_v.shape[0] - 1
    dst = torch.empty((n, F), dtype=torch.float32, device=src.device)
    arg = torch.empty((n, F), dtype=torch.int32, device=src.device) if want_arg else None
    with torch.cuda.device(src.device):
        _lib.check(_reduce_entry("hg_table_reduce_t_f32")(_ptr(ptr_v), _ptr(pos_v), rows, int(k), n, F, _OPS[op], _ptr(src),
                                                          _ptr(dst_scale), _ptr(dst), _ptr(arg), _stream_handle(src.device)))
    return dst, arg


def table_select(idx, gs, arg):
    """dsrc [rows, F] of table_reduce_t's src: row i sums gs[idx[i, s]] where arg[idx[i, s]] is the position i k + s, ascending
    s (hg_table_select_f32).  gs and arg are [n, F]."""
    rows, k = idx.shape
    n, F = gs.shape
    dsrc = torch.empty((rows, F), dtype=torch.float32, device=gs.device)
    with torch.cuda.device(gs.device):
        _lib.check(_reduce_entry("hg_table_select_f32")(_ptr(idx), rows, k, n, F, _ptr(gs), _ptr(arg), _ptr(dsrc),
                                                        _stream_handle(gs.device)))
    return dsrc


def table_select_t(ptr_v, pos_v, k, gs, arg):
    """dsrc [n, F] of table_reduce's src: vertex v sums gs[p // k] over its positions p that won their row, in table_gather_t's
    order (hg_table_select_t_f32).  gs and arg are [rows, F]."""
    rows, F = gs.shape
    n = ptr_v.shape[0] - 1
    dsrc = torch.empty((n, F), dtype=torch.float32, device=gs.device)
    with torch.cuda.device(gs.device):
        _lib.check(_reduce_entry("hg_table_select_t_f32")(_ptr(ptr_v), _ptr(pos_v), rows, int(k), n, F, _ptr(gs), _ptr(arg),
                                                          _ptr(dsrc), _stream_handle(gs.device)))
    return dsrc


class _KnnGatherSum(torch.autograd.Function):
    """One sum hop over the table; the gradient is the other hop with the scale moved to the source side.  Saves the table,
    its transpose and the scale."""

    @staticmethod
    def forward(ctx, src, idx, ptr_v, pos_v, scale, to):
        ctx.to = to
        ctx.save_for_backward(idx, ptr_v, pos_v, scale)
        if to == "hyperedge":
            return table_gather(idx, src, None, None, scale)
        return table_gather_t(ptr_v, pos_v, idx.shape[1], src, None, None, scale)

    @staticmethod
    def backward(ctx, grad):
        idx, ptr_v, pos_v, scale = ctx.saved_tensors
        grad = grad.contiguous()
        if ctx.to == "hyperedge":
            dsrc = table_gather_t(ptr_v, pos_v, idx.shape[1], grad, None, scale)
        else:
            dsrc = table_gather(idx, grad, None, scale)
        return dsrc, None, None, None, None, None


class _KnnGatherReduce(torch.autograd.Function):
    """One max / min hop over the table.  Saves arg, the table, its transpose and the scale -- no source rows; the backward
    is the select kernel of the other walk on grad * scale."""

    @staticmethod
    def forward(ctx, src, idx, ptr_v, pos_v, scale, to, op):
        ctx.to = to
        if to == "hyperedge":
            dst, arg = table_reduce(idx, src, op, scale)
        else:
            dst, arg = table_reduce_t(ptr_v, pos_v, idx.shape[1], src, op, scale)
        ctx.save_for_backward(idx, ptr_v, pos_v, scale, arg)
        ctx.mark_non_differentiable(arg)
        return dst, arg

    @staticmethod
    def backward(ctx, grad, _):
        idx, ptr_v, pos_v, scale, arg = ctx.saved_tensors
        gs = (grad if scale is None else grad * scale[:, None]).contiguous()
        if ctx.to == "hyperedge":
            dsrc = table_select_t(ptr_v, pos_v, idx.shape[1], gs, arg)
        else:
            dsrc = table_select(idx, gs, arg)
        return dsrc, None, None, None, None, None, None


def knn_gather(idx, src, to="hyperedge", reduce="sum", scale=None, transpose=None, num_nodes=None, return_index=False):
    """One hop over a neighbour table idx [rows, k] (int32, ops.knn's) as an operator of its own, with no plan and no host step,
    differentiable in src.  to='hyperedge': src is [n, F] and dst[i] = scale[i] * reduce_s src[idx[i, s]], [rows, F];
    to='vertex': src is [rows, F] and dst[v] = scale[v] * reduce over the positions p with idx[p] == v of src[p // k], [n, F]
    with n = num_nodes (default: rows), through `transpose` = ops.knn_transpose(idx, n), computed where it is needed and not
    given.  scale: one float32 factor per row of dst ([count] or [count, 1]), or None; it gets no gradient.
    reduce: 'sum' is hg_table_gather_f32 / hg_table_gather_t_f32 bit for bit, and its gradient the other of the two with the
    scale on the source side.  'mean' runs the same kernels with dst_scale = scale * (1 / len) formed in float32 by torch, len
    = k for a hyperedge and the vertex's number of entries for a vertex (none: 0); nothing is read back.  'max' / 'min'
    (hg_table_reduce_f32 / hg_table_reduce_t_f32) take the greatest / smallest entry of every row and column under the total
    order (value, then the smaller position p = i k + s): -0.0 ties +0.0, a row of -inf has a winner, an entry outside
    0 .. n - 1 is no candidate, a row with no candidate is +0.0 whatever its scale, NaN is unspecified; every call gives the
    same bits.  Their gradient goes to the winner alone -- a duplicate entry gets it once -- through the select kernels
    (hg_table_select_*), no atomics; the node keeps arg, the table, its transpose and the scale, and no source rows.
    return_index=True (max / min only) returns (dst, arg), arg int32 the winner's position (-1: no candidate), not
    differentiable.  float32 only: no bfloat16 rows, no weights, no heads.
    Refusals, in this order and before a device is touched: TypeError for an idx (ptr_v, pos_v) that is not int32 and a src
    or scale that is not float32 (bfloat16 too, whatever Options.incidence_bf16 says); ValueError for an unknown to or
    reduce, for the shapes and k, for return_index with 'sum' / 'mean'; RuntimeError for a scale that requires a gradient
    and for CPU tensors."""
    _table_shape(idx)
    _check_dtype(src, "src", torch.float32, " (knn_gather has no bfloat16, float16 or float64 form)")
    if scale is not None:
        _check_dtype(scale, "scale", torch.float32)
    _check_transpose_types(transpose)
    if to not in HOPS:
        raise ValueError("to must be 'hyperedge' or 'vertex', got %r" % (to,))
    if reduce not in REDUCES:
        raise ValueError("reduce must be one of %s, got %r" % (", ".join(repr(r) for r in REDUCES), reduce))
    rows, k = _table_shape_values(idx)
    if src.dim() != 2 or src.shape[0] < 1 or src.shape[1] < 1:
        raise ValueError("src must be [%s, F >= 1], got %s" % ("n >= 1" if to == "hyperedge" else "rows", tuple(src.shape)))
    if to == "hyperedge":
        n, count = src.shape[0], rows
        if num_nodes is not None and num_nodes != n:
            raise ValueError("src has %d rows, num_nodes is %r" % (n, num_nodes))
    else:
        if src.shape[0] != rows:
            raise ValueError("to='vertex' takes one row of src per row of idx: %d rows, src has %d" % (rows, src.shape[0]))
        n = rows if num_nodes is None else num_nodes
        if not isinstance(n, numbers.Integral) or isinstance(n, bool) or not 1 <= n < 2 ** 31 - 1:
            raise ValueError("num_nodes must be a positive integer, got %r" % (num_nodes,))
        n = count = int(n)
    if scale is not None and tuple(scale.shape) not in ((count,), (count, 1)):
        raise ValueError("scale must be [%d] or [%d, 1], got %s" % (count, count, tuple(scale.shape)))
    _check_transpose_shapes(transpose, n, rows * k)
    if return_index and reduce not in _OPS:
        raise ValueError("return_index needs reduce='max' or 'min', got %r" % reduce)
    if torch.is_grad_enabled() and scale is not None and scale.requires_grad:
        raise RuntimeError("scale gets no gradient from knn_gather: pass scale.detach()")
    _check_table_index(idx, "idx")
    _check_feat(src, "src", device=idx.device)
    if scale is not None:
        _check_feat(scale, "scale", device=idx.device)
        scale = scale.detach().reshape(-1)
    needs_grad = torch.is_grad_enabled() and src.requires_grad
    ptr_v = pos_v = None
    if to == "vertex" or needs_grad:
        if transpose is None:
            transpose = knn_transpose(idx, n)
        ptr_v, pos_v = transpose
        _check_table_index(ptr_v, "ptr_v")
        _check_table_index(pos_v, "pos_v")
    if reduce in _OPS:
        if needs_grad:
            dst, arg = _KnnGatherReduce.apply(src, idx, ptr_v, pos_v, scale, to, reduce)
        elif to == "hyperedge":
            dst, arg = table_reduce(idx, src, reduce, scale, want_arg=return_index)
        else:
            dst, arg = table_reduce_t(ptr_v, pos_v, k, src, reduce, scale, want_arg=return_index)
        return (dst, arg) if return_index else dst
    if reduce == "mean":
        if to == "hyperedge":
            recip = torch.full((rows,), 1.0 / k, dtype=torch.float32, device=idx.device)
        else:
            recip = 1.0 / (ptr_v[1:] - ptr_v[:-1]).to(torch.float32).clamp(min=1.0)  # no entry: the kernels write +0.0 themselves
        scale = recip if scale is None else scale * recip
    if needs_grad:
        return _KnnGatherSum.apply(src, idx, ptr_v, pos_v, scale, to)
    if to == "hyperedge":
        return table_gather(idx, src, None, None, scale)
    return table_gather_t(ptr_v, pos_v, k, src, None, None, scale)


# ---- attention softmax over the table (hg_table_softmax_f32 / hg_table_softmax_bwd_f32 / hg_table_sum_f32) -------------------

_GROUPS = {"hyperedge": _lib.HG_TABLE_HYPEREDGE, "vertex": _lib.HG_TABLE_VERTEX}


def _softmax_entry(name):
    """An hg_table_softmax_* / hg_table_sum_f32 entry of the library; a build without it is an error, never another path."""
    L = _lib.lib()
    if not hasattr(L, name):
        raise RuntimeError("this build of libhgaggr has no %s (attention softmax over a neighbour table)" % name)
    return getattr(L, name)


def table_softmax(idx, n, group, node_score=None, edge_score=None, entry_score=None, slope=0.2, ptr_v=None, pos_v=None, heads=1):
    """alpha [rows, k] of hg_table_softmax_f32 over n vertices: the softmax over each hyperedge's members ('hyperedge') or each
    vertex's positions ('vertex', through ptr_v / pos_v) of leaky_relu((own + other) + entry).  No checks, no gradient.
    heads = H > 1: alpha [rows, k, H] of hg_table_softmax_heads_f32 on scores with the head as their last dimension."""
    rows, k = idx.shape
    if heads > 1:
        alpha = torch.empty((rows, k, heads), dtype=torch.float32, device=idx.device)
        with torch.cuda.device(idx.device):
            _lib.check(_heads_entry("hg_table_softmax_heads_f32")(_ptr(idx), rows, k, n, heads, _GROUPS[group], _ptr(node_score),
                                                                  _ptr(edge_score), _ptr(entry_score), slope, _ptr(ptr_v),
                                                                  _ptr(pos_v), _ptr(alpha), _stream_handle(idx.device)))
        return alpha
    alpha = torch.empty((rows, k), dtype=torch.float32, device=idx.device)
    with torch.cuda.device(idx.device):
        _lib.check(_softmax_entry("hg_table_softmax_f32")(_ptr(idx), rows, k, n, _GROUPS[group], _ptr(node_score), _ptr(edge_score),
                                                          _ptr(entry_score), slope, _ptr(ptr_v), _ptr(pos_v), _ptr(alpha),
                                                          _stream_handle(idx.device)))
    return alpha


def table_softmax_bwd(idx, n, group, alpha, dalpha, node_score=None, edge_score=None, entry_score=None, slope=0.2, ptr_v=None,
                      pos_v=None, want_group=True, heads=1):
    """(ds [rows, k], dgroup or None) of hg_table_softmax_bwd_f32: the gradient of every position's raw score and, per segment,
    its own sum -- [rows] for 'hyperedge', [n] for 'vertex'.  heads = H > 1: hg_table_softmax_bwd_heads_f32, one more dimension
    H at the end of each."""
    rows, k = idx.shape
    if heads > 1:
        ds = torch.empty((rows, k, heads), dtype=torch.float32, device=idx.device)
        nseg = rows if group == "hyperedge" else n
        dgroup = torch.empty((nseg, heads), dtype=torch.float32, device=idx.device) if want_group else None
        with torch.cuda.device(idx.device):
            _lib.check(_heads_entry("hg_table_softmax_bwd_heads_f32")(_ptr(idx), rows, k, n, heads, _GROUPS[group], _ptr(node_score),
                                                                      _ptr(edge_score), _ptr(entry_score), slope, _ptr(ptr_v),
                                                                      _ptr(pos_v), _ptr(alpha), _ptr(dalpha), _ptr(ds),
                                                                      _ptr(dgroup), _stream_handle(idx.device)))
        return ds, dgroup
    ds = torch.empty((rows, k), dtype=torch.float32, device=idx.device)
    dgroup = torch.empty(rows if group == "hyperedge" else n, dtype=torch.float32, device=idx.device) if want_group else None
    with torch.cuda.device(idx.device):
        _lib.check(_softmax_entry("hg_table_softmax_bwd_f32")(_ptr(idx), rows, k, n, _GROUPS[group], _ptr(node_score),
                                                              _ptr(edge_score), _ptr(entry_score), slope, _ptr(ptr_v), _ptr(pos_v),
                                                              _ptr(alpha), _ptr(dalpha), _ptr(ds), _ptr(dgroup),
                                                              _stream_handle(idx.device)))
    return ds, dgroup


def table_sum(idx, n, side, val, ptr_v=None, pos_v=None, heads=1):
    """out[seg] = the sum of val [rows, k] over the segment's candidates (hg_table_sum_f32): [rows] for 'hyperedge', [n] for
    'vertex' (through ptr_v / pos_v).  heads = H > 1: val [rows, k, H], out [segments, H] (hg_table_sum_heads_f32)."""
    rows, k = idx.shape
    if heads > 1:
        out = torch.empty((rows if side == "hyperedge" else n, heads), dtype=torch.float32, device=idx.device)
        with torch.cuda.device(idx.device):
            _lib.check(_heads_entry("hg_table_sum_heads_f32")(_ptr(idx), rows, k, n, heads, _GROUPS[side], _ptr(ptr_v), _ptr(pos_v),
                                                              _ptr(val), _ptr(out), _stream_handle(idx.device)))
        return out
    out = torch.empty(rows if side == "hyperedge" else n, dtype=torch.float32, device=idx.device)
    with torch.cuda.device(idx.device):
        _lib.check(_softmax_entry("hg_table_sum_f32")(_ptr(idx), rows, k, n, _GROUPS[side], _ptr(ptr_v), _ptr(pos_v), _ptr(val),
                                                      _ptr(out), _stream_handle(idx.device)))
    return out


def _head_shape(idx, heads, segments=None):
    """The shape of a per-position ([rows, k]) or per-segment array, with the head as one more dimension where heads > 1."""
    lead = tuple(idx.shape) if segments is None else (segments,)
    return lead + (heads,) if heads > 1 else lead


def table_softmax_dropout(idx, n, group, p_drop, rng_state, node_score=None, edge_score=None, entry_score=None, slope=0.2,
                          ptr_v=None, pos_v=None, heads=1):
    """(alpha, alpha after dropout) of hg_table_softmax_dropout_heads_f32, both [rows, k] or [rows, k, H]: table_softmax's alpha,
    bit for bit, and keep ? alpha / (1 - p_drop) : 0 for the Philox mask of rng_state (int64 [2] on the device, read by the
    kernel).  One launch for any heads >= 1.  No checks, no gradient."""
    rows, k = idx.shape
    alpha = torch.empty(_head_shape(idx, heads), dtype=torch.float32, device=idx.device)
    out = torch.empty_like(alpha)
    with torch.cuda.device(idx.device):
        _lib.check(_heads_entry("hg_table_softmax_dropout_heads_f32")(
            _ptr(idx), rows, k, n, heads, _GROUPS[group], _ptr(node_score), _ptr(edge_score), _ptr(entry_score), slope,
            float(p_drop), _ptr(rng_state), _ptr(ptr_v), _ptr(pos_v), _ptr(alpha), _ptr(out), _stream_handle(idx.device)))
    return alpha, out


def table_softmax_dropout_bwd(idx, n, group, p_drop, rng_state, alpha, dout, node_score=None, edge_score=None, entry_score=None,
                              slope=0.2, ptr_v=None, pos_v=None, want_group=True, heads=1):
    """(ds, dgroup or None) of hg_table_softmax_dropout_bwd_heads_f32: table_softmax_bwd on dalpha = keep ? dout / (1 - p_drop) : 0,
    the mask formed again from rng_state inside the launch."""
    rows, k = idx.shape
    ds = torch.empty(_head_shape(idx, heads), dtype=torch.float32, device=idx.device)
    nseg = rows if group == "hyperedge" else n
    dgroup = torch.empty(_head_shape(idx, heads, nseg), dtype=torch.float32, device=idx.device) if want_group else None
    with torch.cuda.device(idx.device):
        _lib.check(_heads_entry("hg_table_softmax_dropout_bwd_heads_f32")(
            _ptr(idx), rows, k, n, heads, _GROUPS[group], _ptr(node_score), _ptr(edge_score), _ptr(entry_score), slope,
            float(p_drop), _ptr(rng_state), _ptr(ptr_v), _ptr(pos_v), _ptr(alpha), _ptr(dout), _ptr(ds), _ptr(dgroup),
            _stream_handle(idx.device)))
    return ds, dgroup


class _KnnSoftmax(torch.autograd.Function):
    """alpha over a fixed table.  Saves alpha, the scores given, the table and its transpose; the backward is one launch of the
    backward kernel (ds and the own side's gradient) and, where the other end's score wants one, one segment sum over the
    other side.  heads = H > 1: the same launches on the several-heads entries.  p_drop > 0: dropout on alpha fused into both
    kernels -- returns keep ? alpha / (1 - p) : 0, saves the undropped alpha and the two words of rng_state, from which the
    backward launch forms the mask again."""

    @staticmethod
    def forward(ctx, node_score, edge_score, entry_score, idx, ptr_v, pos_v, group, slope, n, heads=1, p_drop=0.0, rng_state=None):
        ctx.group, ctx.slope, ctx.n, ctx.heads, ctx.p_drop = group, slope, n, heads, p_drop
        if p_drop > 0.0:
            alpha, out = table_softmax_dropout(idx, n, group, p_drop, rng_state, node_score, edge_score, entry_score, slope,
                                               ptr_v, pos_v, heads)
        else:
            alpha = out = table_softmax(idx, n, group, node_score, edge_score, entry_score, slope, ptr_v, pos_v, heads)
        ctx.save_for_backward(alpha, node_score, edge_score, entry_score, idx, ptr_v, pos_v, rng_state)
        return out

    @staticmethod
    def backward(ctx, dalpha):
        alpha, node_score, edge_score, entry_score, idx, ptr_v, pos_v, rng_state = ctx.saved_tensors
        hyperedge = ctx.group == "hyperedge"
        own, other = (1, 0) if hyperedge else (0, 1)  # positions of the two scores among the inputs
        if ctx.p_drop > 0.0:
            ds, dgroup = table_softmax_dropout_bwd(idx, ctx.n, ctx.group, ctx.p_drop, rng_state, alpha, dalpha.contiguous(),
                                                   node_score, edge_score, entry_score, ctx.slope, ptr_v, pos_v,
                                                   want_group=ctx.needs_input_grad[own], heads=ctx.heads)
        else:
            ds, dgroup = table_softmax_bwd(idx, ctx.n, ctx.group, alpha, dalpha.contiguous(), node_score, edge_score, entry_score,
                                           ctx.slope, ptr_v, pos_v, want_group=ctx.needs_input_grad[own], heads=ctx.heads)
        grads = [None, None, None]
        grads[own] = dgroup
        if ctx.needs_input_grad[other]:
            grads[other] = table_sum(idx, ctx.n, "vertex" if hyperedge else "hyperedge", ds, ptr_v, pos_v, ctx.heads)
        if ctx.needs_input_grad[2]:
            grads[2] = ds.view(entry_score.shape)
        return (*grads, None, None, None, None, None, None, None, None, None)


def knn_softmax(idx, node_score=None, edge_score=None, group="hyperedge", negative_slope=0.2, entry_score=None, transpose=None,
                num_nodes=None, heads=1, dropout=0.0, training=True, rng_state=None, return_rng_state=False):
    """Attention coefficients over a neighbour table idx [rows, k] (int32, ops.knn's), with no plan and no host step: alpha
    float32 [rows, k], the softmax over each group of leaky_relu(raw, negative_slope) with
        raw[i, s] = (own + other) + entry_score[i, s]
    group='hyperedge': a group is a table row, own = edge_score[i], other = node_score[idx[i, s]].  group='vertex': a group is
    the positions that name one vertex v (any number, through `transpose` = ops.knn_transpose(idx, n)), own = node_score[v],
    other = edge_score[i].  node_score [n], edge_score [rows], entry_score [rows, k] or [rows * k], float32; any may be None
    (no addition), not all.  n is node_score's length, else num_nodes, else rows.  ops.incidence_softmax's formula, operation
    for operation (hg_table_softmax_f32); alpha keeps the table's layout whichever the group, so it is ops.knn_aggr's weight.
    An entry of idx outside 0 .. n - 1 is no candidate: exactly +0.0, in alpha and in every gradient.
    Differentiable in the three scores, exactly: one launch of hg_table_softmax_bwd_f32 (ds, the gradient of entry_score, and
    its sum per group, the gradient of the group's own score) and one of hg_table_sum_f32 over the other side (the other
    end's).  The transpose is computed where it is needed and not given: for group='vertex', and for a node_score gradient
    under group='hyperedge'.  Deterministic: include/hg_aggr.h has the order of every sum, two calls give the same bits.
    Nothing waits, nothing is read back.  float32 only: no bfloat16 scores.
    heads = H > 1: ops.incidence_softmax's layout on the table -- node_score [n, H], edge_score [rows, H], entry_score
    [rows, k, H] or [rows * k, H], alpha [rows, k, H] -- every head in the same launch (hg_table_softmax_heads_f32; the
    gradients through hg_table_softmax_bwd_heads_f32 and hg_table_sum_heads_f32, one launch each as above).  alpha[..., h]
    and every gradient's column h are, bit for bit, the single-head call's on column h.  heads = 1 is the call above.
    dropout = p in (0, 1) with training=True: the coefficients after dropout, keep ? alpha / (1 - p) : 0, from the same
    launch (hg_table_softmax_dropout_heads_f32, any heads) -- no stored mask, no further pass; the gradients stay exact, the
    one backward launch (hg_table_softmax_dropout_bwd_heads_f32) forms the mask again.  rng_state: int64 [2] on idx's device,
    the {key, sid} of the Philox mask (keep depends on it, the table position i k + s and the head alone -- not on the
    group); None draws one with torch.randint on that device: it follows torch.manual_seed, costs no host synchronisation
    and, captured into a graph, gives every replay a new mask.  return_rng_state=True returns (coefficients, the state used
    -- None where no dropout ran).  dropout = 0.0 or training=False is the call above: the same code path, the same bits,
    torch's generator untouched.  Still nothing waits and nothing is read back.
    Refusals, in this order and before a device is touched: ValueError for a dropout outside [0, 1); TypeError for an idx
    (ptr_v, pos_v) that is not int32, a score that is not float32 (bfloat16 too, whatever Options.incidence_bf16 says) and an
    rng_state that is not int64; ValueError for an unknown group, for heads, for the shapes and k, for no score at all, for
    an rng_state of other than 2 elements; RuntimeError for CPU tensors and an rng_state off idx's device."""
    from .ops import _dropout_p  # ops imports this module
    p_drop = _dropout_p(dropout)
    if p_drop == 0.0 or not training:  # no dropout: the state is neither looked at nor drawn nor returned
        p_drop, rng_state = 0.0, None
    _table_shape(idx)
    scores = (("node_score", node_score), ("edge_score", edge_score), ("entry_score", entry_score))
    for name, t in scores:
        if t is not None:
            _check_dtype(t, name, torch.float32, " (knn_softmax has no bfloat16, float16 or float64 form)")
    _check_transpose_types(transpose)
    if rng_state is not None:
        _rng_state_dtype(rng_state)
    if group not in _GROUPS:
        raise ValueError("group must be 'hyperedge' or 'vertex', got %r" % (group,))
    H = _heads_value(heads)
    tail = (H,) if H > 1 else ()  # the head is the last dimension of every score
    rows, k = _table_shape_values(idx)
    if all(t is None for _, t in scores):
        raise ValueError("knn_softmax needs at least one of node_score, edge_score and entry_score")
    if node_score is not None:
        if node_score.dim() != 1 + len(tail) or node_score.shape[0] < 1 or tuple(node_score.shape[1:]) != tail:
            raise ValueError("node_score must be %s, got %s" % ("[n >= 1, heads = %d]" % H if tail else "[n >= 1]",
                                                                 tuple(node_score.shape)))
        n = node_score.shape[0]
        if num_nodes is not None and num_nodes != n:
            raise ValueError("node_score has %d elements, num_nodes is %r" % (n, num_nodes))
    else:
        n = rows if num_nodes is None else num_nodes
        if not isinstance(n, numbers.Integral) or isinstance(n, bool) or not 1 <= n < 2 ** 31 - 1:
            raise ValueError("num_nodes must be a positive integer, got %r" % (num_nodes,))
        n = int(n)
    if edge_score is not None and tuple(edge_score.shape) != (rows, *tail):
        raise ValueError("edge_score must be %s, got %s" % ("[rows, heads] = [%d, %d]" % (rows, H) if tail else "[rows] = [%d]" % rows,
                                                             tuple(edge_score.shape)))
    if entry_score is not None and tuple(entry_score.shape) not in ((rows, k, *tail), (rows * k, *tail)):
        want = "[rows, k, heads] = [%d, %d, %d] or [rows * k, heads] = [%d, %d]" % (rows, k, H, rows * k, H) if tail \
            else "[rows, k] = [%d, %d] or [rows * k] = [%d]" % (rows, k, rows * k)
        raise ValueError("entry_score must be %s, got %s" % (want, tuple(entry_score.shape)))
    _check_transpose_shapes(transpose, n, rows * k)
    if rng_state is not None:
        _rng_state_length(rng_state)
    _check_table_index(idx, "idx")
    for name, t in scores:
        if t is not None:
            _check_feat(t, name, device=idx.device)
    if rng_state is not None:
        _rng_state_device(rng_state, idx.device)
    grad = torch.is_grad_enabled()
    ptr_v = pos_v = None
    if group == "vertex" or (grad and node_score is not None and node_score.requires_grad):
        if transpose is None:
            transpose = knn_transpose(idx, n)
        ptr_v, pos_v = transpose
        _check_table_index(ptr_v, "ptr_v")
        _check_table_index(pos_v, "pos_v")
    slope = float(negative_slope)
    if p_drop > 0.0 and rng_state is None:  # on the device: no synchronisation, and a captured draw is drawn again by every replay
        info = torch.iinfo(torch.int64)  # randint's upper end is exclusive: every int64 but 2^63 - 1, which a key can spare
        rng_state = torch.randint(info.min, info.max, (2,), dtype=torch.int64, device=idx.device)
    if grad and any(t is not None and t.requires_grad for _, t in scores):
        out = _KnnSoftmax.apply(node_score, edge_score, entry_score, idx, ptr_v, pos_v, group, slope, n, H, p_drop, rng_state)
    elif p_drop > 0.0:  # nothing to differentiate: the operator itself, without the autograd node
        out = table_softmax_dropout(idx, n, group, p_drop, rng_state, node_score, edge_score, entry_score, slope, ptr_v, pos_v, H)[1]
    else:
        out = table_softmax(idx, n, group, node_score, edge_score, entry_score, slope, ptr_v, pos_v, H)
    return (out, rng_state) if return_rng_state else out


def _knn_aggr_reduced(idx, X, weight, degE, degV, transpose, first, second):
    """knn_aggr with a reduction other than the two sums: two knn_gather calls, degE the first hop's scale and degV the second's."""
    _table_shape(idx)
    _check_dtype(X, "X", torch.float32, " (knn_aggr with first / second other than 'sum' has no bfloat16 form)")
    scales = (("weight", weight), ("degE", degE), ("degV", degV))
    for name, t in scales:
        if t is not None:
            _check_dtype(t, name, torch.float32)
    _check_transpose_types(transpose)
    for name, r in (("first", first), ("second", second)):
        if r not in REDUCES:
            raise ValueError("%s must be one of %s, got %r" % (name, ", ".join(repr(x) for x in REDUCES), r))
    if weight is not None:
        raise ValueError("first=%r, second=%r take no weight (a comparison has no weighted form here, and the means keep the "
                         "sums' weights out as well)" % (first, second))
    rows, k = _table_shape_values(idx)
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be [n >= 1, F >= 1], got %s" % (tuple(X.shape),))
    n = X.shape[0]
    for name, t, count in (("degE", degE, rows), ("degV", degV, n)):
        if t is not None and tuple(t.shape) not in ((count,), (count, 1)):
            raise ValueError("%s must be [%d] or [%d, 1], got %s" % (name, count, count, tuple(t.shape)))
    _check_transpose_shapes(transpose, n, rows * k)
    if torch.is_grad_enabled():
        for name, t in scales:
            if t is not None and t.requires_grad:
                raise RuntimeError("%s gets no gradient from knn_aggr: pass %s.detach()" % (name, name))
    _check_table_index(idx, "idx")
    _check_feat(X, "X", device=idx.device)
    if transpose is None:
        transpose = knn_transpose(idx, n)
    Xe = knn_gather(idx, X, "hyperedge", first, degE, transpose)
    return knn_gather(idx, Xe, "vertex", second, degV, transpose, num_nodes=n)


def _weight_heads(idx, weight):
    """H of a knn_aggr weight: its last dimension where it is [rows * k, H] or [rows, k, H] with H > 1, else 1 (a weight of
    any other shape is the single-head call's to accept or refuse).  Looks at shapes only and raises nothing."""
    if not isinstance(idx, torch.Tensor) or not isinstance(weight, torch.Tensor) or idx.dim() != 2 or weight.dim() < 2:
        return 1
    rows, k = idx.shape
    lead, H = tuple(weight.shape[:-1]), weight.shape[-1]
    if H > 1 and lead in ((rows * k,), (rows, k)) and tuple(weight.shape) != (rows, k):
        return int(H)
    return 1


class _KnnAggr(torch.autograd.Function):
    """Y = degV . H_w (degE . (H_w^T X)) over a neighbour table; the gradient of X is the same two gathers swapped.  Saves the
    table, its transpose, the weight and the scales -- nothing of rows * F elements.  Where the weight asks for its gradient,
    dw[p = (i, s)] = degV[v] <dY[v], Xe[i]> + <X[v], G[i]>, v = idx[i, s], one launch of hg_table_dot_f32: Xe is computed
    again in the backward, and the input X is saved as well.
    bfloat16 X: Xe and G stay float32, Y and dX are rounded once in the second gather's store, dw (float32) comes from
    hg_table_dot_bf16 -- the float32 node on X.float() and dY.float(), bit for bit, with the same saved tensors.
    heads = H > 1: w [.., H]; the same gathers and the same dot on the several-heads entries, the same saved tensors."""

    @staticmethod
    def forward(ctx, X, w, idx, ptr_v, pos_v, degE, degV, heads=1):
        ctx.heads = heads
        Xe = table_gather(idx, X, w, None, degE, heads=heads)
        Y = table_gather_t(ptr_v, pos_v, idx.shape[1], Xe, w, None, degV, dst_dtype=X.dtype, heads=heads)
        ctx.save_for_backward(idx, ptr_v, pos_v, w, degE, degV, *((X,) if ctx.needs_input_grad[1] else ()))
        return Y

    @staticmethod
    def backward(ctx, dY):
        idx, ptr_v, pos_v, w, degE, degV = ctx.saved_tensors[:6]
        dY = dY.contiguous()
        H = ctx.heads
        G = table_gather(idx, dY, w, degV, degE, heads=H)
        dX = table_gather_t(ptr_v, pos_v, idx.shape[1], G, w, dst_dtype=dY.dtype, heads=H) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            X = ctx.saved_tensors[6]
            Xe = table_gather(idx, X, w, None, degE, heads=H)
            dw = table_dot(idx, dY, Xe, degV, X, G, heads=H).view(w.shape)
        return dX, dw, None, None, None, None, None, None


def knn_aggr(idx, X, weight=None, degE=None, degV=None, transpose=None, weight_grad=False, options=None, first="sum",
             second="sum"):
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
    bfloat16 rows: under Options.incidence_bf16 = 'rows' (options=, resolved as every operator resolves it) X may be
    bfloat16 (hg_table_gather_bf16 / hg_table_gather_t_bf16 / hg_table_dot_bf16).  Y and dX are bfloat16: the float32 call
    on X.float() (upstream dY.float()), rounded once; the hyperedge rows between the hops, dw and every sum stay float32,
    and so do weight, degE and degV whatever the option.  By default bfloat16 is refused.
    first / second ('sum', 'mean', 'max', 'min'): the reduction over a hyperedge's members / over a vertex's hyperedges.  With
    both at 'sum' the call is the one above, on its code path and with its bits.  Otherwise it is two ops.knn_gather calls,
    Xe = knn_gather(X, to='hyperedge', reduce=first, scale=degE) and Y = knn_gather(Xe, to='vertex', reduce=second,
    scale=degV): UniSAGE's mean / max and EdgeConv's max on the device table.  A weight then raises ValueError and bfloat16
    TypeError, whatever the option; the gradient of X is knn_gather's (max / min: to the winner alone).
    Several heads: a weight with one more dimension at its end, [rows * k, H] or [rows, k, H] with H > 1, is one weight per
    entry and head, and H is taken from it (the call has no argument of its own for it).  ops.incidence_aggr's layout on the
    table -- X [n, H * Ch], column c weighted by head c // Ch's weights in both hops -- every head in the same two launches
    (hg_table_gather_heads_f32 / hg_table_gather_t_heads_f32), and weight_grad=True gives dw [.., H] from one launch of
    hg_table_dot_heads_f32.  Head h's columns of Y and dX are, bit for bit, the same columns of the call at the full width
    with weight[..., h]; dw[..., h] is the single-head call's on head h's columns.  It needs F % H == 0 and both reductions
    'sum' (ValueError) and float32 rows (bfloat16 raises TypeError whatever the option).  Any other weight is the call above.
    Refusals, in this order and before a device is touched: TypeError for an idx (ptr_v, pos_v) that is not int32 and for
    an X (bfloat16 under the option apart), weight, degE or degV that is not float32; ValueError for the shapes and k;
    RuntimeError for a weight, degE or degV that requires a gradient, and for CPU tensors."""
    if first != "sum" or second != "sum":
        return _knn_aggr_reduced(idx, X, weight, degE, degV, transpose, first, second)
    H = _weight_heads(idx, weight)
    several = H > 1
    bf16 = not several and _rows_bf16(X, options)
    _table_shape(idx)
    if several:
        _check_dtype(X, "X", torch.float32, " (knn_aggr with heads has no bfloat16, float16 or float64 form)")
    elif not bf16:
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
    if X.shape[1] % H:
        raise ValueError("X has F = %d columns, no multiple of heads = %d (weight is %s)" % (X.shape[1], H, tuple(weight.shape)))
    if H == 1 and weight is not None and tuple(weight.shape) not in ((rows * k,), (rows, k)):
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
    _check_feat(X, "X", device=idx.device, bf16_ok=bf16)
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
    return _KnnAggr.apply(X, w, idx, ptr_v, pos_v, degE, degV, H)


def _attention_entry(name):
    """An hg_table_attention_* entry of the library; a build without it is an error, never another path."""
    L = _lib.lib()
    if not hasattr(L, name):
        raise RuntimeError("this build of libhgaggr has no %s (fused attention aggregation over a neighbour table)" % name)
    return getattr(L, name)


def table_attention_stats(idx, n, group, node_score=None, edge_score=None, slope=0.2, ptr_v=None, pos_v=None, heads=1):
    """(seg_max, seg_inv) of hg_table_attention_stats_heads_f32, both [segments, heads] -- segments = rows for 'hyperedge', n for
    'vertex': table_softmax's maximum and reciprocal sum per segment and head, bit for bit.  No checks, no gradient."""
    rows, k = idx.shape
    nseg = rows if group == "hyperedge" else n
    seg_max = torch.empty((nseg, heads), dtype=torch.float32, device=idx.device)
    seg_inv = torch.empty_like(seg_max)
    with torch.cuda.device(idx.device):
        _lib.check(_attention_entry("hg_table_attention_stats_heads_f32")(
            _ptr(idx), rows, k, n, heads, _GROUPS[group], _ptr(node_score), _ptr(edge_score), slope, _ptr(ptr_v), _ptr(pos_v),
            _ptr(seg_max), _ptr(seg_inv), _stream_handle(idx.device)))
    return seg_max, seg_inv


def table_attention_gather(idx, ptr_v, pos_v, n, src, group, node_score, edge_score, slope, seg_max, seg_inv, src_scale=None,
                           dst_scale=None, heads=1, transposed=False):
    """One hop of the fused attention aggregation: table_gather (transposed=False: src [n, F] -> [rows, F]) or table_gather_t
    (src [rows, F] -> [n, F]) with w = table_softmax's alpha, formed inside hg_table_attention_gather(_t)_heads_f32 from the
    scores and table_attention_stats' pair.  No checks, no gradient."""
    rows, k = idx.shape
    F = src.shape[1]
    dst = torch.empty((n if transposed else rows, F), dtype=torch.float32, device=idx.device)
    tail = (rows, k, n, F, heads, _GROUPS[group], _ptr(src), _ptr(node_score), _ptr(edge_score), slope, _ptr(seg_max),
            _ptr(seg_inv), _ptr(src_scale), _ptr(dst_scale), _ptr(dst), _stream_handle(idx.device))
    with torch.cuda.device(idx.device):
        if transposed:
            _lib.check(_attention_entry("hg_table_attention_gather_t_heads_f32")(_ptr(ptr_v), _ptr(pos_v), _ptr(idx), *tail))
        else:
            _lib.check(_attention_entry("hg_table_attention_gather_heads_f32")(_ptr(idx), *tail))
    return dst


class _KnnAttentionAggr(torch.autograd.Function):
    """knn_aggr(X, alpha, weight_grad=True) on alpha = knn_softmax(node_score, edge_score) as one node that never holds alpha
    between forward and backward.  Saves X, the scores, the two statistics per segment and head, the scales, the table and its
    transpose.  Where only X wants a gradient the backward is the two fused gathers swapped.  Where a score wants one it forms
    alpha again with the softmax kernel (the bits the gathers used), runs _KnnAggr's dX / dw formulas and _KnnSoftmax's backward
    on the existing kernels, and frees alpha: every gradient has the two-call path's bits."""

    @staticmethod
    def forward(ctx, X, node_score, edge_score, idx, ptr_v, pos_v, degE, degV, group, slope, heads):
        n = X.shape[0]
        ctx.group, ctx.slope, ctx.heads = group, slope, heads
        seg_max, seg_inv = table_attention_stats(idx, n, group, node_score, edge_score, slope, ptr_v, pos_v, heads)
        call = (group, node_score, edge_score, slope, seg_max, seg_inv)
        Xe = table_attention_gather(idx, ptr_v, pos_v, n, X, *call, None, degE, heads)
        Y = table_attention_gather(idx, ptr_v, pos_v, n, Xe, *call, None, degV, heads, transposed=True)
        need_score = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        ctx.save_for_backward(X if need_score else None, node_score, edge_score, seg_max, seg_inv, idx, ptr_v, pos_v, degE, degV)
        return Y

    @staticmethod
    def backward(ctx, dY):
        X, node_score, edge_score, seg_max, seg_inv, idx, ptr_v, pos_v, degE, degV = ctx.saved_tensors
        dY = dY.contiguous()
        n, k, H, group = dY.shape[0], idx.shape[1], ctx.heads, ctx.group
        need_x, need_node, need_edge = ctx.needs_input_grad[:3]
        tail = (None,) * 8
        if not (need_node or need_edge):  # dX alone: the adjoint is the fused pair itself, swapped
            call = (group, node_score, edge_score, ctx.slope, seg_max, seg_inv)
            G = table_attention_gather(idx, ptr_v, pos_v, n, dY, *call, degV, degE, H)
            return (table_attention_gather(idx, ptr_v, pos_v, n, G, *call, None, None, H, transposed=True), None, None, *tail)
        alpha = table_softmax(idx, n, group, node_score, edge_score, None, ctx.slope, ptr_v, pos_v, H)
        G = table_gather(idx, dY, alpha, degV, degE, heads=H)
        Xe = table_gather(idx, X, alpha, None, degE, heads=H)
        dalpha = table_dot(idx, dY, Xe, degV, X, G, heads=H).view(alpha.shape)
        del Xe  # before dX is allocated: one [rows, F] array fewer at the backward's peak
        dX = table_gather_t(ptr_v, pos_v, k, G, alpha, heads=H) if need_x else None
        del G
        hyperedge = group == "hyperedge"
        need_own, need_other = (need_edge, need_node) if hyperedge else (need_node, need_edge)
        ds, d_own = table_softmax_bwd(idx, n, group, alpha, dalpha, node_score, edge_score, None, ctx.slope, ptr_v, pos_v,
                                      want_group=need_own, heads=H)
        del alpha, dalpha
        d_other = table_sum(idx, n, "vertex" if hyperedge else "hyperedge", ds, ptr_v, pos_v, H) if need_other else None
        d_edge, d_node = (d_own, d_other) if hyperedge else (d_other, d_own)
        return (dX, d_node, d_edge, *tail)


def knn_attention_aggr(idx, X, node_score=None, edge_score=None, group="hyperedge", negative_slope=0.2, degE=None, degV=None,
                       transpose=None, heads=1):
    """Hypergraph attention's aggregation over a neighbour table in one call: what
        knn_aggr(idx, X, knn_softmax(idx, node_score, edge_score, group, negative_slope, heads=heads), degE, degV,
                 weight_grad=True)
    returns, bit for bit, with no [rows, k, heads] array formed in the forward and none saved for the backward.  Forward: one
    launch of hg_table_attention_stats_heads_f32 -- the softmax's maximum and reciprocal sum per segment and head, two
    [rows, heads] or [n, heads] arrays -- and the two fused gathers hg_table_attention_gather_heads_f32 /
    hg_table_attention_gather_t_heads_f32, which form every coefficient from the two scores and those two numbers as they
    gather the row (csrc/hg_table_attention.hip: once per wave in LDS where the lanes of a row share a head, else per lane).
    idx [rows, k] int32; X [n, F] float32; node_score [n] / [n, heads], edge_score [rows] / [rows, heads], either may be None,
    not both; degE [rows] or [rows, 1], degV [n] or [n, 1] or None; transpose: ops.knn_transpose(idx, n) to reuse.
    Gradients are exact for X and both scores and have the two-call path's bits.  Where only X wants one, the backward is the
    two fused gathers swapped; where a score wants one, it forms alpha again with the softmax kernel, runs knn_aggr's and
    knn_softmax's backward kernels on it, and frees it before returning.  degE and degV get no gradient, as in knn_aggr.
    Nothing waits and nothing is read back.
    float32 only.  Not covered, use the two calls above: a logit per entry (entry_score is itself a [rows, k, heads] array),
    attention dropout, bfloat16 rows.
    Refusals, in this order and before a device is touched: TypeError for an idx (ptr_v, pos_v) that is not int32 and for an X,
    score, degE or degV that is not float32; ValueError for an unknown group, for heads, for the shapes and k, for F no
    multiple of heads, for no score at all; RuntimeError for a degE or degV that requires a gradient, and for CPU tensors.  A
    build of the library without the entries raises RuntimeError: there is no other path."""
    _table_shape(idx)
    _check_dtype(X, "X", torch.float32, " (knn_attention_aggr has no bfloat16, float16 or float64 form)")
    scores = (("node_score", node_score), ("edge_score", edge_score))
    scales = (("degE", degE), ("degV", degV))
    for name, t in scores + scales:
        if t is not None:
            _check_dtype(t, name, torch.float32)
    _check_transpose_types(transpose)
    if group not in _GROUPS:
        raise ValueError("group must be 'hyperedge' or 'vertex', got %r" % (group,))
    H = _heads_value(heads)
    tail = (H,) if H > 1 else ()
    rows, k = _table_shape_values(idx)
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be [n >= 1, F >= 1], got %s" % (tuple(X.shape),))
    n, F = X.shape
    if F % H:
        raise ValueError("X has F = %d columns, no multiple of heads = %d" % (F, H))
    if node_score is None and edge_score is None:
        raise ValueError("knn_attention_aggr needs at least one of node_score and edge_score")
    for name, t, count in (("node_score", node_score, n), ("edge_score", edge_score, rows)):
        if t is not None and tuple(t.shape) != (count, *tail):
            raise ValueError("%s must be %s, got %s" % (name, list((count, *tail)), tuple(t.shape)))
    for name, t, count in (("degE", degE, rows), ("degV", degV, n)):
        if t is not None and tuple(t.shape) not in ((count,), (count, 1)):
            raise ValueError("%s must be [%d] or [%d, 1], got %s" % (name, count, count, tuple(t.shape)))
    _check_transpose_shapes(transpose, n, rows * k)
    if torch.is_grad_enabled():
        for name, t in scales:
            if t is not None and t.requires_grad:
                raise RuntimeError("%s gets no gradient from knn_attention_aggr: pass %s.detach()" % (name, name))
    _check_table_index(idx, "idx")
    _check_feat(X, "X", device=idx.device)
    for name, t in scores + scales:
        if t is not None:
            _check_feat(t, name, device=idx.device)
    _attention_entry("hg_table_attention_gather_heads_f32")
    if transpose is None:
        transpose = knn_transpose(idx, n)
    ptr_v, pos_v = transpose
    _check_table_index(ptr_v, "ptr_v")
    _check_table_index(pos_v, "pos_v")
    degE, degV = (None if t is None else t.detach() for _, t in scales)
    return _KnnAttentionAggr.apply(X, node_score, edge_score, idx, ptr_v, pos_v, degE, degV, group, float(negative_slope), H)


DOT_ATTENTION_CH_MAX = 256  # include/hg_aggr.h: one lane group holds a head's columns


def _dot_attention_entry(name):
    """An hg_table_dot_attention_* entry of the library; a build without it is an error, never another path."""
    L = _lib.lib()
    if not hasattr(L, name):
        raise RuntimeError("this build of libhgaggr has no %s (dot-product attention over a neighbour table)" % name)
    return getattr(L, name)


def table_dot_attention(idx, n, src, query, scale, slope, dst_scale=None, heads=1, want_alpha=True):
    """(dst [rows, F], alpha [rows, k, heads] or None) of hg_table_dot_attention_f32: logits scale <query[i], src[idx[i, s]]> per
    head, leaky relu, softmax over the table row and the weighted sum of the same rows, one launch.  No checks, no gradient."""
    rows, k = idx.shape
    F = src.shape[1]
    dst = torch.empty((rows, F), dtype=torch.float32, device=idx.device)
    alpha = torch.empty((rows, k, heads), dtype=torch.float32, device=idx.device) if want_alpha else None
    with torch.cuda.device(idx.device):
        _lib.check(_dot_attention_entry("hg_table_dot_attention_f32")(
            _ptr(idx), rows, k, n, F, heads, _ptr(query), _ptr(src), scale, slope, _ptr(dst_scale), _ptr(dst), _ptr(alpha),
            _stream_handle(idx.device)))
    return dst, alpha


def table_dot_attention_bwd(idx, n, src, query, scale, slope, alpha, ddst, dalpha_ext=None, dst_scale=None, heads=1):
    """(dquery [rows, F], ds [rows, k, heads]) of hg_table_dot_attention_bwd_f32 for the forward's alpha, the gradient ddst of
    its dst and the gradient dalpha_ext that reaches alpha from elsewhere (None: none).  No checks, no gradient."""
    rows, k = idx.shape
    F = src.shape[1]
    dquery = torch.empty((rows, F), dtype=torch.float32, device=idx.device)
    ds = torch.empty((rows, k, heads), dtype=torch.float32, device=idx.device)
    with torch.cuda.device(idx.device):
        _lib.check(_dot_attention_entry("hg_table_dot_attention_bwd_f32")(
            _ptr(idx), rows, k, n, F, heads, _ptr(query), _ptr(src), scale, slope, _ptr(dst_scale), _ptr(alpha), _ptr(ddst),
            _ptr(dalpha_ext), _ptr(dquery), _ptr(ds), _stream_handle(idx.device)))
    return dquery, ds


def table_dot_attention_gather_t(ptr_v, pos_v, k, src, w, src_scale=None, dst_scale=None, heads=1, src2=None, w2=None):
    """dst [n, F] of hg_table_dot_attention_gather_t_f32: dst[v, head h] = dst_scale[v] sum_q ((src[i] src_scale[i]) w[p, h] +
    src2[i] w2[p, h]), p = pos_v[q], i = p // k, one lane group per (vertex, head) summing in ascending q whatever the row's
    length -- so a head's bits do not depend on F or heads.  src, src2 [rows, F]; w, w2 [rows * k, heads].  No checks, no gradient."""
    rows, F = src.shape
    n = ptr_v.shape[0] - 1
    dst = torch.empty((n, F), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(_dot_attention_entry("hg_table_dot_attention_gather_t_f32")(
            _ptr(ptr_v), _ptr(pos_v), rows, k, n, F, heads, _ptr(src), _ptr(w), _ptr(src_scale), _ptr(src2), _ptr(w2),
            _ptr(dst_scale), _ptr(dst), _stream_handle(src.device)))
    return dst


class _KnnDotAttentionAggr(torch.autograd.Function):
    """Y = degV . H_alpha (degE . (H_alpha^T X)) with alpha the row softmax of scale <query[i], X[j]> per head.  Forward: the
    fused kernel (E and alpha in one launch) and hop 1 per (vertex, head), hg_table_dot_attention_gather_t_f32.  Backward: dE
    and hop 1's dalpha from the existing gather and dot, the fused backward kernel (dquery and ds), and dX = the value path +
    the key path, one launch of the hop-1 kernel with two sources.  Saves X, query, the table, its transpose, the scales, alpha [rows, k, H] and E [rows, F] -- nothing of
    rows * k * F elements."""

    @staticmethod
    def forward(ctx, X, query, idx, ptr_v, pos_v, degE, degV, scale, slope, heads):
        ctx.scale, ctx.slope, ctx.heads = scale, slope, heads
        E, alpha = table_dot_attention(idx, X.shape[0], X, query, scale, slope, degE, heads)
        Y = table_dot_attention_gather_t(ptr_v, pos_v, idx.shape[1], E, alpha, None, degV, heads)
        ctx.save_for_backward(X, query, idx, ptr_v, pos_v, degE, degV, alpha, E)
        ctx.mark_non_differentiable(alpha)
        return Y, alpha

    @staticmethod
    def backward(ctx, dY, _):
        X, query, idx, ptr_v, pos_v, degE, degV, alpha, E = ctx.saved_tensors
        dY = dY.contiguous()
        k, H = idx.shape[1], ctx.heads
        need_x, need_q = ctx.needs_input_grad[:2]
        dE = table_gather(idx, dY, alpha, degV, None, heads=H)
        dalpha_ext = table_dot(idx, dY, E, degV, heads=H)
        dquery, ds = table_dot_attention_bwd(idx, X.shape[0], X, query, ctx.scale, ctx.slope, alpha, dE, dalpha_ext, degE, H)
        dX = None
        if need_x:
            dX = table_dot_attention_gather_t(ptr_v, pos_v, k, dE, alpha, degE, None, H, query, ds)
        return (dX, dquery if need_q else None, *(None,) * 8)


def knn_dot_attention_aggr(idx, X, query, negative_slope=1.0, scale=None, degE=None, degV=None, transpose=None, heads=1,
                           return_alpha=False):
    """Dot-product attention's aggregation over a neighbour table, hyperedge group: with j = idx[i, s], Ch = F / heads,
        t[i, s, h] = scale <query[i, head h], X[j, head h]>,   a = t if t > 0 else negative_slope t,
        alpha[i, :, h] = softmax of a over row i's candidates (0 <= j < n; no candidate: +0.0),
        E[i, head h] = degE[i] sum_s alpha[i, s, h] X[j, head h],   Y[v, head h] = degV[v] sum_{p: idx[p] = v} alpha[p, h] E[p // k, head h]
    -- HypergraphAttnConv(score='dot', group='hyperedge')'s formula on the table, query the hyperedges' keys.  idx [rows, k]
    int32; X [n, F] and query [rows, F] float32; scale: a number (default Ch ** -0.5); negative_slope = 1.0 is the plain softmax
    of the logits; degE [rows] or [rows, 1], degV [n] or [n, 1] or None; transpose: ops.knn_transpose(idx, n) to reuse.  Returns
    Y [n, F], and with return_alpha=True (Y, alpha) with alpha [rows, k] or [rows, k, heads], detached.
    Forward: one launch of hg_table_dot_attention_f32 (csrc/hg_table_dot_attention.hip) -- a lane group per (row, head) forms
    the logits, an online softmax and the weighted sum in one walk over the row, every member row of X loaded once -- and hop 1,
    hg_table_dot_attention_gather_t_f32: a lane group per (vertex, head), ascending whatever the row's length, so head h of Y
    (and of alpha) is the single-head call on head h's columns, bit for bit.  Gradients are exact for X (through both hops and
    through the logits) and query: the existing gather and dot give hop 1's share, hg_table_dot_attention_bwd_f32 dquery and the
    logits' gradient, one two-source launch of the hop-1 kernel dX.  Saved for the backward: alpha and E, nothing of rows * k * F elements.  degE and degV get no
    gradient.  Deterministic: every sum's order is include/hg_aggr.h's, two calls give the same bits.  Nothing waits, nothing is
    read back, nothing is allocated outside torch.
    Hub-heavy tables: hop 1 and the dX launch give a vertex to one lane group, which walks the vertex's entries serially (that is
    what makes a head's bits independent of F and heads).  A vertex named by hundreds of rows is the launch's tail -- measured at
    k = 10, in-degrees of 184-305 make the call 1.1-1.4x slower than the composed path at N = 50000 -- and a table with in-degrees
    in the thousands was not measured: ops.knn_softmax(entry_score=) and ops.knn_aggr spread such a row over a workgroup (profiles/r29_table_dot_attention.md).
    X, query and the gradient of Y must share their 16-byte alignment for the forward and backward to pick the same lane width c
    (torch's allocations do).
    Only the hyperedge group exists (the vertex group has no row-local softmax: compose ops.knn_softmax(entry_score=) and
    ops.knn_aggr).  float32 only, no dropout; Ch <= 256.
    Refusals, in this order and before a device is touched: TypeError for an idx (ptr_v, pos_v) that is not int32, for an X,
    query, degE or degV that is not float32 and for a scale that is neither a number nor a tensor; ValueError for heads, for the
    shapes and k, for F no multiple of heads, for Ch > 256, for a query that is not [rows, F]; RuntimeError for a scale, degE or
    degV that requires a gradient, and for CPU tensors.  A build of the library without the entries raises RuntimeError."""
    _table_shape(idx)
    _check_dtype(X, "X", torch.float32, " (knn_dot_attention_aggr has no bfloat16, float16 or float64 form)")
    _check_dtype(query, "query", torch.float32)
    scales = (("degE", degE), ("degV", degV))
    for name, t in scales:
        if t is not None:
            _check_dtype(t, name, torch.float32)
    if scale is not None and not isinstance(scale, torch.Tensor) and (isinstance(scale, bool) or not isinstance(scale, numbers.Real)):
        raise TypeError("scale must be None or a number, got %s" % (type(scale),))
    _check_transpose_types(transpose)
    H = _heads_value(heads)
    rows, k = _table_shape_values(idx)
    if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be [n >= 1, F >= 1], got %s" % (tuple(X.shape),))
    n, F = X.shape
    if F % H:
        raise ValueError("X has F = %d columns, no multiple of heads = %d" % (F, H))
    if F // H > DOT_ATTENTION_CH_MAX:
        raise ValueError("F / heads = %d columns a head, above %d (hg_table_dot_attention_f32 holds a head in one lane group)"
                         % (F // H, DOT_ATTENTION_CH_MAX))
    if tuple(query.shape) != (rows, F):
        raise ValueError("query must be [rows, F] = [%d, %d], got %s" % (rows, F, tuple(query.shape)))
    for name, t, count in (("degE", degE, rows), ("degV", degV, n)):
        if t is not None and tuple(t.shape) not in ((count,), (count, 1)):
            raise ValueError("%s must be [%d] or [%d, 1], got %s" % (name, count, count, tuple(t.shape)))
    if isinstance(scale, torch.Tensor) and scale.numel() != 1:
        raise ValueError("scale must be one number, got a tensor of %s" % (tuple(scale.shape),))
    _check_transpose_shapes(transpose, n, rows * k)
    if isinstance(scale, torch.Tensor) and (scale.requires_grad or scale.is_cuda):
        raise RuntimeError("scale gets no gradient from knn_dot_attention_aggr and is a host number: pass float(scale)")
    if torch.is_grad_enabled():
        for name, t in scales:
            if t is not None and t.requires_grad:
                raise RuntimeError("%s gets no gradient from knn_dot_attention_aggr: pass %s.detach()" % (name, name))
    _check_table_index(idx, "idx")
    _check_feat(X, "X", device=idx.device)
    _check_feat(query, "query", device=idx.device)
    for name, t in scales:
        if t is not None:
            _check_feat(t, name, device=idx.device)
    _dot_attention_entry("hg_table_dot_attention_bwd_f32")
    if transpose is None:
        transpose = knn_transpose(idx, n)
    ptr_v, pos_v = transpose
    _check_table_index(ptr_v, "ptr_v")
    _check_table_index(pos_v, "pos_v")
    degE, degV = (None if t is None else t.detach() for _, t in scales)
    scale = float(F // H) ** -0.5 if scale is None else float(scale)
    Y, alpha = _KnnDotAttentionAggr.apply(X, query, idx, ptr_v, pos_v, degE, degV, scale, float(negative_slope), H)
    if return_alpha:
        return Y, (alpha if H > 1 else alpha.view(rows, k))
    return Y


class KnnHypergraph:
    """The hypergraph "each vertex and its k - 1 nearest neighbours" as a device-only object: what HyperGraph.from_knn builds,
    without the read-back, the host transpose and the plan.  Nothing here reads a tensor back; with segments=None nothing
    waits for the device either (ops.knn waits once for its segment offsets; with set_rows, ops.knn's uniform sets, there
    are no offsets and nothing waits).
      idx [N, k], dist [N, k] (squared), mean [N]: ops.knn(X, k, self_first=True, return_mean=True)
      ptr_v [N + 1], pos_v [N k]: ops.knn_transpose(idx)
      degE [N, 1] = 1 / k and degV [N, 1] = in-degree^-1/2, 1 where no hyperedge names the vertex (HyperGraph's formulas)
      weights(m_prob, X=None): HGNN's exp(-d2 / (m_prob mean)^2) entries [N k].  With X (the rows the table was built
        from, attached to the graph) d2 is ops.knn_dist(idx, X) -- the same bits as `dist`, with a gradient into X; `mean`
        stays detached: its gradient is an N x N sum and HGNN treats avg_dis as a constant of the construction.
      aggregate(Z, probabilistic=False, m_prob=1.0, X=None, first="sum", second="sum"): ops.knn_aggr over the table; X goes
        to weights, and the weights then get their gradient (weight_grad=True); first / second are ops.knn_aggr's reductions
        (no weights with anything but the two sums).  weight=: explicit weights [N k] (or [N, k]) in place of the
        probabilistic ones, passed with weight_grad=True -- attention's alpha; exclusive with probabilistic.  heads=H:
        the weight must be ops.knn_aggr's several-heads weight [N k, H] or [N, k, H] (ValueError otherwise).
      attention(node_score, edge_score, group="hyperedge", negative_slope=0.2, heads=1, dropout=0.0, training=True,
        rng_state=None): ops.knn_softmax over the table with the stored transpose: alpha [N, k], or [N, k, H]; dropout,
        training and rng_state are ops.knn_softmax's (the coefficients after dropout, from the softmax's own launch).
      attention_aggregate(Z, node_score, edge_score, group="hyperedge", negative_slope=0.2, heads=1): ops.knn_attention_aggr
        with the stored table, transpose and degrees -- aggregate(Z, weight=attention(..), heads=heads), bit for bit, with no
        [N, k, heads] array in the forward or kept for the backward.
      dot_attention_aggregate(Z, query, negative_slope=1.0, heads=1): ops.knn_dot_attention_aggr with the stored table,
        transpose and degrees -- dot-product attention of every hyperedge's query row [N, F] to its members' rows of Z.
    form: ops.knn's -- "dot" and "dot_split" give the same idx and dist through a matrix-unit prefilter, and their own mean.  Under "dot" X
    may be bfloat16: the table, dist, mean, transpose and degrees are int32 / float32 as always, and aggregate / weights take
    bfloat16 Z / X where `options` (or the caller's) has Options.incidence_bf16 = 'rows' -- ops.knn_aggr's and ops.knn_dist's
    bfloat16 rows, the weights float32."""

    @classmethod
    def build(cls, X, k, segments=None, form="difference", set_rows=None):
        self = cls.__new__(cls)
        if isinstance(X, torch.Tensor):  # anything else is ops.knn's refusal
            X = X.detach().contiguous()
        self.idx, self.dist, self.mean = knn(X, k, segments=segments, self_first=True, return_mean=True, form=form,
                                            set_rows=set_rows)
        N = self.idx.shape[0]
        self.k, self.num_nodes, self.num_edges, self.nnz = int(k), N, N, N * int(k)
        self.device = self.idx.device
        self.ptr_v, self.pos_v = knn_transpose(self.idx, N)
        self.degE = torch.full((N, 1), 1.0 / int(k), dtype=torch.float32, device=self.device)
        deg = (self.ptr_v[1:] - self.ptr_v[:-1]).to(torch.float32).reshape(N, 1)
        self.degV = torch.where(deg > 0, deg.pow(-0.5), torch.ones_like(deg))
        return self

    def weights(self, m_prob=1.0, X=None, options=None):
        if X is None:
            return knn_incidence_weights(self.dist, self.mean, m_prob)
        dist = knn_dist(self.idx, X, transpose=(self.ptr_v, self.pos_v), options=options)
        return knn_incidence_weights(dist, self.mean, m_prob)

    def aggregate(self, Z, probabilistic=False, m_prob=1.0, X=None, options=None, weight=None, heads=1, first="sum",
                  second="sum"):
        if weight is not None and probabilistic:
            raise ValueError("weight and probabilistic=True exclude each other (both are the table's weights)")
        H = _heads_value(heads)
        if H != _weight_heads(self.idx, weight):
            raise ValueError("heads=%d needs weight [N k, %d] or [N, k, %d], got %s"
                             % (H, H, H, None if weight is None else tuple(weight.shape)))
        if weight is not None:
            return knn_aggr(self.idx, Z, weight, self.degE, self.degV, transpose=(self.ptr_v, self.pos_v), weight_grad=True,
                            options=options, first=first, second=second)
        w = self.weights(m_prob, X, options) if probabilistic else None
        return knn_aggr(self.idx, Z, w, self.degE, self.degV, transpose=(self.ptr_v, self.pos_v), weight_grad=X is not None,
                        options=options, first=first, second=second)

    def attention(self, node_score=None, edge_score=None, group="hyperedge", negative_slope=0.2, heads=1, dropout=0.0,
                  training=True, rng_state=None):
        return knn_softmax(self.idx, node_score, edge_score, group, negative_slope, transpose=(self.ptr_v, self.pos_v),
                           num_nodes=self.num_nodes, heads=heads, dropout=dropout, training=training, rng_state=rng_state)

    def attention_aggregate(self, Z, node_score=None, edge_score=None, group="hyperedge", negative_slope=0.2, heads=1):
        return knn_attention_aggr(self.idx, Z, node_score, edge_score, group, negative_slope, self.degE, self.degV,
                                  transpose=(self.ptr_v, self.pos_v), heads=heads)

    def dot_attention_aggregate(self, Z, query, negative_slope=1.0, heads=1):
        return knn_dot_attention_aggr(self.idx, Z, query, negative_slope, None, self.degE, self.degV,
                                      transpose=(self.ptr_v, self.pos_v), heads=heads)


def table_seq_max():
    """HG_TABLE_SEQ_MAX of the library as built: the longest row one lane group sums in ascending order."""
    return int(_lib.lib().hg_table_seq_max())
