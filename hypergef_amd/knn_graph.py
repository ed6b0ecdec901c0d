"""k-nearest-neighbour hypergraph construction (include/hg_aggr.h, hg_knn_f32): the hyperedges of HGNN's ModelNet40 /
NTU2012 hypergraphs and of DHGNN's layers, "each vertex and its k nearest neighbours in feature space", found on the
device without the N x N distance matrix.

`knn` and `knn_incidence_weights` are exported as `ops.knn` / `ops.knn_incidence_weights`; `incidence_from_knn` is the
host-side layout step of `HyperGraph.from_knn`.
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


def knn(X, k, queries=None, segments=None, self_first=None, return_mean=False, cand_slices=0):
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

    Not differentiable: raises if X (or queries) requires a gradient while grad mode is on; call it under
    torch.no_grad() or on X.detach().  Refusals, in this order and before a device is touched: TypeError for anything
    but float32; ValueError for k outside 1 .. min(64, n), for segments or self_first together with queries, for a segment
    shorter than k; RuntimeError for CPU tensors."""
    for name, t in (("X", X), ("queries", queries)):
        if t is None and name == "queries":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError("%s must be a float32 tensor (knn has no bfloat16 / float16 / float64 form), got %s"
                            % (name, getattr(t, "dtype", type(t))))
    if X.dim() != 2 or X.shape[1] < 1:
        raise ValueError("X must be [n, F] with F >= 1, got %s" % (tuple(X.shape),))
    n, F = X.shape
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
    seg = None if segments is None else _segment_offsets(segments, n, k)
    if not isinstance(cand_slices, numbers.Integral) or isinstance(cand_slices, bool) or not 0 <= cand_slices <= SLICES_MAX:
        raise ValueError("cand_slices must be 0 (auto) or 1 .. %d, got %r" % (SLICES_MAX, cand_slices))
    if torch.is_grad_enabled() and (X.requires_grad or (queries is not None and queries.requires_grad)):
        raise RuntimeError("knn is not differentiable: call it under torch.no_grad() or on X.detach()")
    _check_feat(X, "X")
    if queries is not None:
        _check_feat(queries, "queries", device=X.device)
    if self_first is None:
        self_first = queries is None
    Q = X if queries is None else queries
    nq, k, cand_slices = Q.shape[0], int(k), int(cand_slices)
    dev = X.device
    L = _lib.lib()
    idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
    dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
    mean = torch.empty(nq, dtype=torch.float32, device=dev) if return_mean else None
    ws_bytes = L.hg_knn_workspace_bytes(nq, n, F, k, cand_slices)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    seg_ptr = None if seg is None else seg.ctypes.data_as(ctypes.c_void_p)
    with torch.cuda.device(dev):
        _lib.check(L.hg_knn_f32(_ptr(Q), nq, _ptr(X), n, F, k, seg_ptr, 0 if seg is None else seg.shape[0] - 1,
                                1 if self_first else 0, cand_slices, _ptr(idx), _ptr(dist), _ptr(mean), _ptr(ws), ws_bytes,
                                _stream_handle(dev)))
    return (idx, dist, mean) if return_mean else (idx, dist)


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
