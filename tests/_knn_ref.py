"""Reference of ops.knn in numpy: CPU, float64, test infrastructure only.

    d2(i, j) = sum_c (Q[i, c] - X[j, c])^2                     (float64, the difference form)
    row i    = its k smallest candidates under the total order (d2, j), by np.lexsort((j, d2)), ascending
self_first ranks candidate j == i before every other one; segments (offsets [B + 1]) restrict row i's candidates to the
rows of its own segment; mean[i] = mean of sqrt(d2(i, j)) over every candidate of row i, itself included.
"""
import numpy as np


def distances(Q, X):
    """d2 as float64 [nq, n], row by row (no [nq, n, F] intermediate)."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    out = np.empty((Q.shape[0], X.shape[0]), np.float64)
    for i in range(Q.shape[0]):
        diff = X - Q[i]
        out[i] = (diff * diff).sum(1)
    return out


def candidate_ranges(n, nq, segments=None):
    """(lo [nq], hi [nq]): row i competes with rows lo[i] .. hi[i] - 1."""
    if segments is None:
        return np.zeros(nq, np.int64), np.full(nq, n, np.int64)
    seg = np.asarray(segments, np.int64)
    assert nq == n and seg[0] == 0 and seg[-1] == n and (np.diff(seg) >= 0).all()
    b = np.searchsorted(seg, np.arange(n), side="right") - 1
    return seg[b], seg[b + 1]


def knn(X, k, queries=None, segments=None, self_first=None, D=None):
    """(idx int32 [nq, k], dist float64 [nq, k], mean float64 [nq]).  D: distances(Q, X) where the caller already holds it."""
    X = np.asarray(X)
    Q = X if queries is None else np.asarray(queries)
    if self_first is None:
        self_first = queries is None
    assert not (self_first and queries is not None)
    nq, n = Q.shape[0], X.shape[0]
    if D is None:
        D = distances(Q, X)
    lo, hi = candidate_ranges(n, nq, segments)
    idx = np.empty((nq, k), np.int32)
    dist = np.empty((nq, k), np.float64)
    mean = np.empty(nq, np.float64)
    for i in range(nq):
        j = np.arange(lo[i], hi[i])
        d2 = D[i, lo[i]:hi[i]]
        assert k <= j.shape[0]
        key = d2.copy()
        if self_first:
            key[i - lo[i]] = -1.0  # before every distance; reported as d2(i, i) = 0
        order = np.lexsort((j, key))[:k]
        idx[i] = j[order]
        dist[i] = d2[order]
        mean[i] = np.sqrt(d2).mean()
    return idx, dist, mean


def knn_loops(X, k, queries=None, segments=None, self_first=None):
    """The definition again as plain loops over (query, candidate, column) with a selection by repeated minimum: what
    `knn` is checked against on a small case."""
    X = np.asarray(X, np.float64)
    Q = X if queries is None else np.asarray(queries, np.float64)
    if self_first is None:
        self_first = queries is None
    nq, n, F = Q.shape[0], X.shape[0], X.shape[1]
    idx, dist, mean = [], [], []
    for i in range(nq):
        lo, hi = 0, n
        if segments is not None:
            for b in range(len(segments) - 1):
                if segments[b] <= i < segments[b + 1]:
                    lo, hi = segments[b], segments[b + 1]
        d2 = {}
        for j in range(lo, hi):
            s = 0.0
            for c in range(F):
                s += (Q[i, c] - X[j, c]) * (Q[i, c] - X[j, c])
            d2[j] = s
        left = dict(d2)
        row_i, row_d = [], []
        if self_first:
            row_i.append(i)
            row_d.append(left.pop(i))
        while len(row_i) < k:
            best = None
            for j in sorted(left):
                if best is None or left[j] < left[best]:  # strict: the smaller index wins a tie
                    best = j
            row_i.append(best)
            row_d.append(left.pop(best))
        idx.append(row_i)
        dist.append(row_d)
        mean.append(sum(v ** 0.5 for v in d2.values()) / len(d2))
    return np.asarray(idx, np.int32), np.asarray(dist, np.float64), np.asarray(mean, np.float64)
