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


# ---- the difference form's split of the candidates and its merge (csrc/hg_knn.hip), as a host model -------------------------
# The tile sizes of csrc/hg_knn.h, mirrored; tests/test_table_buffers_host.py holds them against the header's text.
KNN_TQ, KNN_TC, KNN_MAX_K, KNN_MAX_SLICES = 64, 256, 64, 32
DOT_TQ, DOT_TC, DOT_NORM_ROWS = 128, 128, 64
INT_MAX = 2 ** 31 - 1


def auto_slices(nq, n):
    """cand_slices = 0 of the difference form: 2 where few query tiles face at least two candidate tiles, else 1."""
    return 2 if -(-nq // KNN_TQ) <= 128 and -(-n // KNN_TC) >= 2 else 1


def workspace_bytes(nq, n, k, slices):
    """hg_knn_workspace_bytes for `slices` slices: the segment copy (present whenever nq == n), then the lists and the partial
    means of the slices 1 .. slices - 1 -- a slice that owns no candidate tile is counted like any other."""
    seg = ((n + 1) * 4 + 255) // 256 * 256 if nq == n else 0
    extra = max(slices - 1, 0)
    return seg + extra * nq * k * 8 + extra * nq * 4


def slice_ranges(nq, n, slices, segments=None):
    """(a, b), int64 [nq, slices]: row i's candidates in slice s are the rows a[i, s] .. b[i, s] - 1, read from knn_kernel.
    A workgroup owns KNN_TQ query rows; its candidates are the one range from the first row's segment start to the last
    row's segment end, cut into tiles of KNN_TC rows from that start; slice s takes the tiles [tiles s / slices,
    tiles (s + 1) / slices) and a row keeps what of them lies in its own segment."""
    lo, hi = candidate_ranges(n, nq, segments)
    a = np.zeros((nq, slices), np.int64)
    b = np.zeros((nq, slices), np.int64)
    for q0 in range(0, nq, KNN_TQ):
        q1 = min(q0 + KNN_TQ, nq)
        c_lo, c_hi = int(lo[q0]), int(hi[q1 - 1])
        tiles = -(-(c_hi - c_lo) // KNN_TC)
        for s in range(slices):
            s_lo = c_lo + (tiles * s // slices) * KNN_TC
            s_hi = c_lo + (tiles * (s + 1) // slices) * KNN_TC
            a[q0:q1, s] = np.maximum(lo[q0:q1], s_lo)
            b[q0:q1, s] = np.maximum(a[q0:q1, s], np.minimum(hi[q0:q1], s_hi))
    return a, b


def slice_lists(D, k, a, b, self_first):
    """The slices' lists as knn_kernel leaves them for the merge: (ld float32 [nq, slices, k], lj int32 [nq, slices, k],
    used bool [nq, slices, k]).  A list holds the k smallest of its candidates under (key, j), key = d2 or -1 for the row
    itself under self_first; a slot past the slice's candidates is unused and holds the sentinel (+inf, INT_MAX)."""
    nq, slices = a.shape
    ld = np.full((nq, slices, k), np.inf, np.float32)
    lj = np.full((nq, slices, k), INT_MAX, np.int32)
    used = np.zeros((nq, slices, k), bool)
    for i in range(nq):
        for s in range(slices):
            if b[i, s] <= a[i, s]:
                continue
            j = np.arange(a[i, s], b[i, s])
            key = np.asarray(D[i, a[i, s]:b[i, s]], np.float64).copy()
            if self_first and a[i, s] <= i < b[i, s]:
                key[i - a[i, s]] = -1.0
            order = np.lexsort((j, key))[:k]
            m = order.shape[0]
            ld[i, s, :m], lj[i, s, :m], used[i, s, :m] = key[order], j[order], True
    return ld, lj, used


def poison_unused(ld, lj, used, word):
    """The lists with every unused slot holding the 32-bit `word` in both arrays: what the merge would read if the sentinel
    writes were missing and the workspace (slice 0: idx / dist themselves) still held that word."""
    pd = np.where(used, ld, np.array([word], np.uint32).view(np.float32)[0]).astype(np.float32)
    pj = np.where(used, lj, np.array([word], np.uint32).view(np.int32)[0]).astype(np.int32)
    return pd, pj


def _key_less(ad, aj, bd, bj):
    return (ad < bd) | ((ad == bd) & (aj < bj))


def merge_ranks(ld, lj):
    """knn_merge_kernel's rank of every entry of one row's lists (ld, lj [slices, k]), int64 [slices k]: the entry's place in
    its own list plus, per other list, where the kernel's binary search ends -- entries [0, lo) are before this one, with
    equal keys going to the earlier slice.  The search is the kernel's, step for step, so a list that is not sorted (a
    poisoned one) is searched the way the kernel would search it."""
    S, k = ld.shape
    L = S * k
    d, j = ld.reshape(-1)[:, None], lj.reshape(-1)[:, None]
    s_of = np.repeat(np.arange(S), k)
    o = np.arange(S)[None, :]
    earlier = o < s_of[:, None]
    lo = np.zeros((L, S), np.int64)
    hi = np.full((L, S), k, np.int64)
    active = lo < hi
    while active.any():
        m = (lo + hi) >> 1
        mm = np.minimum(m, k - 1)
        od, oj = ld[o, mm], lj[o, mm]
        before = np.where(earlier, ~_key_less(d, j, od, oj), _key_less(od, oj, d, j))
        lo = np.where(active & before, m + 1, lo)
        hi = np.where(active & ~before, m, hi)
        active = lo < hi
    lo[np.arange(L), s_of] = 0  # its own list: the place it has there
    return np.tile(np.arange(k), S) + lo.sum(1)


def merge(ld, lj, rows=None):
    """The model of knn_merge_kernel: (idx int32 [rows, k], dist float32 [rows, k]).  idx / dist hold slice 0's list when the
    merge starts; every entry of rank below k goes to its rank with a key below 0 (the row itself) written as 0."""
    nq, S, k = ld.shape
    rows = np.arange(nq) if rows is None else np.asarray(rows)
    out_i = lj[rows, 0, :].copy()
    out_d = ld[rows, 0, :].copy()
    for r, i in enumerate(rows):
        rank = merge_ranks(ld[i], lj[i])
        d, j = ld[i].reshape(-1), lj[i].reshape(-1)
        w = rank < k
        out_i[r, rank[w]] = j[w]
        out_d[r, rank[w]] = np.where(d[w] < 0, np.float32(0), d[w])
    return out_i, out_d
