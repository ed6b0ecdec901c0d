"""numpy references for the neighbour-table operators (include/hg_aggr.h, hg_table_*): test infrastructure, numpy only.

transpose: the stable argsort of the valid positions by vertex.  gather / gather_t: float32 loops in the contract's order
for rows one lane group sums (every row of gather; rows of gather_t up to HG_TABLE_SEQ_MAX entries).  aggr / aggr_grad:
the whole operator Y = degV . H_w (degE . (H_w^T X)) and its X-gradient in float64."""
import numpy as np


def transpose(idx, n=None):
    """(ptr_v [n + 1], pos_v [valid entries]) of a table idx [rows, k]: the positions p = i k + s with idx[p] == v, ascending,
    for v = 0 .. n - 1; entries outside 0 .. n - 1 are counted nowhere."""
    idx = np.asarray(idx)
    n = idx.shape[0] if n is None else n
    flat = idx.reshape(-1).astype(np.int64)
    valid = np.flatnonzero((flat >= 0) & (flat < n))
    order = valid[np.argsort(flat[valid], kind="stable")]
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, flat[valid] + 1, 1)
    return np.cumsum(ptr).astype(np.int32), order.astype(np.int32)


def transpose_loops(idx, n=None):
    """The definition written out: for every vertex, every position in ascending order."""
    idx = np.asarray(idx)
    n = idx.shape[0] if n is None else n
    flat = idx.reshape(-1)
    ptr, pos = [0], []
    for v in range(n):
        for p in range(flat.shape[0]):
            if flat[p] == v:
                pos.append(p)
        ptr.append(len(pos))
    return np.asarray(ptr, np.int32), np.asarray(pos, np.int32)


def _term(src, j, p, w, src_scale):
    t = src[j].astype(np.float32)
    if src_scale is not None:
        t = (t * np.float32(src_scale[j])).astype(np.float32)
    if w is not None:
        t = (t * np.float32(w[p])).astype(np.float32)
    return t


def gather(idx, src, w=None, src_scale=None, dst_scale=None):
    """dst[i] = dst_scale[i] * sum_s term(i k + s, idx[i, s]) in float32, ascending s, one rounded add a term."""
    idx = np.asarray(idx)
    rows, k = idx.shape
    n, F = src.shape
    out = np.zeros((rows, F), np.float32)
    for i in range(rows):
        acc = np.zeros(F, np.float32)
        for s in range(k):
            j = int(idx[i, s])
            if 0 <= j < n:
                acc = (acc + _term(src, j, i * k + s, w, src_scale)).astype(np.float32)
        if dst_scale is not None:
            acc = (np.float32(dst_scale[i]) * acc).astype(np.float32)
        out[i] = acc
    return out


def gather_t(ptr_v, pos_v, k, src, w=None, src_scale=None, dst_scale=None):
    """dst[v] = dst_scale[v] * sum_q term(pos_v[q], pos_v[q] // k) in float32, ascending q; an empty row is +0.0."""
    n = len(ptr_v) - 1
    F = src.shape[1]
    out = np.zeros((n, F), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in range(n):
            acc = np.zeros(F, np.float32)
            for q in range(int(ptr_v[v]), int(ptr_v[v + 1])):
                p = int(pos_v[q])
                acc = (acc + _term(src, p // k, p, w, src_scale)).astype(np.float32)
            if dst_scale is not None and ptr_v[v + 1] > ptr_v[v]:
                acc = (np.float32(dst_scale[v]) * acc).astype(np.float32)
            out[v] = acc
    return out


def _dense64(idx, n, w):
    """H_w^T as a dense float64 [rows, n] matrix (duplicates within a row add up)."""
    idx = np.asarray(idx)
    rows, k = idx.shape
    Ht = np.zeros((rows, n), np.float64)
    wf = np.ones(rows * k) if w is None else np.asarray(w, np.float64).reshape(-1)
    for i in range(rows):
        for s in range(k):
            j = int(idx[i, s])
            if 0 <= j < n:
                Ht[i, j] += wf[i * k + s]
    return Ht


def _col64(t, count):
    return np.ones((count, 1)) if t is None else np.asarray(t, np.float64).reshape(count, 1)


def aggr(idx, X, w=None, degE=None, degV=None):
    """Y = degV . H_w (degE . (H_w^T X)) in float64."""
    n = X.shape[0]
    Ht = _dense64(idx, n, w)
    return _col64(degV, n) * (Ht.T @ (_col64(degE, Ht.shape[0]) * (Ht @ X.astype(np.float64))))


def aggr_grad(idx, dY, w=None, degE=None, degV=None):
    """dX of aggr for the output gradient dY, in float64: the operator is symmetric up to where the scales sit."""
    n = dY.shape[0]
    Ht = _dense64(idx, n, w)
    return Ht.T @ (_col64(degE, Ht.shape[0]) * (Ht @ (_col64(degV, n) * dY.astype(np.float64))))
