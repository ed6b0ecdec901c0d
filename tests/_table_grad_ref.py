"""numpy models of the operators that train through a neighbour table's weights (include/hg_aggr.h, hg_table_dist_f32,
hg_table_gather_diff_f32 / hg_table_gather_t_diff_f32, hg_table_dot_f32): test infrastructure, numpy only.

float32 models in the header's order, bit for bit: dist (the fma chain, emulated exactly), gather_diff / gather_t_diff
(tests/_table_ref.py's gather / gather_t_ordered with the difference term in place of the plain one) and table_dot (the DOT
ORDER paragraph: lanes, chains, butterfly).  float64 references: dist64, dist_grad64 (dQ, dX of a given dDist) and dw64 (the
gradient of ops.knn_aggr's weights)."""
import numpy as np

import _table_ref as tr

U32 = 2.0 ** -24  # the unit roundoff of float32


def fma32(a, b, c):
    """fma(a, b, c) of float32 arrays, correctly rounded.  a * b is exact in float64 (48 bits); the float64 sum s = p + c and
    its exact error e (TwoSum) give the exact value s + e, and rounding s to float32 is rounding s + e unless s stands exactly
    half way between two float32 numbers while e != 0 -- then e's sign decides."""
    a, b, c = (np.asarray(t, np.float32).astype(np.float64) for t in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    f = s.astype(np.float32)
    f64 = f.astype(np.float64)
    other = np.nextafter(f, np.where(s > f64, np.inf, -np.inf).astype(np.float32))
    tie = (e != 0) & (f64 != s) & ((f64 + other.astype(np.float64)) / 2 == s)
    return np.where(tie, np.where(e > 0, np.maximum(f, other), np.minimum(f, other)), f).astype(np.float32)


def dist(idx, X, Q=None):
    """dist[i, s] = sum_c (Q[i, c] - X[idx[i, s], c])^2 as hg_knn_f32 forms it: c ascending, the difference rounded, one fma
    into one accumulator from +0.0.  An entry outside 0 .. n - 1 is +0.0."""
    idx = np.asarray(idx)
    X = np.asarray(X, np.float32)
    Q = X if Q is None else np.asarray(Q, np.float32)
    rows, k = idx.shape
    n, F = X.shape
    valid = (idx >= 0) & (idx < n)
    j = np.where(valid, idx, 0)
    acc = np.zeros((rows, k), np.float32)
    for c in range(F):
        d = (Q[:, c][:, None] - X[j, c]).astype(np.float32)
        acc = fma32(d, d, acc)
    return np.where(valid, acc, np.float32(0)).astype(np.float32)


def _with_diff_term(ctr, row_of, fn, *args, **kw):
    """fn (one of _table_ref's gathers) with term(p, j) = ((ctr[row_of(p)] - src[j]) * src_scale[j]) * w[p], every step rounded."""
    ctr = np.asarray(ctr, np.float32)

    def term(src, j, p, w, src_scale):
        t = (ctr[row_of(p)] - src[j].astype(np.float32)).astype(np.float32)
        if src_scale is not None:
            t = (t * np.float32(src_scale[j])).astype(np.float32)
        if w is not None:
            t = (t * np.float32(w[p])).astype(np.float32)
        return t

    plain = tr._term
    tr._term = term
    try:
        return fn(*args, **kw)
    finally:
        tr._term = plain


def gather_diff(idx, ctr, src, w=None, src_scale=None, dst_scale=None):
    """dst[i] = dst_scale[i] * sum_s term(i k + s, idx[i, s]) with the centre ctr[i]: float32, ascending s."""
    k = np.asarray(idx).shape[1]
    return _with_diff_term(ctr, lambda p: p // k, tr.gather, idx, np.asarray(src, np.float32), w, src_scale, dst_scale)


def gather_t_diff(idx, ptr_v, pos_v, ctr, src, w=None, src_scale=None, dst_scale=None, aligned16=True, seq_max=128):
    """dst[v] = dst_scale[v] * sum_q term(pos_v[q], pos_v[q] // k) with the centre ctr[v], in the header's ORDER: rows up to
    seq_max ascending, longer ones in the pieces and the tree.  idx gives the vertex a position belongs to."""
    flat = np.asarray(idx).reshape(-1)
    k = np.asarray(idx).shape[1]
    return _with_diff_term(ctr, lambda p: int(flat[p]), tr.gather_t_ordered, ptr_v, pos_v, k, np.asarray(src, np.float32), w,
                           src_scale, dst_scale, aligned16=aligned16, seq_max=seq_max)


def dot_shape(F, aligned16=True):
    """(c, L) of the DOT ORDER paragraph: c columns a lane, L = the power of two at or above min(ceil(F / c), 64) lanes."""
    c = 4 if F % 4 == 0 and aligned16 else 1
    L = 1
    while L < min(-(-F // c), 64):
        L *= 2
    return c, L


def table_dot(idx, A, B, a_scale=None, C=None, D=None, aligned16=True):
    """out[p] = a_scale[j] <A[j], B[i]> + <C[j], D[i]> in float32 in the header's DOT ORDER, [rows * k]."""
    idx = np.asarray(idx)
    rows, k = idx.shape
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    n, F = A.shape
    c, L = dot_shape(F, aligned16)
    flat = idx.reshape(-1)
    valid = (flat >= 0) & (flat < n)
    j = np.where(valid, flat, 0)
    i = np.arange(rows * k) // k
    t = np.zeros((rows * k, L), np.float32)
    for lane in range(L):
        cols = [m + lane * c + u for m in range(0, F, L * c) for u in range(c) if m + lane * c + u < F]
        s1 = np.zeros(rows * k, np.float32)
        s2 = np.zeros(rows * k, np.float32)
        for x in cols:
            s1 = fma32(A[j, x], B[i, x], s1)
            if C is not None:
                s2 = fma32(np.asarray(C, np.float32)[j, x], np.asarray(D, np.float32)[i, x], s2)
        if a_scale is not None:
            s1 = (np.asarray(a_scale, np.float32).reshape(-1)[j] * s1).astype(np.float32)
        t[:, lane] = (s1 + s2).astype(np.float32) if C is not None else s1
    o = L // 2
    lanes = np.arange(L)
    while o >= 1:
        t = (t + t[:, lanes ^ o]).astype(np.float32)
        o //= 2
    return np.where(valid, t[:, 0], np.float32(0)).astype(np.float32)


# ---- float64 ------------------------------------------------------------------------------------------------------------

def dist64(idx, X, Q=None):
    idx = np.asarray(idx)
    X = np.asarray(X, np.float64)
    Q = X if Q is None else np.asarray(Q, np.float64)
    valid = (idx >= 0) & (idx < X.shape[0])
    d = Q[:, None, :] - X[np.where(valid, idx, 0)]
    return np.where(valid, (d * d).sum(-1), 0.0)


def dist_grad64(idx, dDist, X, Q=None):
    """(dQ [rows, F], dX [n, F]) of sum(dDist * dist64) in float64; with Q None the one gradient of X is their sum."""
    idx = np.asarray(idx)
    X = np.asarray(X, np.float64)
    Qr = X if Q is None else np.asarray(Q, np.float64)
    rows, k = idx.shape
    dQ, dX = np.zeros_like(Qr), np.zeros_like(X)
    g = 2.0 * np.asarray(dDist, np.float64).reshape(rows, k)
    for i in range(rows):
        for s in range(k):
            j = int(idx[i, s])
            if 0 <= j < X.shape[0]:
                diff = Qr[i] - X[j]
                dQ[i] += g[i, s] * diff
                dX[j] -= g[i, s] * diff
    return dQ, dX


def table_dot64(idx, A, B, a_scale=None, C=None, D=None):
    """(out, mass) in float64: mass[p] = |a_scale[j]| sum_c |A B| + sum_c |C D|, what the dot-product bound multiplies."""
    idx = np.asarray(idx)
    rows, k = idx.shape
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    flat = idx.reshape(-1)
    valid = (flat >= 0) & (flat < A.shape[0])
    j = np.where(valid, flat, 0)
    i = np.arange(rows * k) // k
    sc = np.ones(A.shape[0]) if a_scale is None else np.asarray(a_scale, np.float64).reshape(-1)
    out = sc[j] * (A[j] * B[i]).sum(1)
    mass = np.abs(sc[j]) * np.abs(A[j] * B[i]).sum(1)
    if C is not None:
        C, D = np.asarray(C, np.float64), np.asarray(D, np.float64)
        out = out + (C[j] * D[i]).sum(1)
        mass = mass + np.abs(C[j] * D[i]).sum(1)
    return np.where(valid, out, 0.0), np.where(valid, mass, 0.0)


def dot_bound(F, mass):
    """(F + 4) 2^-23 mass: the standard bound of a float32 dot product of F terms with four more rounded steps."""
    return (F + 4) * 2.0 ** -23 * mass


def dw64(idx, X, dY, w, degE=None, degV=None):
    """The gradient of sum(dY * aggr(idx, X, w, degE, degV)) in w, float64 [rows * k], from the dense operator: with
    Ht = H_w^T [rows, n], Y = degV . Ht^T (degE . (Ht X)), so dHt = degE . ((Ht X)(degV . dY)^T + (Ht (degV . dY)) X^T)."""
    idx = np.asarray(idx)
    rows, k = idx.shape
    n = X.shape[0]
    Ht = tr._dense64(idx, n, w)
    X, dYs = np.asarray(X, np.float64), tr._col64(degV, n) * np.asarray(dY, np.float64)
    dHt = tr._col64(degE, rows) * ((Ht @ X) @ dYs.T + (Ht @ dYs) @ X.T)
    flat = idx.reshape(-1)
    valid = (flat >= 0) & (flat < n)
    return np.where(valid, dHt[np.arange(rows * k) // k, np.where(valid, flat, 0)], 0.0)
