"""ops.knn(form="dot_split") in numpy: CPU, test infrastructure only (include/hg_aggr.h, hg_knn_dot_split_f32).

    split         a float32 array as its two bfloat16 parts (hi, lo), as float32: hi = bf16(x), lo = bf16(x - hi)
    bound_split   E1s [nq] in float32, operation for operation what the kernels compute
    estimates     d~ under one of _knn_bf16_ref's models of the instruction: float32 norms of the unsplit rows, then per
                  16-column group qh.xh, qh.xl, ql.xh into one accumulator, d~ = (n2q + n2x) - 2 s~
    KINDS / rows  the adversarial float32 inputs of the host test and of the device test
"""
import numpy as np

import _knn_bf16_ref as br
import _knn_dot_ref as dr

F32 = np.float32
U = F32(2.0 ** -24)


def split(x, flush=False):
    """flush: a part below 2^-126 in magnitude is read as zero."""
    x = np.ascontiguousarray(x, F32)
    hi = br.to_bf16(x)
    lo = br.to_bf16(x - hi)  # x - hi is exact in float32
    return br._flush(hi, flush).astype(F32), br._flush(lo, flush).astype(F32)


def bound_split(Q, X):
    """E1s = C_s u (n2q + n2max) + (328 G + 1) 2^-126, G = ceil(F / 16), C_s = (775 + F + 104 G)(1 + 1/64) rounded up."""
    F = np.asarray(X).shape[1]
    assert 1 <= F <= dr.F_MAX
    total = (dr.norms(Q) + dr.norms(X).max()).astype(F32)
    G = (F + 15) // 16
    c2 = 775 + F + 104 * G
    C = F32(c2 + (c2 >> 6) + 1) * U
    with np.errstate(over="ignore", invalid="ignore"):
        return (C * total + F32(328 * G + 1) * F32(br.TINY)).astype(F32)


def estimates(Q, X, model, flush=False):
    (qh, ql), (xh, xl) = split(Q, flush), split(X, flush)
    F = X.shape[1]
    G = (F + 15) // 16
    qh, ql, xh, xl = (np.pad(a.astype(np.float64), ((0, 0), (0, 16 * G - F))) for a in (qh, ql, xh, xl))
    acc = np.zeros((Q.shape[0], X.shape[0]), F32)
    step = br.MODELS[model]
    for g in range(G):
        c = slice(16 * g, 16 * g + 16)
        for a, b in ((qh, xh), (qh, xl), (ql, xh)):
            acc = step(acc, a[:, None, c] * b[None, :, c], flush)  # products of bfloat16 values: exact
    return ((dr.norms(Q)[:, None] + dr.norms(X)[None, :]).astype(F32) - F32(2) * acc).astype(F32)


KINDS = ("randn", "full24", "alternating", "huge_column", "lo_subnormal")
WIDTHS = (1, 15, 16, 17, 64, 1024)


def rows(kind, n, F, seed):
    """float32 rows [n, F].
    randn         standard normal
    full24        random 24-bit significands with the last bit set, 2^e, e in -2 .. 2, random signs: every part is inexact
    alternating   a common row of magnitude about 1 with alternating signs plus 2^-6 randn: q.x cancels column by column
    huge_column   randn with column 0 scaled by 2^30: one product carries the sum, the others fall below its last bits
    lo_subnormal  even columns randn, odd columns randn 2^-120: their hi parts are normal, their lo parts (2^-128 and
                  below) subnormal, and so are the products of two of them"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, F))
    if kind == "full24":
        X = (rng.integers(2 ** 23, 2 ** 24, (n, F)) | 1) * 2.0 ** (rng.integers(-2, 3, (n, F)) - 23) * rng.choice([-1.0, 1.0], (n, F))
    elif kind == "alternating":
        X = (1.0 + 0.25 * rng.random(F)) * np.where(np.arange(F) % 2 == 0, 1.0, -1.0) + 2.0 ** -6 * X
    elif kind == "huge_column":
        X[:, 0] *= 2.0 ** 30
    elif kind == "lo_subnormal":
        X[:, 1::2] *= 2.0 ** -120
        if F == 1:
            X *= 2.0 ** -120
    elif kind != "randn":
        raise ValueError(kind)
    return np.ascontiguousarray(X, F32)
