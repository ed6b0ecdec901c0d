"""ops.knn(form="dot") on bfloat16 rows in numpy: CPU, test infrastructure only (include/hg_aggr.h, hg_knn_dot_bf16).

The scheme is tests/_knn_dot_ref.py's with one change, the bound: E1b in place of E1.  This module has
    to_bf16       float32 values rounded to bfloat16 (kept as float32: every bfloat16 value is one)
    bound_bf16    E1b [nq] in float32, operation for operation what the kernels compute
    MODELS        three models of one v_mfma_f32_32x32x16_bf16 accumulation step, acc' = acc + sum of 16 exact products --
                  sequential round-to-nearest, a pairwise tree, and alignment to the largest exponent with truncation and no
                  guard bit -- each with and without flushing subnormal products and partial sums to zero
    estimates     d~ under a model: float32 norms (an fma chain), G = ceil(F / 16) steps, d~ = (n2q + n2x) - 2 s~
    KINDS / rows  the adversarial inputs of the host test and of the device test
    scheme, certifiable, never_certifiable: _knn_dot_ref's with E1b (the module's bound is swapped while they run)
"""
import contextlib

import numpy as np
import torch

import _knn_dot_ref as dr
import _knn_ref as kr

F32 = np.float32
U = F32(2.0 ** -24)
TINY = 2.0 ** -126  # the smallest normal float32


def to_bf16(x):
    """Round to nearest even to bfloat16; the values, as float32."""
    return torch.from_numpy(np.ascontiguousarray(x, F32)).to(torch.bfloat16).float().numpy()


def _bound_bf16(Q, X):
    """(E1b, n2q + n2max), both float32 [nq]: E1b = C_b u (n2q + n2max) + (65 G + 1) 2^-126, G = ceil(F / 16),
    C_b = (F + 34 G + 4)(1 + 1/64) rounded up."""
    F = np.asarray(X).shape[1]
    assert 1 <= F <= dr.F_MAX
    total = (dr.norms(Q) + dr.norms(X).max()).astype(F32)
    G = (F + 15) // 16
    c2 = F + 34 * G + 4
    C = F32(c2 + (c2 >> 6) + 1) * U
    with np.errstate(over="ignore", invalid="ignore"):
        return (C * total + F32(65 * G + 1) * F32(TINY)).astype(F32), total


def bound_bf16(Q, X):
    return _bound_bf16(Q, X)[0]


# ---- models of one accumulation step: acc float32 [...], P float64 [..., 16] exact products --------------------------------

def _flush(x, flush):
    return np.where(np.abs(x) < TINY, 0.0, x) if flush else x


def step_sequential(acc, P, flush):
    """acc + p_0, + p_1, ...: every addition rounded to nearest float32."""
    P = _flush(P, flush)
    for i in range(P.shape[-1]):
        acc = _flush((acc.astype(np.float64) + P[..., i]).astype(F32), flush)
    return acc


def step_tree(acc, P, flush):
    """The 16 products summed pairwise, every addition rounded to nearest float32, then added to acc."""
    level = _flush(P, flush).astype(F32)  # a product of two bfloat16 values is a float32 value
    while level.shape[-1] > 1:
        level = _flush((level[..., 0::2].astype(np.float64) + level[..., 1::2].astype(np.float64)).astype(F32), flush)
    return _flush((acc.astype(np.float64) + level[..., 0].astype(np.float64)).astype(F32), flush)


def step_truncate(acc, P, flush):
    """All 17 terms aligned to the largest exponent and truncated there to 24 bits, no guard bit; the exact sum of those is
    truncated to 24 significant bits."""
    terms = np.concatenate([acc.astype(np.float64)[..., None], _flush(P, flush)], axis=-1)
    big = np.abs(terms).max(axis=-1)
    _, e = np.frexp(big)  # big = m 2^e, m in [0.5, 1)
    quantum = np.ldexp(1.0, e - 24)  # 24 bits of the largest term
    with np.errstate(invalid="ignore", divide="ignore"):
        total = (np.trunc(terms / quantum[..., None]) * quantum[..., None]).sum(axis=-1)  # integers below 17 2^24: exact
        total = np.where(big == 0, 0.0, total)
        _, e2 = np.frexp(total)
        q2 = np.ldexp(1.0, e2 - 24)
        total = np.where(total == 0, 0.0, np.trunc(total / q2) * q2)
    return _flush(total.astype(F32), flush)


MODELS = {"sequential": step_sequential, "tree": step_tree, "truncate": step_truncate}


def dots(Q, X, model, flush=False):
    """s~ [nq, n] float32: G steps of 16 columns, ascending, zeros past F."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    F = X.shape[1]
    G = (F + 15) // 16
    pad = 16 * G - F
    Qp, Xp = np.pad(Q, ((0, 0), (0, pad))), np.pad(X, ((0, 0), (0, pad)))
    acc = np.zeros((Q.shape[0], X.shape[0]), F32)
    step = MODELS[model]
    for g in range(G):
        P = Qp[:, None, 16 * g:16 * g + 16] * Xp[None, :, 16 * g:16 * g + 16]  # exact in float64
        acc = step(acc, P, flush)
    return acc


def estimates(Q, X, model, flush=False):
    s = dots(Q, X, model, flush)
    return ((dr.norms(Q)[:, None] + dr.norms(X)[None, :]).astype(F32) - F32(2) * s).astype(F32)


# ---- inputs ------------------------------------------------------------------------------------------------------------------

KINDS = ("randn", "positive", "alternating", "descending", "full8", "tiny", "huge")


def rows(kind, n, F, seed):
    """bfloat16-valued float32 rows [n, F].
    randn        standard normal
    positive     uniform in [0.5, 1.5): no cancellation, the sum of |q x| is the sum
    alternating  a common row of magnitude about 1 with alternating signs plus 2^-6 randn: q.x cancels column by column
    descending   magnitudes 2^-(c / 8) randn: late columns fall below the accumulator's last bit
    full8        significands with all eight bits set (1.9921875 2^e, e in -2 .. 2, random signs): products need 16 bits
    tiny / huge  randn scaled by 2^-70 / 2^60 F^-1/2: products near 2^-140 (subnormal) / norms near 2^120, short of overflow"""
    rng = np.random.default_rng(seed)
    if kind == "randn":
        X = rng.standard_normal((n, F))
    elif kind == "positive":
        X = rng.uniform(0.5, 1.5, (n, F))
    elif kind == "alternating":
        X = (1.0 + 0.25 * rng.random(F)) * np.where(np.arange(F) % 2 == 0, 1.0, -1.0) + 2.0 ** -6 * rng.standard_normal((n, F))
    elif kind == "descending":
        X = rng.standard_normal((n, F)) * 2.0 ** -(np.arange(F) / 8.0)
    elif kind == "full8":
        X = 1.9921875 * 2.0 ** rng.integers(-2, 3, (n, F)) * rng.choice([-1.0, 1.0], (n, F))
    elif kind == "tiny":
        X = rng.standard_normal((n, F)) * 2.0 ** -70
    elif kind == "huge":
        X = rng.standard_normal((n, F)) * 2.0 ** (60 - int(np.ceil(np.log2(F) / 2)))  # norms near 2^120 at every width: finite
    else:
        raise ValueError(kind)
    return to_bf16(X)


# ---- the scheme under E1b ------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _bf16_bound():
    saved = dr._bound
    dr._bound = _bound_bf16
    try:
        yield
    finally:
        dr._bound = saved


def scheme(*args, **kw):
    with _bf16_bound():
        return dr.scheme(*args, **kw)


def certifiable(*args, **kw):
    with _bf16_bound():
        return dr.certifiable(*args, **kw)


def never_certifiable(*args, **kw):
    with _bf16_bound():
        return dr.never_certifiable(*args, **kw)


def distances(Q, X):
    return kr.distances(Q, X)
