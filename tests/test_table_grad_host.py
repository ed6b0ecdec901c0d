"""Training through a neighbour table's weights, without a device: the exported names and the header's contract, the
float32 models of tests/_table_grad_ref.py against their float64 references at the bounds the device tests use (so a bound
has room for the documented order before the device is asked), the C entries' refusals (every pointer is host memory:
nothing is launched) and what ops.knn_dist, ops.knn_aggr(weight_grad=True) and DynamicHypergraphConv(learn_distances=True)
refuse before a device is touched, in which order."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _table_grad_ref as gr  # noqa: E402
import _table_ref as tr  # noqa: E402

SYMBOLS = ("hg_table_dist_f32", "hg_table_gather_diff_f32", "hg_table_gather_t_diff_f32", "hg_table_dot_f32")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _assert_close(y, ref, what=""):
    """Class (b) of tests/test_gpu_parity.py, as tests/test_table_gpu.py states it."""
    bad = ~(np.abs(y - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref)))
    assert not bad.any(), "%s: 1e-5 max(1, |ref|): %d off, worst %g" % (what, bad.sum(), np.abs(y - ref).max())
    bad = ~np.isclose(y, ref, rtol=1e-4, atol=1e-6)
    assert not bad.any(), "%s: allclose(1e-4, 1e-6): %d off, worst %g" % (what, bad.sum(), np.abs(y - ref).max())


def test_exports(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "hg_aggr.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert "%s(" % name in header, name
    assert "DOT ORDER:" in header and "t[l xor o]" in header  # the order of the dot products is part of the header
    assert hg.ops.knn_dist is hg.knn_graph.knn_dist and hg.knn_dist is hg.ops.knn_dist
    assert L.hg_version() == 410


def test_fma_model_is_correctly_rounded():
    """Against exact rational arithmetic, on cases that round twice through float64: a product that ends exactly half way
    between two float32 numbers once a tiny addend is absorbed."""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 2.0 ** rng.integers(-40, 20, 4000)).astype(np.float32)
    a[:3], b[:3] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)  # 1 + 2^-11 + 2^-24: a tie of float32 at 1 + 2^-11
    c[:3] = np.float32(2.0 ** -60), np.float32(-2.0 ** -60), 0
    got = gr.fma32(a, b, c)

    def rnd(x):  # a Fraction to the nearest float32, ties to even
        f = np.float32(float(x))
        lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
        best = min((lo, f, hi), key=lambda t: (abs(Fraction(float(t)) - x), int(np.float32(t).view(np.uint32)) & 1))
        return np.float32(best)

    for t in range(4000):
        want = rnd(Fraction(float(a[t])) * Fraction(float(b[t])) + Fraction(float(c[t])))
        assert got[t] == want, (t, a[t], b[t], c[t])
    assert got[0] > got[2] == np.float32(1 + 2.0 ** -11) and got[1] == got[2]  # the tie is to even unless the addend breaks it


@pytest.mark.parametrize("F", [1, 3, 4, 20, 64, 260])
def test_dist_model(F):
    rng = np.random.default_rng(F)
    n, rows, k = 40, 23, 5
    X = rng.standard_normal((n, F)).astype(np.float32)
    Q = rng.standard_normal((rows, F)).astype(np.float32)
    idx = rng.integers(-1, n + 1, (rows, k)).astype(np.int32)
    got, ref = gr.dist(idx, X, Q), gr.dist64(idx, X, Q)
    # F + 2 rounded steps on non-negative terms: the relative error of the sum is below (F + 2) u
    assert (np.abs(got - ref) <= (F + 2) * gr.U32 * ref).all()
    out = (idx < 0) | (idx >= n)
    assert out.any() and not got[out].any() and not np.signbit(got).any()
    # integer-valued rows: exact, and a row against itself exactly +0.0
    Xi = rng.integers(-8, 9, (n, F)).astype(np.float32)
    sq = rng.integers(0, n, (n, k)).astype(np.int32)
    sq[:, 0] = np.arange(n)
    got = gr.dist(sq, Xi)
    assert np.array_equal(got, gr.dist64(sq, Xi)) and not got[:, 0].any()


@pytest.mark.parametrize("F", [1, 3, 4, 20, 64, 260])
def test_difference_gather_models(F):
    """Both gathers against float64 at the device tests' rule, on inputs scaled so that |ref| <= 1 dominates; the centre of a
    duplicate row gives exactly 0; on integers the long-row order cannot matter."""
    rng = np.random.default_rng(10 + F)
    rows, k, n = 31, 6, 19
    idx = rng.integers(-1, n + 1, (rows, k)).astype(np.int32)
    ptr, pos = tr.transpose(idx, n)
    X = (rng.standard_normal((n, F)) * 0.3).astype(np.float32)
    Q = (rng.standard_normal((rows, F)) * 0.3).astype(np.float32)
    X[idx[4, 1] if 0 <= idx[4, 1] < n else 0] = Q[4]
    dD = (rng.standard_normal((rows, k)) * 0.1).astype(np.float32)
    g = (2 * dD).astype(np.float32).reshape(-1)
    dQ64, dX64 = gr.dist_grad64(idx, dD, X, Q)
    assert np.abs(dQ64).max() <= 2 and np.abs(dX64).max() <= 2  # of the order of 1: the absolute part of the rule decides
    _assert_close(gr.gather_diff(idx, Q, X, g), dQ64, "dQ, F = %d" % F)
    _assert_close(gr.gather_t_diff(idx, ptr, pos, X, Q, g), dX64, "dX, F = %d" % F)
    same = np.tile(X[:1], (rows, 1))
    assert not gr.gather_diff(np.zeros((rows, k), np.int32), same, X, g).any()
    # a hub table (rows above HG_TABLE_SEQ_MAX): integer values, every order gives the same bits
    t = tr.hub_table(min(F, 12), True, lengths=(129, 130, 515, 1000))
    hi, hn, hF = t["idx"], t["n"], min(F, 12)
    hptr, hpos = tr.transpose(hi, hn)
    src = rng.integers(-4, 5, (hi.shape[0], hF)).astype(np.float32)
    ctr = rng.integers(-4, 5, (hn, hF)).astype(np.float32)
    w = rng.integers(1, 4, hi.size).astype(np.float32)
    got = gr.gather_t_diff(hi, hptr, hpos, ctr, src, w)
    want = np.zeros((hn, hF))
    for v in range(hn):
        p = hpos[hptr[v]:hptr[v + 1]]
        want[v] = ((ctr[v].astype(np.float64) - src[p // 2]) * w[p][:, None]).sum(0)
    assert np.array_equal(got, want) and np.abs(want).max() < 2 ** 24
    assert tr._term.__module__ == "_table_ref"  # the plain term is back in place


@pytest.mark.parametrize("F,aligned", [(1, True), (3, True), (4, True), (4, False), (20, True), (64, True), (260, True), (260, False)])
def test_table_dot_model(F, aligned):
    rng = np.random.default_rng(20 + F)
    rows, k, n = 9, 4, 13
    idx = rng.integers(-1, n + 1, (rows, k)).astype(np.int32)
    A, C = (rng.standard_normal((n, F)).astype(np.float32) for _ in range(2))
    B, D = (rng.standard_normal((rows, F)).astype(np.float32) for _ in range(2))
    sc = rng.standard_normal(n).astype(np.float32)
    c, L = gr.dot_shape(F, aligned)
    assert L & (L - 1) == 0 and L <= 64 and c == (4 if F % 4 == 0 and aligned else 1) and L >= min(-(-F // c), 64) > L // 2
    for args in ((None, None, None), (sc, None, None), (None, C, D), (sc, C, D)):
        got = gr.table_dot(idx, A, B, *args, aligned16=aligned)
        ref, mass = gr.table_dot64(idx, A, B, *args)
        assert (np.abs(got - ref) <= gr.dot_bound(F, mass)).all(), (F, aligned)
        out = ((idx < 0) | (idx >= n)).reshape(-1)
        assert out.any() and not got[out].any()
    # integers: exact in every order
    Ai, Bi = rng.integers(-3, 4, (n, F)).astype(np.float32), rng.integers(-3, 4, (rows, F)).astype(np.float32)
    assert np.array_equal(gr.table_dot(idx, Ai, Bi, aligned16=aligned), gr.table_dot64(idx, Ai, Bi)[0])


def test_weight_gradient_reference_is_the_derivative():
    """dw64 against central differences of the float64 operator, and the formula the backward uses against dw64."""
    rng = np.random.default_rng(3)
    rows, k, n, F = 7, 3, 6, 4
    idx = rng.integers(0, n, (rows, k)).astype(np.int32)
    idx[2, 1] = idx[2, 0]
    X, dY = rng.standard_normal((n, F)), rng.standard_normal((n, F))
    w = rng.random(rows * k) + 0.5
    degE, degV = rng.random(rows) + 0.5, rng.random(n) + 0.5
    dw = gr.dw64(idx, X, dY, w, degE, degV)
    for p in range(rows * k):
        hi, lo = w.copy(), w.copy()
        hi[p] += 1e-6
        lo[p] -= 1e-6
        num = ((tr.aggr(idx, X, hi, degE, degV) - tr.aggr(idx, X, lo, degE, degV)) * dY).sum() / 2e-6
        assert abs(num - dw[p]) <= 1e-6 * max(1.0, abs(dw[p])), p
    Xe = degE[:, None] * (tr._dense64(idx, n, w) @ X)
    G = degE[:, None] * (tr._dense64(idx, n, w) @ (degV[:, None] * dY))
    got, _ = gr.table_dot64(idx, dY, Xe, degV, X, G)
    assert np.allclose(got, dw, rtol=1e-12, atol=1e-12)
    # and the gradients of dist
    Q = rng.standard_normal((rows, F))
    dD = rng.standard_normal((rows, k))
    dQ, dX = gr.dist_grad64(idx, dD, X, Q)
    h = np.zeros_like(X)
    h[3, 2] = 1e-6
    num = ((gr.dist64(idx, X + h, Q) - gr.dist64(idx, X - h, Q)) * dD).sum() / 2e-6
    assert abs(num - dX[3, 2]) <= 1e-6 * max(1.0, abs(dX[3, 2]))
    h = np.zeros_like(Q)
    h[1, 0] = 1e-6
    num = ((gr.dist64(idx, X, Q + h) - gr.dist64(idx, X, Q - h)) * dD).sum() / 2e-6
    assert abs(num - dQ[1, 0]) <= 1e-6 * max(1.0, abs(dQ[1, 0]))


def test_c_refusals_before_any_device_call(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    rows, k, n, F = 4, 3, 4, 8
    idx = np.zeros((rows, k), np.int32)
    ptr, pos = np.zeros(n + 1, np.int32), np.zeros(rows * k, np.int32)
    src, ctr, dst = (np.zeros((rows, F), np.float32) for _ in range(3))
    out = np.zeros(rows * k, np.float32)
    null = ctypes.c_void_p()
    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED

    def p(a):
        return null if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def gather(i=idx, s=src, c=ctr, d=dst, r=rows, kk=k, nn=n, f=F):
        return L.hg_table_gather_diff_f32(p(i), r, kk, nn, f, p(s), null, null, null, p(c), p(d), null)

    def gather_t(pt=ptr, ps=pos, s=src, c=ctr, d=dst, r=rows, kk=k, nn=n, f=F):
        return L.hg_table_gather_t_diff_f32(p(pt), p(ps), r, kk, nn, f, p(s), null, null, null, p(c), p(d), null)

    def dist(i=idx, q=src, x=ctr, d=out, r=rows, kk=k, nn=n, f=F):
        return L.hg_table_dist_f32(p(i), r, kk, nn, f, p(q), p(x), p(d), null)

    def dot(i=idx, a=src, b=ctr, c=None, dd=None, o=out, r=rows, kk=k, nn=n, f=F):
        return L.hg_table_dot_f32(p(i), r, kk, nn, f, p(a), null, p(b), p(c), p(dd), p(o), null)

    for call in (gather, gather_t):
        assert call(s=None) == INV and b"null src or dst" in L.hg_last_error()
        assert call(d=None) == INV
        assert call(c=None) == INV and b"null ctr" in L.hg_last_error()
        assert call(f=0) == INV and call(r=0) == INV and call(nn=0) == INV
        assert call(kk=65) == INV and b"k must be in 1 .. 64" in L.hg_last_error()
        assert call(kk=0, f=0) == INV and b"at least 1" in L.hg_last_error()  # the sizes before k
        assert call(r=2 ** 25, kk=64) == INV and b"2^31" in L.hg_last_error()
        assert call(s=None, f=0) == INV and b"null" in L.hg_last_error()  # the pointers before the sizes
    assert gather(i=None) == INV and b"null idx" in L.hg_last_error()
    assert gather_t(pt=None) == INV and gather_t(ps=None) == INV and b"null ptr_v or pos_v" in L.hg_last_error()
    for call, names in ((dist, ("q", "x", "d")), (dot, ("a", "b", "o"))):
        assert call(i=None) == INV and b"null" in L.hg_last_error()
        for name in names:
            assert call(**{name: None}) == INV and b"null" in L.hg_last_error(), name
        assert call(f=0) == INV and call(r=0) == INV and call(nn=0) == INV
        assert call(kk=65) == INV and b"k must be in 1 .. 64" in L.hg_last_error()
        assert call(kk=0, f=0) == INV and b"at least 1" in L.hg_last_error()
        assert call(r=2 ** 25, kk=64) == INV and b"2^31" in L.hg_last_error()
    assert dot(c=src) == INV and b"both" in L.hg_last_error() and dot(dd=src) == INV
    assert dot(c=src, f=0) == INV and b"both" in L.hg_last_error()  # the pair before the sizes
    odd = np.zeros(rows * F * 4 + 8, np.uint8)[1:]
    oddp = ctypes.c_void_p(odd.ctypes.data)
    assert L.hg_table_gather_diff_f32(p(idx), rows, k, n, F, p(src), null, null, null, oddp, p(dst), null) == UNS
    assert L.hg_table_dist_f32(p(idx), rows, k, n, F, oddp, p(ctr), p(out), null) == UNS
    assert L.hg_table_dot_f32(p(idx), rows, k, n, F, p(src), null, oddp, null, null, p(out), null) == UNS
    assert not dst.any() and not out.any()


def test_python_refusals_and_their_order(hg):
    ops = hg.ops
    idx = torch.zeros(6, 3, dtype=torch.int32)
    X = torch.zeros(6, 4)
    w = torch.zeros(18)
    # knn_dist: dtypes (TypeError), then shapes (ValueError), then the device (RuntimeError)
    for bad in (idx.long(), idx.float(), [[0]]):
        with pytest.raises(TypeError, match="int32"):
            ops.knn_dist(bad, X)
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            ops.knn_dist(idx, X.to(dt))
        with pytest.raises(TypeError, match="float32"):
            ops.knn_dist(idx, X, queries=X.to(dt))
        with pytest.raises(TypeError, match="float32"):  # the dtype before the shape
            ops.knn_dist(torch.zeros(6, 65, dtype=torch.int32), X.to(dt))
    with pytest.raises(TypeError, match="int32"):
        ops.knn_dist(idx, X, transpose=(torch.zeros(7), torch.zeros(18, dtype=torch.int32)))
    with pytest.raises(TypeError, match="pair"):
        ops.knn_dist(idx, X, transpose=torch.zeros(7, dtype=torch.int32))
    for bad in (torch.zeros(6, dtype=torch.int32), torch.zeros(6, 0, dtype=torch.int32), torch.zeros(6, 65, dtype=torch.int32),
                torch.zeros(0, 3, dtype=torch.int32)):
        with pytest.raises(ValueError):
            ops.knn_dist(bad, X)
    with pytest.raises(ValueError, match="X must be"):
        ops.knn_dist(idx, torch.zeros(6))
    with pytest.raises(ValueError, match="one row per row of X"):
        ops.knn_dist(idx, torch.zeros(9, 4))
    with pytest.raises(ValueError, match="queries must be"):
        ops.knn_dist(idx, torch.zeros(9, 4), queries=torch.zeros(6, 5))
    with pytest.raises(ValueError, match="queries must be"):
        ops.knn_dist(idx, torch.zeros(9, 4), queries=torch.zeros(5, 4))
    with pytest.raises(ValueError, match="transpose must be"):
        ops.knn_dist(idx, X, transpose=(torch.zeros(6, dtype=torch.int32), torch.zeros(18, dtype=torch.int32)))
    for call in (lambda: ops.knn_dist(idx, X), lambda: ops.knn_dist(idx, torch.zeros(9, 4), queries=X),
                 lambda: ops.knn_dist(idx, X.clone().requires_grad_()),
                 lambda: ops.knn_dist(idx, X, transpose=(torch.zeros(7, dtype=torch.int32), torch.zeros(18, dtype=torch.int32)))):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    # knn_aggr: the default refuses a weight that wants a gradient with the old message; weight_grad=True lets the weight
    # through to the device check and still refuses the scales
    with pytest.raises(RuntimeError, match="weight gets no gradient from knn_aggr: pass weight.detach\\(\\)"):
        ops.knn_aggr(idx, X, weight=w.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="weight gets no gradient"):
        ops.knn_aggr(idx, X, weight=w.clone().requires_grad_(), weight_grad=False)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.knn_aggr(idx, X, weight=w.clone().requires_grad_(), weight_grad=True)
    with pytest.raises(RuntimeError, match="degE gets no gradient"):
        ops.knn_aggr(idx, X, weight=w.clone().requires_grad_(), degE=torch.zeros(6, 1, requires_grad=True), weight_grad=True)
    with pytest.raises(RuntimeError, match="degV gets no gradient"):
        ops.knn_aggr(idx, X, weight=w, degV=torch.zeros(6, requires_grad=True), weight_grad=True)
    with pytest.raises(ValueError, match="weight must be"):  # the shape before the gradient and the device
        ops.knn_aggr(idx, X, weight=torch.zeros(17, requires_grad=True), weight_grad=True)
    # the layer
    for kw in (dict(), dict(probabilistic=True), dict(device_graph=True)):
        with pytest.raises(ValueError, match="learn_distances"):
            hg.DynamicHypergraphConv(4, 4, k=3, learn_distances=True, **kw)
    layer = hg.DynamicHypergraphConv(4, 4, k=3, probabilistic=True, device_graph=True, learn_distances=True)
    assert layer.learn_distances and not hg.DynamicHypergraphConv(4, 4, k=3, probabilistic=True, device_graph=True).learn_distances
    assert [n for n, _ in layer.named_parameters()] == ["lin.weight"]
    with pytest.raises(RuntimeError, match="GPU"):
        layer(X)
