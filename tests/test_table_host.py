"""Aggregation over a neighbour table, without a device: the exported names, tests/_table_ref.py's transpose against the
definition written as loops, its float32 reference of the long-row order (every entry summed once, inside the device
tests' tolerance of float64, other bits under another tree), HG_TABLE_SEQ_MAX as the library was built, the workspace size and the C entries' refusals
(decided before any device call: every pointer here is host memory), and what ops.knn_transpose / ops.knn_aggr refuse
before a device is touched, in which order."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _table_ref as tr  # noqa: E402

SYMBOLS = ("hg_table_seq_max", "hg_table_transpose_workspace_bytes", "hg_table_transpose", "hg_table_gather_f32",
           "hg_table_gather_t_f32")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "hg_aggr.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert "%s(" % name in header, name
    assert "ASCENDING p" in header and "ORDER:" in header  # the order contract is part of the header
    assert L.hg_version() == 410  # detected by symbol: the version does not move
    for name in ("knn_transpose", "knn_aggr", "KnnHypergraph"):
        assert hasattr(hg, name), name
    assert hg.knn_aggr is hg.ops.knn_aggr and hg.knn_transpose is hg.ops.knn_transpose
    assert hg.KnnHypergraph is hg.knn_graph.KnnHypergraph
    makefile = open(os.path.join(ROOT, "hypergef_amd", "csrc", "Makefile")).read()
    assert "hg_table.hip" in makefile.split("SRCS")[1].split("\n")[0] and "hg_table.h" in makefile.split("HDRS")[1].split("\n")[0]
    assert "hg_table.hip" in makefile.split("\nasm:")[1].split("\n")[0]


def test_seq_max_of_the_library(hg):
    from hypergef_amd import _lib, knn_graph
    got = _lib.lib().hg_table_seq_max()
    assert got >= 64  # hop 0 (k <= 64 entries a row) is always sequential
    assert knn_graph.table_seq_max() == got
    header = open(os.path.join(ROOT, "include", "hg_aggr.h")).read()
    assert "#define HG_TABLE_SEQ_MAX %d" % got in header


def test_reference_transpose_agrees_with_the_loops():
    rng = np.random.default_rng(7)
    for rows, k, n in ((6, 3, 6), (5, 2, 9), (9, 4, 3), (1, 1, 1)):
        idx = rng.integers(-1, n + 1, (rows, k)).astype(np.int32)  # -1 and n are ignored
        idx[0, 0] = 0
        if k > 1:
            idx[-1, 1] = idx[-1, 0]  # a duplicate within a row
        got, want = tr.transpose(idx, n), tr.transpose_loops(idx, n)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (rows, k, n)
        assert got[0][-1] == ((idx >= 0) & (idx < n)).sum() == got[1].shape[0]
    idx = np.array([[0, 2, 2], [1, 0, 3], [2, 0, 1], [3, 1, 2]], np.int32)
    ptr, pos = tr.transpose(idx)
    assert ptr.tolist() == [0, 3, 6, 10, 12]
    assert pos.tolist() == [0, 4, 7, 3, 8, 10, 1, 2, 6, 11, 5, 9]


def test_reference_gathers_are_one_another_s_transpose():
    rng = np.random.default_rng(8)
    rows, k, n, F = 7, 3, 5, 4
    idx = rng.integers(0, n, (rows, k)).astype(np.int32)
    X = rng.standard_normal((n, F)).astype(np.float32)
    w = rng.random(rows * k).astype(np.float32)
    degE, degV = rng.random(rows).astype(np.float32), rng.random(n).astype(np.float32)
    ptr, pos = tr.transpose(idx, n)
    Y = tr.gather_t(ptr, pos, k, tr.gather(idx, X, w, None, degE), w, None, degV)
    assert np.allclose(Y, tr.aggr(idx, X, w, degE, degV), rtol=1e-5, atol=1e-6)
    dY = rng.standard_normal((n, F)).astype(np.float32)
    dX = tr.gather_t(ptr, pos, k, tr.gather(idx, dY, w, degV, degE), w)
    assert np.allclose(dX, tr.aggr_grad(idx, dY, w, degE, degV), rtol=1e-5, atol=1e-6)
    # <Y, dY> = <X, dX>: aggr_grad is aggr's adjoint
    assert np.isclose((tr.aggr(idx, X, w, degE, degV) * dY).sum(), (X * tr.aggr_grad(idx, dY, w, degE, degV)).sum())
    empty = tr.gather_t(np.array([0, 0, 2], np.int32), np.array([0, 1], np.int32), 1, X[:2], None, None,
                        np.array([np.inf, 1.0], np.float32))
    assert not empty[0].any() and not np.signbit(empty[0]).any()


def _hub_inputs(t, F, seed, integer):
    """src [rows, F], w [rows k], src_scale [rows], dst_scale [n] for a hub table: small integers (every order of a sum is
    exact) or randn with weights in [0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    rows, k = t["idx"].shape
    if integer:
        draw = lambda lo, hi, size: rng.integers(lo, hi, size).astype(np.float32)  # noqa: E731
        return draw(-4, 5, (rows, F)), draw(1, 4, rows * k), draw(-2, 3, rows), draw(-2, 3, t["n"])
    return (rng.standard_normal((rows, F)).astype(np.float32), (rng.random(rows * k) + 0.5).astype(np.float32),
            rng.standard_normal(rows).astype(np.float32), rng.standard_normal(t["n"]).astype(np.float32))


def test_long_row_shapes_of_the_header():
    for F, aligned, P in tr.LONG_ROW_WIDTHS:
        c, L, R, got, P2 = tr.long_row_shape(F, aligned)
        assert got == P == 4 * R and R == 64 // L and L == min(-(-F // c), 64), (F, aligned)
        assert P2 >= P > P2 // 2 and P2 & (P2 - 1) == 0
    assert [tr.long_row_shape(F, a)[4] for F, a, _ in tr.LONG_ROW_WIDTHS] == [256, 128, 256, 64, 64, 128, 4, 4]
    assert tr.long_row_shape(32)[3] == 32 and tr.long_row_shape(33)[3] == 4  # the widths of test_long_rows


@pytest.mark.parametrize("F,aligned,P", tr.LONG_ROW_WIDTHS)
def test_ordered_reference_sums_every_entry_once(F, aligned, P):
    """Integer-valued rows, weights and scales: every partial sum is an integer below 2^24, so every order gives the same
    bits and the pieces-and-tree reference must equal the sequential one -- unless it drops or repeats an entry."""
    t = tr.hub_table(F, aligned, lengths=(129, 130, 515, 1000))
    assert sorted(set(t["lens"])) == [129, 130, 515, 1000] and t["P"] == P
    ptr, pos = tr.transpose(t["idx"], t["n"])
    assert [int(ptr[h + 1] - ptr[h]) for h in t["hubs"]] == t["lens"]
    assert ptr[t["full"] + 1] - ptr[t["full"]] == 128 and ptr[t["empty"] + 1] == ptr[t["empty"]]
    src, w, ss, ds = _hub_inputs(t, F, 100 + F, integer=True)
    for args in ((None, None, None), (w, ss, ds)):
        want = tr.gather_t(ptr, pos, 2, src, *args)
        got = tr.gather_t_ordered(ptr, pos, 2, src, *args, aligned16=aligned)
        assert np.abs(want).max() < 2 ** 24 and np.abs(want[t["hubs"]]).max() > 0
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))


@pytest.mark.parametrize("F,aligned,P", tr.LONG_ROW_WIDTHS)
def test_ordered_reference_is_within_the_device_tolerance_of_float64(F, aligned, P):
    from test_table_gpu import _assert_close
    t = tr.hub_table(F, aligned)
    idx, n = t["idx"], t["n"]
    ptr, pos = tr.transpose(idx, n)
    src, w, _, _ = _hub_inputs(t, F, 200 + F, integer=False)
    deg = np.diff(ptr).astype(np.float64)
    degV = np.where(deg > 0, np.maximum(deg, 1) ** -0.5, 1.0).astype(np.float32)  # the operator's vertex scale
    got = tr.gather_t_ordered(ptr, pos, 2, src, w, None, degV, aligned16=aligned)
    ref = np.zeros((n, F))
    for v in range(n):
        p = pos[ptr[v]:ptr[v + 1]]
        ref[v] = degV[v].astype(np.float64) * (src[p // 2].astype(np.float64) * w[p].astype(np.float64)[:, None]).sum(0)
    _assert_close(got, ref, "gather_t_ordered, F = %d" % F)
    # rows up to seq_max entries, the one of exactly seq_max included, are gather_t's
    seq = tr.gather_t(ptr, pos, 2, src, w, None, degV)
    short = np.diff(ptr) <= 128
    assert short[t["full"]] and not short[t["hubs"]].any()
    assert np.array_equal(got[short], seq[short])
    if F == 3:  # the same rows under a longer sequential limit: a hub of 129 and one of 130 entries become gather_t's too
        got = tr.gather_t_ordered(ptr, pos, 2, src, w, None, degV, seq_max=130)
        short = np.diff(ptr) <= 130
        assert short.sum() == n - len(t["hubs"]) + 4 and np.array_equal(got[short], seq[short])


def test_ordered_reference_tells_another_tree_apart():
    """A tree that starts at P / 2 instead of P' / 2 (F = 3: P = 84, P' = 128) gives other bits on one randn hub, so the
    bit-for-bit device test can fail on a wrong order."""
    rng = np.random.default_rng(9)
    P, P2 = tr.long_row_shape(3)[3:]
    assert (P, P2) == (84, 128)
    terms = rng.standard_normal((1000, 3)).astype(np.float32)
    live = np.ones(1000, bool)
    right = tr.long_row_sum(terms, live, P)
    assert np.array_equal(right, tr.long_row_sum(terms, live, P, first_stride=P2 // 2))
    assert not np.array_equal(right, tr.long_row_sum(terms, live, P, first_stride=P // 2))
    assert not np.array_equal(right, np.add.accumulate(terms, axis=0, dtype=np.float32)[-1])  # nor the sequential sum
    # an ignored entry keeps its place: the pieces are those of the whole length, not of the live entries
    live[[0, 500, 999]] = False
    kept = tr.long_row_sum(terms, live, P)
    zeroed = terms.copy()
    zeroed[~live] = 0
    assert np.array_equal(kept, tr.long_row_sum(zeroed, np.ones(1000, bool), P))
    assert not np.array_equal(kept, tr.long_row_sum(terms[live], np.ones(997, bool), P))


@pytest.mark.parametrize("F", [5, 32])
def test_composed_float32_operator_is_within_the_device_tolerance(F):
    """gather then gather_t_ordered, the device's two launches in float32 on the CPU, against the float64 operator and its
    gradient over the hub table the device test uses: the tolerance has room for the order before the device is asked."""
    from test_table_gpu import _assert_close
    t = tr.hub_operator_case(F)
    idx, n, w, degE, degV = t["idx"], t["n"], t["w"], t["degE"], t["degV"]
    ptr, pos = tr.transpose(idx, n)
    Y = tr.gather_t_ordered(ptr, pos, 2, tr.gather(idx, t["X"], w, None, degE), w, None, degV)
    _assert_close(Y, tr.aggr(idx, t["X"], w, degE, degV), "Y, F = %d" % F)
    dX = tr.gather_t_ordered(ptr, pos, 2, tr.gather(idx, t["G"], w, degV, degE), w)
    _assert_close(dX, tr.aggr_grad(idx, t["G"], w, degE, degV), "dX, F = %d" % F)


def test_workspace_and_c_refusals_before_any_device_call(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    for rows, k, n in ((1, 1, 1), (300, 10, 300), (50000, 10, 50000), (7, 64, 1000000), (2 ** 25 - 1, 64, 5)):
        got = L.hg_table_transpose_workspace_bytes(rows, k, n)
        assert 4 * rows * k <= got <= 5 * rows * k + 4096, (rows, k, n, got)  # the second buffer and the tile histograms
    for args in ((0, 1, 1), (1, 0, 1), (1, 65, 1), (1, 1, 0), (2 ** 25, 64, 5)):
        assert L.hg_table_transpose_workspace_bytes(*args) == 0, args

    rows, k, n, F = 4, 3, 4, 8
    idx = np.zeros((rows, k), np.int32)
    ptr, pos = np.zeros(n + 1, np.int32), np.zeros(rows * k, np.int32)
    src, dst = np.zeros((rows, F), np.float32), np.zeros((rows, F), np.float32)
    ws = np.zeros(1 << 16, np.uint8)
    null = ctypes.c_void_p()

    def p(a):
        return null if a is None else a.ctypes.data_as(ctypes.c_void_p)

    INV, UNS, WSP = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED, _lib.HG_ERR_WORKSPACE

    def transpose(i=idx, r=rows, kk=k, nn=n, pt=ptr, ps=pos, w=ws, wb=None):
        return L.hg_table_transpose(p(i), r, kk, nn, p(pt), p(ps), p(w), (0 if w is None else w.nbytes) if wb is None else wb, null)

    assert transpose(i=None) == INV and b"null" in L.hg_last_error()
    assert transpose(ps=None) == INV
    assert transpose(r=0) == INV and transpose(nn=0) == INV
    for kk in (0, -1, 65):
        assert transpose(kk=kk) == INV and b"k must be in 1 .. 64" in L.hg_last_error()
    assert transpose(i=None, kk=0) == INV and b"null" in L.hg_last_error()  # the pointers before k
    assert transpose(r=2 ** 25, kk=64) == INV and b"2^31" in L.hg_last_error()
    assert transpose(w=None) == WSP and transpose(wb=8) == WSP
    assert b"hg_table_transpose_workspace_bytes asks for" in L.hg_last_error()

    def gather(i=idx, s=src, d=dst, r=rows, kk=k, nn=n, f=F):
        return L.hg_table_gather_f32(p(i), r, kk, nn, f, p(s), null, null, null, p(d), null)

    def gather_t(pt=ptr, ps=pos, s=src, d=dst, r=rows, kk=k, nn=n, f=F):
        return L.hg_table_gather_t_f32(p(pt), p(ps), r, kk, nn, f, p(s), null, null, null, p(d), null)

    for call in (gather, gather_t):
        assert call(s=None) == INV and b"null src or dst" in L.hg_last_error()
        assert call(d=None) == INV
        assert call(f=0) == INV and call(r=0) == INV and call(nn=0) == INV
        assert call(kk=65) == INV and b"k must be in 1 .. 64" in L.hg_last_error()
        assert call(kk=0, f=0) == INV and b"at least 1" in L.hg_last_error()  # the sizes before k
        assert call(r=2 ** 25, kk=64) == INV and b"2^31" in L.hg_last_error()
    assert gather(i=None) == INV and b"null idx" in L.hg_last_error()
    assert gather_t(pt=None) == INV and gather_t(ps=None) == INV and b"null ptr_v or pos_v" in L.hg_last_error()
    odd = np.zeros(rows * F * 4 + 8, np.uint8)[1:]
    assert L.hg_table_gather_f32(p(idx), rows, k, n, F, ctypes.c_void_p(odd.ctypes.data), null, null, null, p(dst), null) == UNS
    assert not dst.any() and not ptr.any() and not pos.any() and not ws.any()


def test_python_refusals_and_their_order(hg):
    ops = hg.ops
    idx = torch.zeros(6, 3, dtype=torch.int32)
    X = torch.zeros(6, 4)
    w = torch.zeros(18)
    # TypeError: dtypes, before every shape
    for bad in (idx.long(), idx.float(), [[0]]):
        with pytest.raises(TypeError, match="int32"):
            ops.knn_transpose(bad)
        with pytest.raises(TypeError, match="int32"):
            ops.knn_aggr(bad, X)
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            ops.knn_aggr(idx, X.to(dt))
        with pytest.raises(TypeError, match="float32"):
            ops.knn_aggr(idx, X, weight=w.to(dt))
        with pytest.raises(TypeError, match="float32"):
            ops.knn_aggr(idx, X, degE=torch.zeros(6, dtype=dt))
        with pytest.raises(TypeError, match="float32"):
            ops.knn_aggr(idx, X, degV=torch.zeros(6, dtype=dt))
        with pytest.raises(TypeError, match="float32"):  # the dtype before the shape
            ops.knn_aggr(torch.zeros(6, 65, dtype=torch.int32), X.to(dt))
    with pytest.raises(TypeError, match="int32"):
        ops.knn_aggr(idx, X, transpose=(torch.zeros(7), torch.zeros(18, dtype=torch.int32)))
    with pytest.raises(TypeError, match="pair"):
        ops.knn_aggr(idx, X, transpose=torch.zeros(7, dtype=torch.int32))
    # ValueError: shapes and k
    for bad in (torch.zeros(6, dtype=torch.int32), torch.zeros(6, 0, dtype=torch.int32), torch.zeros(6, 65, dtype=torch.int32),
                torch.zeros(0, 3, dtype=torch.int32)):
        with pytest.raises(ValueError):
            ops.knn_transpose(bad)
        with pytest.raises(ValueError):
            ops.knn_aggr(bad, X)
    with pytest.raises(ValueError, match="k must be"):
        ops.knn_transpose(torch.zeros(6, 65, dtype=torch.int32))
    for n in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="n must be"):
            ops.knn_transpose(idx, n=n)
    with pytest.raises(ValueError, match="X must be"):
        ops.knn_aggr(idx, torch.zeros(6))
    with pytest.raises(ValueError, match="weight must be"):
        ops.knn_aggr(idx, X, weight=torch.zeros(17))
    with pytest.raises(ValueError, match="weight must be"):
        ops.knn_aggr(idx, X, weight=torch.zeros(3, 6))
    with pytest.raises(ValueError, match="degE must be"):
        ops.knn_aggr(idx, X, degE=torch.zeros(5))
    with pytest.raises(ValueError, match="degV must be"):
        ops.knn_aggr(idx, torch.zeros(9, 4), degV=torch.zeros(6))
    with pytest.raises(ValueError, match="transpose must be"):
        ops.knn_aggr(idx, X, transpose=(torch.zeros(6, dtype=torch.int32), torch.zeros(18, dtype=torch.int32)))
    # RuntimeError: a weight or scale that wants a gradient, with a message that says so; after the shapes, before the device
    for kw in (dict(weight=w.clone().requires_grad_()), dict(degE=torch.zeros(6, 1, requires_grad=True)),
               dict(degV=torch.zeros(6, requires_grad=True))):
        name = next(iter(kw))
        with pytest.raises(RuntimeError, match="%s gets no gradient" % name):
            ops.knn_aggr(idx, X, **kw)
    with pytest.raises(ValueError, match="weight must be"):  # the shape before the gradient
        ops.knn_aggr(idx, X, weight=torch.zeros(17, requires_grad=True))
    # what is left is the device
    for call in (lambda: ops.knn_transpose(idx), lambda: ops.knn_transpose(idx, n=9), lambda: ops.knn_aggr(idx, X),
                 lambda: ops.knn_aggr(idx, X, weight=w.reshape(6, 3), degE=torch.zeros(6, 1), degV=torch.zeros(6)),
                 lambda: ops.knn_aggr(idx, X.clone().requires_grad_(), weight=w),
                 lambda: ops.knn_aggr(idx, X, transpose=(torch.zeros(7, dtype=torch.int32), torch.zeros(18, dtype=torch.int32)))):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with torch.no_grad():  # no gradient is asked for: the weight's flag does not matter
        with pytest.raises(RuntimeError, match="GPU"):
            ops.knn_aggr(idx, X, weight=w.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="GPU"):
        hg.KnnHypergraph.build(X, 3)
    with pytest.raises(TypeError, match="float32"):
        hg.KnnHypergraph.build(X.double(), 3)
    layer = hg.DynamicHypergraphConv(4, 4, k=3, device_graph=True)
    assert layer.device_graph and not hg.DynamicHypergraphConv(4, 4, k=3).device_graph
    with pytest.raises(RuntimeError, match="GPU"):
        layer(X)
