"""Training through a neighbour table's weights on the device (-m gpu): ops.knn_dist against the search's own dist and
against the float32 model bit for bit, the two difference gathers bit for bit against the float32 models (the long-row order
included) and against float64, hg_table_dot_f32 against float64 at the dot-product bound and bit for bit against its model,
ops.knn_aggr(weight_grad=True) against the dense float64 gradient and the planned operator's, the whole path against a
float64 autograd restatement, DynamicHypergraphConv(learn_distances=True) eagerly and captured, and one case past 2^31
elements."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _table_grad_ref as gr  # noqa: E402
import _table_ref as tr  # noqa: E402
from test_table_gpu import _assert_close, _dev, _dev_rows, _np  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = (1, 3, 4, 20, 64, 260)  # scalar and 16-byte lanes, lane groups below 64 lanes, a second column pass


def _bits(t):
    return t.contiguous().view(torch.int32)


def _irregular(F, k, seed):
    """A table [rows, k] over n vertices with rows != n, rows no multiple of a workgroup's rows, a row naming one vertex twice
    and entries outside 0 .. n - 1; queries Q [rows, F] and rows X [n, F], one of X equal to a query that names it."""
    rng = np.random.default_rng(seed)
    rows, n = 77, 45
    idx = rng.integers(0, n, (rows, k)).astype(np.int32)
    X = rng.standard_normal((n, F)).astype(np.float32)
    Q = rng.standard_normal((rows, F)).astype(np.float32)
    if k > 1:
        idx[3, 1] = idx[3, 0]
        idx[5, k - 1], idx[6, 0] = -1, n
    else:
        idx[5, 0], idx[6, 0] = -1, n
    X[idx[9, 0]] = Q[9]  # an identical pair
    return idx, X, Q, rng


# ---- 1. dist against the search ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", WIDTHS)
def test_dist_is_the_search_s_dist(hg, F):
    rng = np.random.default_rng(F)
    n = 203
    for kind in ("integer", "randn"):
        Xn = (rng.integers(-3, 4, (n, F)) if kind == "integer" else rng.standard_normal((n, F))).astype(np.float32)
        Xn[17] = Xn[4]  # identical rows
        Qn = rng.standard_normal((37, F)).astype(np.float32)
        X, Q = _dev(Xn), _dev(Qn)
        for k in (1, 3, 10, 64):
            for form in ("difference", "dot"):
                idx, dist = hg.ops.knn(X, k, form=form)  # self_first
                got = hg.ops.knn_dist(idx, X)
                assert torch.equal(_bits(got), _bits(dist)), (F, kind, k, form)
                assert not got[:, 0].any()
                idx, dist = hg.ops.knn(X, k, self_first=False, form=form)
                assert torch.equal(_bits(hg.ops.knn_dist(idx, X)), _bits(dist)), (F, kind, k, form, "no self_first")
                idx, dist = hg.ops.knn(X, k, queries=Q, form=form)
                assert torch.equal(_bits(hg.ops.knn_dist(idx, X, queries=Q)), _bits(dist)), (F, kind, k, form, "queries")
        same = torch.tensor([[4, 17], [17, 4]], dtype=torch.int32, device=DEV)
        d = hg.ops.knn_dist(same, X, queries=X[[17, 4]].contiguous())
        assert not d.any() and not torch.signbit(d).any()


# ---- 2. dist on irregular tables -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("aligned", [True, False])
def test_dist_on_irregular_tables(hg, F, aligned):
    for k in (1, 3, 10, 64):
        idx, X, Q, _ = _irregular(F, k, 100 + F + k)
        got = hg.ops.knn_dist(_dev(idx), _dev_rows(X, aligned), queries=_dev_rows(Q, aligned))
        want = gr.dist(idx, X, Q)
        assert np.array_equal(_np(got).view(np.int32), want.view(np.int32)), (F, k, aligned)
        out = (idx < 0) | (idx >= X.shape[0])
        assert out.any() and not _np(got)[out].any() and not np.signbit(_np(got)).any()
        assert _np(got)[9, 0] == 0


# ---- 3. the difference gathers ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("aligned", [True, False])
def test_difference_gathers_bit_exact(hg, F, aligned):
    from hypergef_amd import knn_graph as kg
    for k in (1, 3, 10, 64):
        idx, X, Q, rng = _irregular(F, k, 200 + F + k)
        rows, n = idx.shape[0], X.shape[0]
        ptr, pos = tr.transpose(idx, n)
        assert np.diff(ptr).max() <= kg.table_seq_max() or k == 64
        w = rng.standard_normal(rows * k).astype(np.float32)
        sv, se = rng.standard_normal(n).astype(np.float32), rng.standard_normal(rows).astype(np.float32)
        idx_d, X_d, Q_d = _dev(idx), _dev_rows(X, aligned), _dev_rows(Q, aligned)
        ptr_d, pos_d = hg.ops.knn_transpose(idx_d, n)
        for use_w, use_src, use_dst in ((0, 0, 0), (1, 0, 0), (1, 1, 1)):
            a = (w if use_w else None, sv if use_src else None, se if use_dst else None)
            got = kg.table_gather(idx_d, X_d, *[_dev(x) for x in a], ctr=Q_d)
            want = gr.gather_diff(idx, Q, X, *a)
            assert np.array_equal(_np(got), want), ("gather_diff", F, k, aligned, use_w, use_src, use_dst)
            assert torch.equal(_bits(got), _bits(kg.table_gather(idx_d, X_d, *[_dev(x) for x in a], ctr=Q_d)))
            a = (a[0], a[2], a[1])
            got = kg.table_gather_t(ptr_d, pos_d, k, Q_d, *[_dev(x) for x in a], ctr=X_d)
            want = gr.gather_t_diff(idx, ptr, pos, X, Q, *a, aligned16=aligned, seq_max=kg.table_seq_max())
            assert np.array_equal(_np(got), want), ("gather_t_diff", F, k, aligned, use_w, use_src, use_dst)
            assert torch.equal(_bits(got), _bits(kg.table_gather_t(ptr_d, pos_d, k, Q_d, *[_dev(x) for x in a], ctr=X_d)))
        # the centre of a duplicate row: exactly 0, whatever the weight
        dup = np.tile(X[:1], (rows, 1))
        zero = kg.table_gather(_dev(np.zeros((rows, k), np.int32)), X_d, _dev(w), ctr=_dev_rows(dup, aligned))
        assert not zero.any()


@pytest.mark.parametrize("F,aligned,P", tr.LONG_ROW_WIDTHS)
def test_difference_gather_t_over_hubs(hg, F, aligned, P):
    """Vertex rows above HG_TABLE_SEQ_MAX in the header's pieces and tree, with the centre loaded per row: bit for bit."""
    from hypergef_amd import knn_graph as kg
    seq = kg.table_seq_max()
    t = tr.hub_table(F, aligned, seq, seed=F)
    idx, n, k = t["idx"], t["n"], 2
    rows = idx.shape[0]
    ptr, pos = tr.transpose(idx, n)
    assert (np.diff(ptr)[t["hubs"]] > seq).all() and t["P"] == P
    rng = np.random.default_rng(500 + F)
    src = rng.standard_normal((rows, F)).astype(np.float32)
    ctr = rng.standard_normal((n, F)).astype(np.float32)
    w = (rng.random(rows * k) + 0.5).astype(np.float32)
    ds = rng.standard_normal(n).astype(np.float32)
    ptr_d, pos_d = hg.ops.knn_transpose(_dev(idx), n)
    src_d, ctr_d = _dev_rows(src, aligned), _dev_rows(ctr, aligned)
    for a in ((None, None, None), (w, None, ds)):
        got = kg.table_gather_t(ptr_d, pos_d, k, src_d, *[_dev(x) for x in a], ctr=ctr_d)
        want = gr.gather_t_diff(idx, ptr, pos, ctr, src, *a, aligned16=aligned, seq_max=seq)
        bad = np.flatnonzero((_np(got) != want).any(1))
        assert np.array_equal(_np(got), want), "F = %d: rows %s differ (hubs %s)" % (F, bad.tolist(), t["hubs"])
        assert torch.equal(_bits(got), _bits(kg.table_gather_t(ptr_d, pos_d, k, src_d, *[_dev(x) for x in a], ctr=ctr_d)))
        assert not _np(got)[t["empty"]].any()


# ---- 4. dDist to dX / dQ ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", WIDTHS)
def test_dist_gradients_against_float64(hg, F):
    for k in (1, 3, 10, 64):
        idx, X, Q, rng = _irregular(F, k, 300 + F + k)
        s = 0.3 / np.sqrt(k)  # a vertex row has about 1.7 k entries: |ref| stays of the order of 1, where the rule is absolute
        X, Q = (X * np.float32(s)).astype(np.float32), (Q * np.float32(s)).astype(np.float32)
        dD = (rng.standard_normal(idx.shape) * 0.3).astype(np.float32)
        dQ64, dX64 = gr.dist_grad64(idx, dD, X, Q)
        assert np.abs(dQ64).max() <= 4 and np.abs(dX64).max() <= 4
        Xd, Qd = _dev(X).requires_grad_(True), _dev(Q).requires_grad_(True)
        dist = hg.ops.knn_dist(_dev(idx), Xd, queries=Qd)
        inputs = (Xd.data_ptr(), Qd.data_ptr())  # what is saved is a table-sized index array or an input itself
        assert all(t is None or t.numel() <= max(idx.size, X.shape[0] + 1) or t.data_ptr() in inputs for t in dist.grad_fn.saved_tensors)
        dX, dQ = torch.autograd.grad(dist, (Xd, Qd), _dev(dD))
        _assert_close(dX, dX64, "dX, F = %d, k = %d" % (F, k))
        _assert_close(dQ, dQ64, "dQ, F = %d, k = %d" % (F, k))
        dX2, dQ2 = torch.autograd.grad(hg.ops.knn_dist(_dev(idx), Xd, queries=Qd), (Xd, Qd), _dev(dD))
        assert torch.equal(_bits(dX), _bits(dX2)) and torch.equal(_bits(dQ), _bits(dQ2))
    # queries None: the two gathers in one gradient; self_first entries contribute exactly 0
    rng = np.random.default_rng(F)
    Xn = (rng.standard_normal((150, F)) * 0.3).astype(np.float32)
    X = _dev(Xn).requires_grad_(True)
    idx, _ = hg.ops.knn(X.detach(), 5)
    dD = (rng.standard_normal((150, 5)) * 0.3).astype(np.float32)
    (dX,) = torch.autograd.grad(hg.ops.knn_dist(idx, X), X, _dev(dD))
    dQ64, dX64 = gr.dist_grad64(_np(idx), dD, Xn)
    _assert_close(dX, dQ64 + dX64, "dX of a square table, F = %d" % F)
    only_self = torch.arange(150, dtype=torch.int32, device=DEV).reshape(150, 1)
    (dX,) = torch.autograd.grad(hg.ops.knn_dist(only_self, X), X, torch.ones(150, 1, device=DEV))
    assert not dX.any()


# ---- 5. hg_table_dot_f32 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("aligned", [True, False])
def test_table_dot(hg, F, aligned):
    from hypergef_amd import knn_graph as kg
    for k in (1, 3, 10, 64):
        idx, A, B, rng = _irregular(F, k, 400 + F + k)
        rows, n = idx.shape[0], A.shape[0]
        C = rng.standard_normal((n, F)).astype(np.float32)
        D = rng.standard_normal((rows, F)).astype(np.float32)
        sc = rng.standard_normal(n).astype(np.float32)
        idx_d = _dev(idx)
        dev = [_dev_rows(x, aligned) for x in (A, B, C, D)]
        for use_sc, use_cd in ((0, 0), (1, 0), (0, 1), (1, 1)):
            args = (sc if use_sc else None, C if use_cd else None, D if use_cd else None)
            dargs = (_dev(sc) if use_sc else None, dev[2] if use_cd else None, dev[3] if use_cd else None)
            got = kg.table_dot(idx_d, dev[0], dev[1], *dargs)
            ref, mass = gr.table_dot64(idx, A, B, *args)
            err = np.abs(_np(got) - ref)
            assert (err <= gr.dot_bound(F, mass)).all(), (F, k, aligned, use_sc, use_cd, (err / np.maximum(mass, 1e-30)).max())
            assert np.array_equal(_np(got), gr.table_dot(idx, A, B, *args, aligned16=aligned)), (F, k, aligned, use_sc, use_cd)
            assert torch.equal(_bits(got), _bits(kg.table_dot(idx_d, dev[0], dev[1], *dargs)))
            out = ((idx < 0) | (idx >= n)).reshape(-1)
            assert not _np(got)[out].any() and not np.signbit(_np(got)[out]).any()
        # a row's bits wherever it stands: the table rolled by 13 rows, with B and D
        roll = np.roll(np.arange(rows), 13)
        moved = kg.table_dot(_dev(idx[roll]), dev[0], _dev_rows(B[roll], aligned), _dev(sc), dev[2], _dev_rows(D[roll], aligned))
        assert torch.equal(_bits(moved.view(rows, k)), _bits(got.view(rows, k)[_dev(roll)]))


# ---- 6. knn_aggr(weight_grad=True) -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def knn_case(hg):
    torch.manual_seed(5)
    P = torch.randn(300, 6, device=DEV)
    idx, dist, mean = hg.ops.knn(P, 10, self_first=True, return_mean=True)
    hyperg = hg.HyperGraph.from_knn(P, 10, DEV)
    assert torch.equal(hyperg.H_T_colind.reshape(300, 10), idx)
    return dict(P=P, idx=idx, dist=dist, mean=mean, w=hg.ops.knn_incidence_weights(dist, mean), hyperg=hyperg)


@pytest.mark.parametrize("F", [20, 64])
def test_weight_gradient(hg, knn_case, F):
    c = knn_case
    idx, hyperg = c["idx"], c["hyperg"]
    rng = np.random.default_rng(60 + F)
    Xn = (rng.standard_normal((300, F)) * 0.3).astype(np.float32)
    Gn = (rng.standard_normal((300, F)) * 0.3).astype(np.float32)
    degE, degV = _np(hyperg.degE), _np(hyperg.degV)
    X0 = _dev(Xn).requires_grad_(True)
    Y0 = hg.ops.knn_aggr(idx, X0, c["w"], hyperg.degE, hyperg.degV)
    (dX0,) = torch.autograd.grad(Y0, X0, _dev(Gn))
    for shape in ((3000,), (300, 10)):
        X = _dev(Xn).requires_grad_(True)
        w = c["w"].clone().reshape(shape).requires_grad_(True)
        Y = hg.ops.knn_aggr(idx, X, w, hyperg.degE, hyperg.degV, weight_grad=True)
        saved = Y.grad_fn.saved_tensors
        assert all(t is None or t.numel() <= 3000 or t.data_ptr() == X.data_ptr() for t in saved)
        dX, dw = torch.autograd.grad(Y, (X, w), _dev(Gn))
        assert dw.shape == w.shape
        assert torch.equal(_bits(Y), _bits(Y0)) and torch.equal(_bits(dX), _bits(dX0))
        ref = gr.dw64(_np(idx), Xn, Gn, _np(c["w"]), degE, degV)
        _assert_close(dw.reshape(-1), ref, "dw, F = %d" % F)
    # the planned operator on HyperGraph.from_knn of the same points: its two weight gradients add up to dw
    X2 = _dev(Xn)
    a, b = c["w"].clone().requires_grad_(True), c["w"].clone().requires_grad_(True)
    with hg.ops.options(backward="adjoint"):
        Y2 = hg.ops.HGNNAggrIncidence(hyperg, X2, a, b, hyperg.degE, hyperg.degV, torch.ones(300, device=DEV))
        da, db = torch.autograd.grad(Y2, (a, b), _dev(Gn))
    _assert_close(dw.reshape(-1), _np(da).astype(np.float64) + _np(db).astype(np.float64), "dw against incidence_aggr")
    # a weight that asks for no gradient, and no_grad, take the default path
    Y3 = hg.ops.knn_aggr(idx, X0, c["w"], hyperg.degE, hyperg.degV, weight_grad=True)
    assert torch.equal(_bits(Y3), _bits(Y0)) and type(Y3.grad_fn).__name__ == type(Y0.grad_fn).__name__


def test_weight_gradient_over_hubs_and_ignored_entries(hg):
    from hypergef_amd import knn_graph as kg
    t = tr.hub_operator_case(5, kg.table_seq_max())
    idx, n = t["idx"].copy(), t["n"]
    idx[7, 1], idx[8, 0] = -1, n
    # dw is linear in the output gradient: G is scaled so that |ref| <= 1, where the rule is absolute
    G = (t["G"] / max(1.0, np.abs(gr.dw64(idx, t["X"], t["G"], t["w"], t["degE"], t["degV"])).max())).astype(np.float32)
    X = _dev(t["X"]).requires_grad_(True)
    w = _dev(t["w"]).requires_grad_(True)
    Y = hg.ops.knn_aggr(_dev(idx), X, w, _dev(t["degE"]), _dev(t["degV"]), weight_grad=True)
    dX, dw = torch.autograd.grad(Y, (X, w), _dev(G))
    _assert_close(dX, tr.aggr_grad(idx, G, t["w"], t["degE"], t["degV"]), "dX over hubs")
    _assert_close(dw, gr.dw64(idx, t["X"], G, t["w"], t["degE"], t["degV"]), "dw over hubs")
    assert _np(dw)[7 * 2 + 1] == 0 and _np(dw)[8 * 2] == 0


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------------

def _restated(Xn, Wn, idx, mean, degE, degV, m_prob, Gn):
    """sum(G * Y) of the probabilistic layer over a fixed table in float64 torch on the CPU, with autograd: (Y, dX, dW)."""
    X = torch.from_numpy(Xn.astype(np.float64)).requires_grad_(True)
    W = torch.from_numpy(Wn.astype(np.float64)).requires_grad_(True)
    idx = torch.from_numpy(idx.astype(np.int64))
    rows, k = idx.shape
    d2 = ((X[:, None, :] - X[idx]) ** 2).sum(-1)
    w = torch.exp(-d2 / (m_prob * torch.from_numpy(mean.astype(np.float64))[:, None]) ** 2)
    Z = X @ W.T
    Xe = torch.from_numpy(degE.astype(np.float64)).reshape(-1, 1) * (w[:, :, None] * Z[idx]).sum(1)
    Y = torch.zeros_like(Z).index_add(0, idx.reshape(-1), (w[:, :, None] * Xe[:, None, :]).reshape(rows * k, -1))
    Y = torch.from_numpy(degV.astype(np.float64)).reshape(-1, 1) * Y
    dX, dW = torch.autograd.grad(Y, (X, W), torch.from_numpy(Gn.astype(np.float64)))
    return Y.detach().numpy(), dX.numpy(), dW.numpy()


def test_end_to_end_against_float64_autograd(hg):
    N, F, k = 300, 20, 10
    rng = np.random.default_rng(7)
    Xn = rng.standard_normal((N, F)).astype(np.float32)
    Gn = (rng.standard_normal((N, F)) * 0.3).astype(np.float32)
    torch.manual_seed(7)
    lin = hg.ops.Linear(F, F, bias=False).to(DEV)
    X = _dev(Xn).requires_grad_(True)
    g = hg.KnnHypergraph.build(X, k)
    Y = g.aggregate(lin(X), True, 1.0, X=X)
    dX, dW = torch.autograd.grad(Y, (X, lin.weight), _dev(Gn))
    Y64, dX64, dW64 = _restated(Xn, _np(lin.weight), _np(g.idx), _np(g.mean), _np(g.degE), _np(g.degV), 1.0, Gn)
    _assert_close(Y, Y64, "Y")
    _assert_close(dX, dX64, "dX")
    _assert_close(dW, dW64, "dLin")
    # without X the weights are constants: another dX, the same Y
    X1 = _dev(Xn).requires_grad_(True)
    Y1 = g.aggregate(lin(X1), True, 1.0)
    (dX1,) = torch.autograd.grad(Y1, X1, _dev(Gn))
    assert torch.equal(_bits(Y1), _bits(Y)) and not torch.equal(dX1, dX)
    assert torch.equal(_bits(g.weights(1.0, X=X.detach())), _bits(g.weights(1.0)))


# ---- 8. the layer ------------------------------------------------------------------------------------------------------------------

def test_layer(hg):
    torch.manual_seed(9)
    X = torch.randn(300, 12, device=DEV)
    G = torch.randn(300, 32, device=DEV)
    off = hg.DynamicHypergraphConv(12, 32, k=10, probabilistic=True, device_graph=True).to(DEV)
    on = hg.DynamicHypergraphConv(12, 32, k=10, probabilistic=True, device_graph=True, learn_distances=True).to(DEV)
    on.load_state_dict(off.state_dict())
    outs = []
    for layer in (off, on):
        x = X.clone().requires_grad_(True)
        y = layer(x)
        saved = [None if t is None else tuple(t.shape) for t in y.grad_fn.saved_tensors]  # before the backward frees them
        gx, gw = torch.autograd.grad(y, (x, layer.lin.weight), G)
        outs.append((y.detach(), gx, gw, saved))
    # the layer as it was: the library's own composition of the parent's forward, bit for bit, with its saved tensors
    x = X.clone().requires_grad_(True)
    g = hg.KnnHypergraph.build(x, 10)
    y = hg.ops.knn_aggr(g.idx, off.lin(x), hg.ops.knn_incidence_weights(g.dist, g.mean, 1.0), g.degE, g.degV,
                        transpose=(g.ptr_v, g.pos_v))
    assert outs[0][3] == [None if t is None else tuple(t.shape) for t in y.grad_fn.saved_tensors]
    assert type(y.grad_fn).__name__ == "_KnnAggrBackward"
    gx, gw = torch.autograd.grad(y, (x, off.lin.weight), G)
    assert torch.equal(_bits(outs[0][0]), _bits(y.detach())) and torch.equal(_bits(outs[0][1]), _bits(gx))
    assert torch.equal(_bits(outs[0][2]), _bits(gw))
    # learn_distances: the same output bits, another input gradient
    assert torch.equal(_bits(outs[1][0]), _bits(outs[0][0]))
    assert not torch.equal(outs[1][1], outs[0][1])
    # against float64 autograd over the same table; dX is linear in G, which is scaled so that |ref| <= 1
    args = (_np(X), _np(on.lin.weight), _np(on.hyperg.idx), _np(on.hyperg.mean), _np(on.hyperg.degE), _np(on.hyperg.degV), 1.0)
    Gs = (_np(G) / max(1.0, np.abs(_restated(*args, _np(G))[1]).max())).astype(np.float32)
    x = X.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(on(x), x, _dev(Gs))
    _assert_close(gx, _restated(*args, Gs)[1], "dX of the learning layer")


def test_layer_capture_searches_again_on_replay(hg):
    torch.manual_seed(13)
    layer = hg.DynamicHypergraphConv(16, 16, k=4, probabilistic=True, device_graph=True, learn_distances=True).to(DEV)
    Xa, Xb = torch.randn(130, 16, device=DEV), torch.randn(130, 16, device=DEV)
    G = torch.randn(130, 16, device=DEV)

    def eager(X):
        layer.lin.weight.grad = None
        x = X.clone().requires_grad_(True)
        y = layer(x)
        y.backward(G)
        return y.detach().clone(), layer.lin.weight.grad.detach().clone(), x.grad.clone(), layer.hyperg.idx.clone()

    ya, ga, xa, ia = eager(Xa)
    yb, gb, xb, ib = eager(Xb)
    assert not torch.equal(ia, ib)
    static_x = Xa.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            layer.lin.weight.grad = None
            static_x.grad = None
            layer(static_x).backward(G)
    torch.cuda.current_stream().wait_stream(side)
    layer.lin.weight.grad = None
    static_x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = layer(static_x)
        static_y.backward(G)
    static_idx = layer.hyperg.idx
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_y, ya) and torch.equal(layer.lin.weight.grad, ga) and torch.equal(static_idx, ia)
    assert torch.equal(static_x.grad, xa)
    with torch.no_grad():
        static_x.copy_(Xb)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_idx, ib)
    assert torch.equal(static_y, yb) and torch.equal(layer.lin.weight.grad, gb) and torch.equal(static_x.grad, xb)


# ---- 9. large offsets ----------------------------------------------------------------------------------------------------------------

def test_rows_past_two_to_the_31_elements(hg):
    """A source of just over 2^31 elements and a tiny table naming its last rows: an offset formed in 32 bits reads zeros
    near the start instead.  dist, the hyperedge difference gather and table_dot, each bit for bit against its model."""
    from hypergef_amd import knn_graph as kg
    F = 512
    n = 2 ** 31 // F + 8
    assert n * F > 2 ** 31
    rng = np.random.default_rng(31)
    last = rng.standard_normal((8, F)).astype(np.float32)
    big = torch.zeros((n, F), dtype=torch.float32, device=DEV)
    big[n - 8:] = _dev(last)
    idx = np.array([[n - 1, n - 3, n - 8], [n - 2, n - 1, n - 5], [n - 8, n - 7, n - 6], [n - 4, n - 4, n - 1]], np.int32)
    small = (idx - (n - 8)).astype(np.int32)  # the same table over the last eight rows alone
    Q = rng.standard_normal((4, F)).astype(np.float32)
    w = rng.standard_normal(12).astype(np.float32)
    try:
        got = hg.ops.knn_dist(_dev(idx), big, queries=_dev(Q))
        assert np.array_equal(_np(got), gr.dist(small, last, Q))
        got = kg.table_gather(_dev(idx), big, _dev(w), ctr=_dev(Q))
        assert np.array_equal(_np(got), gr.gather_diff(small, Q, last, w))
        got = kg.table_dot(_dev(idx), big, _dev(Q))
        assert np.array_equal(_np(got), gr.table_dot(small, last, Q))
    finally:
        del big
        torch.cuda.empty_cache()
