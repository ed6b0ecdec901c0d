"""Several heads over a neighbour table on the GPU (hg_table_*_heads_f32, ops.knn_softmax(heads=), ops.knn_aggr(weight [.., H]),
DynamicHypergraphConv(heads=)).  The contract is exact: head h of every result is, bit for bit, the single-head call on
column h / on head h's columns, so the single-head call is the reference of the bits, and float64 (_table_ref.aggr,
_table_grad_ref.dw64, the dense layer of test_table_softmax_gpu.py) that of the values, at the existing bounds.

Tables: test_table_softmax_gpu.py's [77, k] over 53 vertices (about 15 % of the entries out of range, a row with none), k in
(1, 3, 9, 64); for the vertex side and hop 1 _table_ref.hub_table / hub_operator_case: vertex rows either side of
HG_TABLE_SEQ_MAX and several sweeps of the workgroup.  Heads (2, 3, 4, 8): a scalar slab, no power of two, one 16-byte slab,
two.  (H, Ch) of the aggregation: scalar lanes, a lane that would straddle heads, 16-byte lanes, a second column pass."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _table_grad_ref as tg  # noqa: E402
import _table_ref as tr  # noqa: E402
from test_table_gpu import _assert_close  # noqa: E402
from test_table_softmax_gpu import _bits, _dev, _layer64, _table  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = (1, 3, 9, 64)
HEADS = (2, 3, 4, 8)
MODES = {"node": (0,), "edge": (1,), "both": (0, 1), "entry": (0, 1, 2)}
CELLS = [("hyperedge", k) for k in KS] + [("vertex", k) for k in KS] + [("vertex", "hub")]


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("group,which", CELLS)
def test_softmax_head_is_the_single_head_call(hg, group, which, H):
    idx, n = _table(which)
    rows, k = idx.shape
    didx = _dev(idx)
    tp = hg.ops.knn_transpose(didx, n)
    valid = torch.from_numpy((idx >= 0) & (idx < n)).to(DEV)
    rng = np.random.default_rng(H)
    full = [_dev(rng.standard_normal(s).astype(np.float32)) for s in ((n, H), (rows, H), (rows, k, H))]
    dalpha = _dev(rng.standard_normal((rows, k, H)).astype(np.float32))  # signed

    def call(scores, heads, d):
        ins = [None if s is None else s.clone().requires_grad_(True) for s in scores]
        alpha = hg.ops.knn_softmax(didx, ins[0], ins[1], group, 0.2, ins[2], transpose=tp, num_nodes=n, heads=heads)
        return alpha.detach(), torch.autograd.grad(alpha, [t for t in ins if t is not None], d)

    for mode, given in MODES.items():
        scores = [s if i in given else None for i, s in enumerate(full)]
        alpha, grads = call(scores, H, dalpha)
        assert tuple(alpha.shape) == (rows, k, H)
        assert not _bits(alpha)[~valid].any(), "%s: an out-of-range position is not +0.0 in every head" % mode
        for h in range(H):
            a1, g1 = call([None if s is None else s[..., h].contiguous() for s in scores], 1, dalpha[..., h].contiguous())
            assert torch.equal(_bits(alpha[..., h]), _bits(a1)), (mode, h)
            for name, got, want in zip(given, grads, g1):
                assert torch.equal(_bits(got[..., h]), _bits(want)), (mode, h, "gradient of score %d" % name)


def _aggr_case(which, F):
    if which == "hub":
        t = tr.hub_operator_case(F)
        return {key: t[key] for key in ("idx", "n", "X", "G", "degE", "degV")}
    idx, n = _table(9)
    rng = np.random.default_rng(F)
    # the kNN hypergraph's scales, as hub_operator_case has them: _assert_close's absolute floor of 1e-6 is one for sums of
    # magnitude 1, which degE = 1 / k and degV = in-degree^-1/2 give and scales around 1 (sums of a hundred terms) do not
    deg = np.bincount(idx[(idx >= 0) & (idx < n)], minlength=n).astype(np.float64)
    return dict(idx=idx, n=n, X=rng.standard_normal((n, F)).astype(np.float32), G=rng.standard_normal((n, F)).astype(np.float32),
                degE=np.full(idx.shape[0], 1.0 / idx.shape[1], np.float32),
                degV=np.where(deg > 0, np.maximum(deg, 1) ** -0.5, 1.0).astype(np.float32))


@pytest.mark.parametrize("which", ["irregular", "hub"])
@pytest.mark.parametrize("H,Ch", [(2, 1), (3, 5), (4, 4), (8, 20), (4, 68)])
def test_aggregation_head_is_the_single_head_call(hg, H, Ch, which):
    F = H * Ch
    c = _aggr_case(which, F)
    idx, n = c["idx"], c["n"]
    w = (np.random.default_rng(H * Ch).random((idx.size, H)) + 0.5).astype(np.float32)
    didx, X, G, degE, degV, wd = (_dev(a) for a in (idx, c["X"], c["G"], c["degE"], c["degV"], w))
    tp = hg.ops.knn_transpose(didx, n)

    def call(x, weight, g):  # the heads are the weight's last dimension
        x, weight = x.clone().requires_grad_(True), weight.clone().requires_grad_(True)
        Y = hg.ops.knn_aggr(didx, x, weight, degE, degV, transpose=tp, weight_grad=True)
        return (Y.detach(), *torch.autograd.grad(Y, (x, weight), g))

    Y, dX, dw = call(X, wd, G)
    assert tuple(Y.shape) == (n, F) and tuple(dw.shape) == (idx.size, H)
    for h in range(H):
        cols = slice(h * Ch, (h + 1) * Ch)
        wh = wd[:, h].contiguous()
        Y1, dX1, _ = call(X, wh, G)  # the full width with head h's weights: the same long-row pieces
        assert torch.equal(_bits(Y[:, cols]), _bits(Y1[:, cols])), ("Y", h)
        assert torch.equal(_bits(dX[:, cols]), _bits(dX1[:, cols])), ("dX", h)
        _, _, dw1 = call(X[:, cols].contiguous(), wh, G[:, cols].contiguous())
        assert torch.equal(_bits(dw[:, h]), _bits(dw1)), ("dw", h)
        xs, gs = c["X"][:, cols], c["G"][:, cols]
        _assert_close(Y[:, cols], tr.aggr(idx, xs, w[:, h], c["degE"], c["degV"]), "Y, head %d" % h)
        _assert_close(dX[:, cols], tr.aggr_grad(idx, gs, w[:, h], c["degE"], c["degV"]), "dX, head %d" % h)
        _assert_close(dw[:, h], tg.dw64(idx, xs, gs, w[:, h], c["degE"], c["degV"]), "dw, head %d" % h)


def _step(layer, X, G):
    x = X.clone().requires_grad_(True)
    y = layer(x)
    return (y.detach().clone(), *torch.autograd.grad(y, [x, *layer.parameters()], G))


@pytest.mark.parametrize("group", ["hyperedge", "vertex"])
@pytest.mark.parametrize("H,C,concat", [(2, 4, True), (3, 5, False), (4, 4, False), (8, 5, True)])
def test_layer_against_float64_the_planned_layer_and_capture(hg, H, C, concat, group):
    torch.manual_seed(24)
    N, Fin, K = 60, 12, 5
    X = torch.randn(N, Fin, device=DEV)
    G = torch.randn(N, H * C if concat else C, device=DEV)
    layer = hg.DynamicHypergraphConv(Fin, C, k=K, device_graph=True, attention=group, heads=H, concat=concat).to(DEV)
    got = _step(layer, X, G)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, _step(layer, X, G))), "two calls differ"
    hyperg = hg.HyperGraph.from_knn(X, K, DEV)
    assert torch.equal(layer.hyperg.idx.reshape(-1), hyperg.H_T_colind)
    planned = hg.HypergraphAttnConv(hyperg, Fin, C, group=group, heads=H, concat=concat).to(DEV)
    planned.load_state_dict(dict(layer.state_dict(), bias=torch.zeros(G.shape[1])))
    with hg.ops.options(backward="adjoint"):
        plan = _step(planned, X, G)
    # float64, head by head: the heads share nothing but X, so Y is the heads' outputs side by side and dX their sum
    W, a_v, a_e = (t.detach() for t in (layer.lin.weight, layer.a_v, layer.a_e))
    per_head = [_layer64(X, W[h * C:(h + 1) * C], a_v[h * C:(h + 1) * C], a_e[h * C:(h + 1) * C], layer.hyperg.idx, group, 0.2,
                         G[:, h * C:(h + 1) * C] if concat else G / H) for h in range(H)]
    Ys, dXs = zip(*per_head)
    ref = (np.concatenate(Ys, 1) if concat else sum(Ys) / H, sum(dXs))
    for what, a, b, r in zip(("Y", "dX"), got, plan, ref):
        err_plan, err = np.abs(b.cpu().numpy() - r).max(), np.abs(a.cpu().numpy() - r)
        print("%s H=%d %s: planned layer's error %.3g, table layer's %.3g" % (group, H, what, err_plan, err.max()))
        assert (err <= np.maximum(4 * err_plan, 1e-5 * np.maximum(1.0, np.abs(r)))).all(), what
    # capture: the training step under torch.cuda.graph replays to the eager step's bits
    x = X.clone().requires_grad_(True)
    leaves = [x, *layer.parameters()]

    def step():
        for t in leaves:
            t.grad = None
        y = layer(x)
        y.backward(G)
        return y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = step()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, (y.detach(), *(t.grad for t in leaves))))


@pytest.mark.parametrize("group", ["hyperedge", "vertex"])
def test_one_head_is_the_layer_as_it_was(hg, group):
    torch.manual_seed(25)
    X, G = torch.randn(60, 12, device=DEV), torch.randn(60, 5, device=DEV)
    old = hg.DynamicHypergraphConv(12, 5, k=5, device_graph=True, attention=group).to(DEV)
    new = hg.DynamicHypergraphConv(12, 5, k=5, device_graph=True, attention=group, heads=1, concat=False).to(DEV)
    new.load_state_dict(old.state_dict())
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(_step(old, X, G), _step(new, X, G)))
