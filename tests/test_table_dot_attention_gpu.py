"""Dot-product attention over a neighbour table on the GPU (hg_table_dot_attention_f32 / _bwd_f32, ops.knn_dot_attention_aggr,
DynamicHypergraphConv(score="dot")) against the formulas of include/hg_aggr.h written out in torch float64 on the CPU, at
_assert_close: the project's bound for this composition of a softmax and two weighted sums (test_table_attention_gpu.py).

Tables: test_table_softmax_gpu.py's [77, k] over 53 vertices (entries -1, n and beyond, a row with no candidate), k = 1, under
one batch (5) and eight full batches (64), and _table_ref.hub_table at the width, whose long vertex rows drive hop 1 and the dX
gather.  (F, H): lane groups of 8, 4, 1 and 64 lanes at 16-byte lanes, a padded group (Ch = 80: 20 of 32 lanes), and 4-byte
lanes (Ch = 6 and Ch = 2).  The output gradient is scaled by F^-1/2: dalpha is a dot product over the columns, and the bound's
absolute floor of 1e-6 is one for sums of magnitude 1."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _table_ref as tr  # noqa: E402
from test_table_gpu import _assert_close  # noqa: E402
from test_table_softmax_gpu import _bits, _dev, _table  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(32, 1), (64, 4), (16, 4), (24, 4), (6, 3), (320, 4), (256, 1)]


def _case(which, F, H):
    if which == "hub":
        t = tr.hub_table(F)
        idx, n = t["idx"], t["n"]
    else:
        idx, n = _table(which)
    rows, k = idx.shape
    rng = np.random.default_rng(F + H)
    deg = np.bincount(idx[(idx >= 0) & (idx < n)], minlength=n)
    return dict(idx=_dev(idx), n=n, X=_dev(rng.standard_normal((n, F)).astype(np.float32)),
                Q=_dev(rng.standard_normal((rows, F)).astype(np.float32)),
                G=_dev((rng.standard_normal((n, F)) / np.sqrt(F)).astype(np.float32)),
                degE=_dev(np.full(rows, 1.0 / k, np.float32)),
                degV=_dev(np.where(deg > 0, np.maximum(deg, 1) ** -0.5, 1.0).astype(np.float32)))


def _float64(c, slope, H):
    """(Y, alpha, dX, dquery) in float64 on the CPU."""
    idx = c["idx"].long().cpu()
    rows, k = idx.shape
    n, F = c["X"].shape
    valid = (idx >= 0) & (idx < n)
    j = torch.where(valid, idx, 0)
    X, Q = (c[name].double().cpu().requires_grad_(True) for name in ("X", "Q"))
    degE, degV, G = (c[name].double().cpu() for name in ("degE", "degV", "G"))
    Xj = X.view(n, H, F // H)[j]                                                       # [rows, k, H, Ch]
    t = (F // H) ** -0.5 * (Q.view(rows, 1, H, F // H) * Xj).sum(-1)
    a = torch.where(t > 0, t, slope * t).masked_fill(~valid[..., None], -1e300)  # exp underflows to exactly 0 beside a candidate
    alpha = (torch.softmax(a, 1) * valid[..., None])[..., None]                  # a row with no candidate: all 0
    E = degE.view(rows, 1, 1) * (alpha * Xj).sum(1)
    Y = degV.view(n, 1, 1) * torch.zeros(n, H, F // H, dtype=torch.float64).index_add(
        0, j.reshape(-1), (alpha * E[:, None]).view(rows * k, H, -1))
    Y = Y.view(n, F)
    dX, dQ = torch.autograd.grad(Y, [X, Q], G)
    return [t.detach().numpy() for t in (Y, alpha.view(rows, k, H), dX, dQ)]


def _run(hg, c, slope, H, tp):
    X, Q = c["X"].clone().requires_grad_(True), c["Q"].clone().requires_grad_(True)
    Y, alpha = hg.ops.knn_dot_attention_aggr(c["idx"], X, Q, slope, None, c["degE"], c["degV"], transpose=tp, heads=H, return_alpha=True)
    assert not alpha.requires_grad
    return (Y.detach(), alpha, *torch.autograd.grad(Y, [X, Q], c["G"]))


@pytest.mark.parametrize("slope", [1.0, 0.2])
@pytest.mark.parametrize("F,H", SHAPES)
@pytest.mark.parametrize("which", [1, 5, 64, "hub"])
def test_operator_against_float64(hg, which, F, H, slope):
    c = _case(which, F, H)
    tp = hg.ops.knn_transpose(c["idx"], c["n"])
    got = _run(hg, c, slope, H, tp)
    for name, a, r in zip(("Y", "alpha", "dX", "dquery"), got, _float64(c, slope, H)):
        _assert_close(a.cpu().numpy().reshape(r.shape), r, name)
    for a, b in zip(got, _run(hg, c, slope, H, tp)):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("F,H", [(64, 4), (24, 4)])
@pytest.mark.parametrize("which", [5, "hub"])
def test_a_head_is_the_single_head_call(hg, which, F, H):
    """Hop 1 sums a vertex row per (vertex, head) in ascending order whatever its length, so Y holds on the hub tables too: the
    existing transposed heads gather, which cuts a long row by the call's F, would differ on hub_table(64)'s six hubs."""
    c = _case(which, F, H)
    Ch = F // H
    with torch.no_grad():
        Y, alpha = hg.ops.knn_dot_attention_aggr(c["idx"], c["X"], c["Q"], 0.2, None, c["degE"], c["degV"], heads=H, return_alpha=True)
        single = []
        for h in range(H):
            Xh, Qh = (c[name][:, h * Ch:(h + 1) * Ch].contiguous() for name in ("X", "Q"))
            assert Xh.data_ptr() % 16 == 0 and Qh.data_ptr() % 16 == 0  # equal alignment: equal c
            single.append(hg.ops.knn_dot_attention_aggr(c["idx"], Xh, Qh, 0.2, None, c["degE"], c["degV"], return_alpha=True))
        for h, (_, ah) in enumerate(single):
            assert torch.equal(_bits(alpha[..., h].contiguous()), _bits(ah)), h
        Ys = torch.cat([Yh for Yh, _ in single], 1)
        off = _bits(Y) != _bits(Ys)
        assert not off.any(), "Y: %d of %d elements differ, rows %s" % (int(off.sum()), off.numel(), off.any(1).nonzero().reshape(-1).tolist())


def _layers(hg, heads):
    torch.manual_seed(29)
    X = torch.randn(60, 12, device=DEV)
    layer = hg.DynamicHypergraphConv(12, 8, k=5, device_graph=True, attention="hyperedge", heads=heads, score="dot",
                                     negative_slope=0.2).to(DEV)
    return X, layer


@pytest.mark.parametrize("heads", [2, 1])
def test_layer_is_the_planned_dot_layer(hg, heads):
    X, layer = _layers(hg, heads)
    ref = hg.HypergraphAttnConv(hg.HyperGraph.from_knn(X, 5, DEV), 12, 8, group="hyperedge", heads=heads, score="dot",
                                negative_slope=0.2).to(DEV)
    with torch.no_grad():
        ref.lin.weight.copy_(layer.lin.weight)
        ref.lin_k.weight.copy_(layer.lin_k.weight)
    G = torch.randn(60, 8 * heads, device=DEV)
    steps = []
    for m in (layer, ref):
        x = X.clone().requires_grad_(True)
        y = m(x)
        steps.append((y, *torch.autograd.grad(y, [x, m.lin.weight, m.lin_k.weight], G)))
    for name, a, b in zip(("Y", "dX", "d lin", "d lin_k"), *steps):
        _assert_close(a.detach().cpu().numpy(), b.detach().double().cpu().numpy(), name)


def test_layer_step_is_captured(hg):
    X, layer = _layers(hg, 2)
    X2 = torch.randn(60, 12, device=DEV)
    params = list(layer.parameters())

    def step(x):
        return torch.autograd.grad(layer(x).square().sum(), params)

    static = X.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(static)
    static.copy_(X2)
    eager = step(X2)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out, eager))
