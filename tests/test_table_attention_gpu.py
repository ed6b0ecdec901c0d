"""Fused attention aggregation over a neighbour table on the GPU (hg_table_attention_*, ops.knn_attention_aggr,
DynamicHypergraphConv(fused_attention=True)).  The contract is exact: the output and every gradient have the bits of
ops.knn_aggr on ops.knn_softmax's alpha, so that pair is the reference of the bits and float64 (the softmax and the two weighted
sums written out in torch) that of the values, at _assert_close's bounds -- test_table_heads_gpu.py's for the same pair.

Tables: test_table_softmax_gpu.py's [77, k] over 53 vertices (entries -1, n and beyond, a row with none, vertices no row
names), k in (1, 5, 64), and _table_ref.hub_table at the width: vertex rows either side of HG_TABLE_SEQ_MAX, so both groups run
the transposed gather's long-row phase and the vertex group the statistics' workgroup segments.  (F, H): a single head, the LDS
slab (Ch = 16), per-lane coefficients (Ch = 4), a lane that straddles heads (Ch = 6), 4-byte lanes, a second column pass."""
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
SHAPES = [(32, 1), (64, 4), (16, 4), (24, 4), (6, 3), (320, 4)]
MODES = {"both": (True, True), "node": (True, False), "edge": (False, True)}


def _case(which, F, H):
    """The table, float32 inputs on the device and the kNN hypergraph's scales.  The output gradient is scaled by F^-1/2: dalpha
    is a dot product over the columns, and _assert_close's absolute floor of 1e-6 is one for sums of magnitude 1."""
    if which == "hub":
        t = tr.hub_table(F)
        idx, n = t["idx"], t["n"]
    else:
        idx, n = _table(which)
    rows, k = idx.shape
    rng = np.random.default_rng(F + H)
    deg = np.bincount(idx[(idx >= 0) & (idx < n)], minlength=n)
    c = dict(idx=_dev(idx), n=n, X=_dev(rng.standard_normal((n, F)).astype(np.float32)),
             G=_dev((rng.standard_normal((n, F)) / np.sqrt(F)).astype(np.float32)),
             sv=_dev(rng.standard_normal((n, H) if H > 1 else n).astype(np.float32)),
             se=_dev(rng.standard_normal((rows, H) if H > 1 else rows).astype(np.float32)),
             degE=_dev(np.full(rows, 1.0 / k, np.float32)),
             degV=_dev(np.where(deg > 0, np.maximum(deg, 1) ** -0.5, 1.0).astype(np.float32)))
    return c


def _run(f, c, sv, se):
    """(Y, dX, the gradients of the scores given) of one path."""
    ins = [t.clone().requires_grad_(True) for t in (c["X"], sv, se) if t is not None]
    X, sv, se = ins[0], ins[1] if sv is not None else None, ins[-1] if se is not None else None
    Y = f(X, sv, se)
    return (Y.detach(), *torch.autograd.grad(Y, ins, c["G"]))


def _float64(c, sv, se, group, slope, H):
    """The same in float64 on the CPU: the softmax per segment and the two weighted sums, written out."""
    idx = c["idx"].long().cpu()
    rows, k = idx.shape
    n, F = c["X"].shape
    valid = (idx >= 0) & (idx < n)
    j = torch.where(valid, idx, 0)
    ins = [t.double().cpu().requires_grad_(True) for t in (c["X"], sv, se) if t is not None]
    X, degE, degV, G = ins[0], c["degE"].double().cpu(), c["degV"].double().cpu(), c["G"].double().cpu()
    raw = torch.zeros(rows, k, H, dtype=torch.float64)
    if se is not None:
        raw = raw + ins[-1].view(rows, 1, H)
    if sv is not None:
        raw = raw + ins[1].view(n, H)[j]
    ex = torch.exp(torch.where(raw > 0, raw, slope * raw)) * valid[..., None]
    seg = j if group == "vertex" else torch.arange(rows)[:, None].expand(rows, k)
    total = torch.zeros(n if group == "vertex" else rows, H, dtype=torch.float64).index_add(0, seg.reshape(-1), ex.view(-1, H))
    alpha = (ex / total[seg].clamp(min=1e-300))[..., None]  # [rows, k, H, 1]
    Xe = degE.view(rows, 1, 1) * (alpha * X.view(n, H, F // H)[j]).sum(1)
    Y = degV.view(n, 1, 1) * torch.zeros(n, H, F // H, dtype=torch.float64).index_add(0, j.reshape(-1),
                                                                                    (alpha * Xe[:, None]).view(rows * k, H, -1))
    Y = Y.view(n, F)
    return [t.detach().numpy() for t in (Y, *torch.autograd.grad(Y, ins, G))]


@pytest.mark.parametrize("group", ["hyperedge", "vertex"])
@pytest.mark.parametrize("F,H", SHAPES)
@pytest.mark.parametrize("which", [1, 5, 64, "hub"])
def test_fused_is_the_two_calls_and_float64(hg, which, F, H, group):
    c = _case(which, F, H)
    idx, n = c["idx"], c["n"]
    tp = hg.ops.knn_transpose(idx, n)
    if which == "hub":
        assert int((tp[0][1:] - tp[0][:-1]).max()) > hg.knn_graph.table_seq_max()

    def fused(X, sv, se):
        return hg.ops.knn_attention_aggr(idx, X, sv, se, group, 0.2, c["degE"], c["degV"], transpose=tp, heads=H)

    def two(X, sv, se):
        alpha = hg.ops.knn_softmax(idx, sv, se, group, 0.2, transpose=tp, num_nodes=n, heads=H)
        return hg.ops.knn_aggr(idx, X, alpha, c["degE"], c["degV"], transpose=tp, weight_grad=True)

    for mode, (node, edge) in MODES.items():
        sv, se = c["sv"] if node else None, c["se"] if edge else None
        got, want = _run(fused, c, sv, se), _run(two, c, sv, se)
        names = ["Y", "dX"] + ["d node_score"] * node + ["d edge_score"] * edge
        for name, a, b in zip(names, got, want):
            assert torch.equal(_bits(a), _bits(b)), (mode, name)
        X = c["X"].clone().requires_grad_(True)  # dX alone: the backward of the two fused gathers
        assert torch.equal(_bits(torch.autograd.grad(fused(X, sv, se), X, c["G"])[0]), _bits(want[1])), (mode, "dX alone")
        for name, a, r in zip(names, got, _float64(c, sv, se, group, 0.2, H)):
            _assert_close(a.cpu().numpy().reshape(r.shape), r, "%s, %s" % (mode, name))


@pytest.mark.parametrize("group", ["hyperedge", "vertex"])
@pytest.mark.parametrize("which,H", [(5, 1), (5, 4), ("hub", 4), ("hub", 3)])
def test_statistics_reproduce_alpha(hg, which, H, group):
    """alpha[:, s, h] = the fused hop-1 gather of rows of ones over the one-column table idx[:, s] with the full table's
    statistics: 0 + 1 * alpha(p, h), so the stored pair and the formula give knn_softmax's bits."""
    kg = hg.knn_graph
    c = _case(which, 8 * H, H)
    idx, n, sv, se = c["idx"], c["n"], c["sv"], c["se"]
    rows, k = idx.shape
    ptr_v, pos_v = hg.ops.knn_transpose(idx, n)
    alpha = hg.ops.knn_softmax(idx, sv, se, group, 0.2, transpose=(ptr_v, pos_v), num_nodes=n, heads=H).view(rows, k, H)
    m, inv = kg.table_attention_stats(idx, n, group, sv, se, 0.2, ptr_v, pos_v, H)
    assert tuple(m.shape) == tuple(inv.shape) == (rows if group == "hyperedge" else n, H)
    ones = torch.ones(n, 8 * H, device=DEV)
    for s in range(k):
        col = idx[:, s:s + 1].contiguous()
        got = kg.table_attention_gather(col, None, None, n, ones, group, sv, se, 0.2, m, inv, heads=H)
        assert torch.equal(_bits(got.view(rows, H, 8)), _bits(alpha[:, s, :, None].expand(rows, H, 8))), s


def test_no_coefficient_array_is_saved(hg):
    c = _case(5, 64, 4)
    idx = c["idx"]
    count = idx.numel() * 4

    def saved(f):
        sizes = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: sizes.append(t.numel()) or t, lambda t: t):
            f(c["X"].clone().requires_grad_(True), c["sv"].clone().requires_grad_(True), c["se"].clone().requires_grad_(True))
        return sizes

    assert count not in saved(lambda X, sv, se: hg.ops.knn_attention_aggr(idx, X, sv, se, heads=4))
    assert count in saved(lambda X, sv, se: hg.ops.knn_aggr(idx, X, hg.ops.knn_softmax(idx, sv, se, num_nodes=c["n"], heads=4),
                                                            weight_grad=True))


@pytest.mark.parametrize("group", ["hyperedge", "vertex"])
def test_layer_flag_keeps_the_bits(hg, group):
    torch.manual_seed(26)
    X, G = torch.randn(60, 12, device=DEV), torch.randn(60, 16, device=DEV)
    steps = []
    for flag in (False, True):
        torch.manual_seed(27)
        layer = hg.DynamicHypergraphConv(12, 8, k=5, device_graph=True, attention=group, heads=2, fused_attention=flag).to(DEV)
        x = X.clone().requires_grad_(True)
        y = layer(x)
        steps.append((y.detach(), *torch.autograd.grad(y, [x, *layer.parameters()], G)))
    assert len(steps[0]) == 5 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*steps))
