"""The attention softmax over a neighbour table on the GPU (hg_table_softmax_f32 / _bwd_f32, hg_table_sum_f32, ops.knn_softmax,
DynamicHypergraphConv(attention=)), both groups, against a float64 evaluation of the same float32 scores.  U = 2^-24.

Tables: [77, k] over 53 vertices, k in (1, 3, 8, 9, 33, 64) -- the lane-group widths 1, 4, 8, 16 and 64 with and without padding
lanes -- about 15 % of the entries out of range, row 5 out of range throughout, row 6 with one candidate, vertex 51 named once
and vertex 52 never; for the vertex group also _table_ref.hub_table(1), whose vertex rows have 0, 128, 129, 130, 515 and 1000
entries: either side of HG_TABLE_SEQ_MAX, and more than one and more than three sweeps of the 256 threads.

The bounds are those derived in tests/test_attention_gpu.py's header: |alpha - ref| <= c ref with c = (L + 16 + 16 Smax) U, and
for the gradients (2 c + (L + D + 8) U) max(mass, TINY); L the longest segment, D the longest segment of the reducing side."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _table_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
TINY = 1e-30
KS = (1, 3, 8, 9, 33, 64)
MODES = ("node", "edge", "both", "entry")
CELLS = [("hyperedge", k) for k in KS] + [("vertex", k) for k in KS] + [("vertex", "hub")]


def _table(which):
    if which == "hub":
        t = tr.hub_table(1)
        return t["idx"], t["n"]
    rng = np.random.default_rng(which)
    idx = rng.integers(0, 51, (77, which)).astype(np.int32)
    bad = rng.random(idx.shape) < 0.15
    idx[bad] = rng.choice(np.asarray([-1, 53, 2 ** 30, -(2 ** 31)]), int(bad.sum()))
    idx[5] = 53
    idx[6] = -1
    idx[6, 0] = 7
    idx[8, -1] = 51
    return idx, 53


def _scores(idx, n, mode, scale=1.0, seed=0):
    rng = np.random.default_rng(seed)
    sv, se, en = ((scale * rng.standard_normal(s)).astype(np.float32) for s in (n, idx.shape[0], idx.shape))
    return (sv if mode != "edge" else None, se if mode != "node" else None, en if mode == "entry" else None)


def _dev(a, grad=False):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def _ref(idx, n, group, sv, se, en, slope, dalpha=None):
    """float64: alpha, and with dalpha the gradients (ds, d node_score, d edge_score) and their masses; L and D per side."""
    rows, k = idx.shape
    flat = idx.reshape(-1).astype(np.int64)
    valid = (flat >= 0) & (flat < n)
    v, e = np.where(valid, flat, 0), np.repeat(np.arange(rows), k)
    raw = np.zeros(rows * k)
    for t in ((None if sv is None else sv[v]), (None if se is None else se[e]), (None if en is None else en.reshape(-1))):
        raw = raw if t is None else raw + t.astype(np.float64)
    seg, nseg = (v, n) if group == "vertex" else (e, rows)
    x = np.where(raw > 0, raw, slope * raw)
    m = np.full(nseg, -np.inf)
    np.maximum.at(m, seg[valid], x[valid])
    ex = np.where(valid, np.exp(x - np.where(valid, m[seg], 0.0)), 0.0)
    alpha = np.where(valid, ex / np.maximum(np.bincount(seg, ex, nseg), TINY)[seg], 0.0)
    longest = {"vertex": int(np.bincount(v[valid], minlength=n).max()), "hyperedge": k}
    out = dict(alpha=alpha.reshape(rows, k), valid=valid.reshape(rows, k), seg=seg, L=longest[group], longest=longest,
               c=(longest[group] + 16 + 16 * np.abs(raw[valid]).max()) * U)
    if dalpha is not None:
        d = dalpha.reshape(-1).astype(np.float64)
        ds = alpha * (d - np.bincount(seg, alpha * d, nseg)[seg]) * np.where(raw > 0, 1.0, slope)
        mass = alpha * (np.abs(d) + np.bincount(seg, alpha * np.abs(d), nseg)[seg]) * max(1.0, slope)
        out.update(grads=(np.bincount(v, ds * valid, n), np.bincount(e, ds, rows), ds.reshape(rows, k)),
                   mass=(np.bincount(v, mass * valid, n), np.bincount(e, mass, rows), mass.reshape(rows, k)),
                   D=(longest["vertex"], k, 0))
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("group,which", CELLS)
def test_alpha_exact_facts_and_float64(hg, group, which):
    idx, n = _table(which)
    didx = _dev(idx)
    tp = hg.ops.knn_transpose(didx, n)
    for mode in MODES:
        for slope in (0.2, 1.0):
            sv, se, en = _scores(idx, n, mode)
            args = (didx, _dev(sv), _dev(se), group, slope, _dev(en))
            got = hg.ops.knn_softmax(*args, transpose=tp, num_nodes=n)
            assert torch.equal(_bits(got), _bits(hg.ops.knn_softmax(*args, num_nodes=n))), (mode, slope)
            r = _ref(idx, n, group, sv, se, en, slope)
            a = got.cpu().numpy()
            assert not _bits(got).cpu().numpy()[~r["valid"]].any(), "an out-of-range position is not +0.0"
            count = np.bincount(r["seg"][r["valid"].reshape(-1)], minlength=max(n, idx.shape[0]))
            single = r["valid"].reshape(-1) & (count[r["seg"]] == 1)
            assert which == "hub" or single.any()
            assert (a.reshape(-1)[single] == 1.0).all(), "a one-candidate segment is not exactly 1.0"
            err, bound = np.abs(a - r["alpha"]), r["c"] * r["alpha"]
            print("%s %s %s slope %g: worst |alpha - ref| / bound = %.3g" % (group, which, mode, slope, (err / np.maximum(bound, TINY)).max()))
            assert (err <= bound).all(), (mode, slope, float((err - bound).max()))
    sv, se, en = _scores(idx, n, "entry", scale=1e4)
    big = hg.ops.knn_softmax(didx, _dev(sv), _dev(se), group, 0.2, _dev(en), transpose=tp)
    assert torch.isfinite(big).all()


@pytest.mark.parametrize("group,which", [("hyperedge", 3), ("hyperedge", 9), ("vertex", 3), ("vertex", 9), ("vertex", "hub")])
def test_gradients_against_float64(hg, group, which):
    idx, n = _table(which)
    sv, se, en = _scores(idx, n, "entry", seed=1)
    dalpha = np.random.default_rng(2).standard_normal(idx.shape).astype(np.float32)
    r = _ref(idx, n, group, sv, se, en, 0.2, dalpha)
    ins = [_dev(t, grad=True) for t in (sv, se, en)]
    for attempt in range(2):
        alpha = hg.ops.knn_softmax(_dev(idx), ins[0], ins[1], group, 0.2, ins[2])
        grads = torch.autograd.grad(alpha, ins, _dev(dalpha))
        if attempt:
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, first))
        first = grads
    for name, got, ref, mass, D in zip(("d node_score", "d edge_score", "d entry_score"), grads, r["grads"], r["mass"], r["D"]):
        err = np.abs(got.cpu().numpy() - ref)
        bound = (2 * r["c"] + (r["L"] + D + 8) * U) * np.maximum(mass, TINY)
        print("%s %s %s: worst error / bound = %.3g" % (group, which, name, (err / bound).max()))
        assert (err <= bound).all(), (name, float((err / bound).max()))
    assert not _bits(grads[2]).cpu().numpy()[~r["valid"]].any(), "ds of an out-of-range position is not +0.0"


def _layer64(X, W, a_v, a_e, idx, group, slope, G):
    """The attention layer on the table idx [N, k] (all in range) in float64, dense: (Y, dX for the output gradient G)."""
    X = X.double().cpu().requires_grad_(True)
    W, a_v, a_e, G, idx = W.double().cpu(), a_v.double().cpu(), a_e.double().cpu(), G.double().cpu(), idx.long().cpu()
    N, k = idx.shape
    Z = X @ W.t()
    raw = (Z @ a_v)[idx] + (Z @ a_e)[idx].mean(1, keepdim=True)
    x = torch.where(raw > 0, raw, slope * raw)
    if group == "hyperedge":
        alpha = torch.softmax(x, 1)
    else:
        ex = torch.exp(x - x.max())
        alpha = ex / torch.zeros(N, dtype=torch.float64).index_add(0, idx.reshape(-1), ex.reshape(-1))[idx]
    Ht = torch.zeros(N, N, dtype=torch.float64).index_put((torch.arange(N)[:, None].expand(N, k), idx), alpha, accumulate=True)
    deg = torch.bincount(idx.reshape(-1), minlength=N).double()
    degV = torch.where(deg > 0, deg.clamp(min=1).pow(-0.5), torch.ones_like(deg))[:, None]
    Y = degV * (Ht.t() @ ((Ht @ Z) / k))
    return Y.detach().numpy(), torch.autograd.grad(Y, X, G)[0].numpy()


@pytest.mark.parametrize("group", ["hyperedge", "vertex"])
def test_layer_against_the_planned_layer_and_capture(hg, group):
    torch.manual_seed(23)
    X = torch.randn(300, 12, device=DEV)
    G = torch.randn(300, 32, device=DEV)
    layer = hg.DynamicHypergraphConv(12, 32, k=10, device_graph=True, attention=group).to(DEV)
    hyperg = hg.HyperGraph.from_knn(X, 10, DEV)
    planned = hg.HypergraphAttnConv(hyperg, 12, 32, group=group).to(DEV)
    planned.load_state_dict(dict(layer.state_dict(), bias=torch.zeros(32)))

    def run(net):
        x = X.clone().requires_grad_(True)
        y = net(x)
        return y.detach().clone(), torch.autograd.grad(y, x, G)[0]

    got = run(layer)
    with hg.ops.options(backward="adjoint"):
        plan = run(planned)
    assert torch.equal(layer.hyperg.idx.reshape(-1), hyperg.H_T_colind)
    ref = _layer64(X, layer.lin.weight.detach(), layer.a_v.detach(), layer.a_e.detach(), layer.hyperg.idx, group, 0.2, G)
    for what, a, b, r in zip(("Y", "dX"), got, plan, ref):
        err_plan, err = np.abs(b.cpu().numpy() - r).max(), np.abs(a.cpu().numpy() - r)
        print("%s %s: planned layer's error %.3g, table layer's %.3g" % (group, what, err_plan, err.max()))
        assert (err <= np.maximum(4 * err_plan, 1e-5 * np.maximum(1.0, np.abs(r)))).all(), what
    # capture: a forward under torch.cuda.graph replays to the eager call's bits
    static_x = X.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            layer(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        static_y = layer(static_x)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(static_y), _bits(got[0]))
