"""ops.knn on the device against tests/_knn_ref.py.

Exact class: inputs randint(-4, 5) as float32, so every d2 is an integer fp32 holds exactly (at most 64 F < 2^24) and ties
are everywhere: idx and dist must equal the reference, whose selection is np.lexsort((j, d2)).  Float class: randn inputs
against the float64 distances D with eps = (F + 3) 2^-23, the fp32 rounding bound of an F-term sum of squared differences,
doubled.  The kernel's query tile is 64 rows and its candidate tile 256 (hg_knn.h): the sizes straddle both.
cand_slices runs up to its limit of 32, where most slices own no candidate tile and the merge reads lists of unused slots.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _grad_ref as gr  # noqa: E402
import _incidence_ref as ir  # noqa: E402
import _knn_ref as kr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 300)
WIDTHS = (1, 3, 32, 33, 260)
U23 = 2.0 ** -23


def _ints(n, F, seed):
    return np.random.default_rng(seed).integers(-4, 5, (n, F)).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ks(n):
    return sorted({k for k in (1, 2, 10, 64, n if n <= 64 else 1) if k <= n})


def _assert_exact(got, want, what):
    idx, dist = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert idx.dtype == np.int32 and dist.dtype == np.float32, what
    assert np.array_equal(idx, want[0]), "%s: idx differs in %d rows" % (what, int((idx != want[0]).any(1).sum()))
    assert np.array_equal(dist.astype(np.float64), want[1]), what
    assert not np.signbit(dist).any(), what


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_exact_class(hg, n, F):
    X = _ints(n, F, 100 * n + F)
    D = kr.distances(X, X)
    x = _dev(X)
    for k in _ks(n):
        for self_first in (True, False):
            got = hg.ops.knn(x, k, self_first=self_first)
            _assert_exact(got, kr.knn(X, k, self_first=self_first, D=D), "n=%d F=%d k=%d self_first=%s" % (n, F, k, self_first))
    if n >= 2:  # the mean rides along: same lists, and sqrt of exact integers summed in fp32
        k = min(2, n)
        idx, dist, mean = hg.ops.knn(x, k, return_mean=True)
        want = kr.knn(X, k, D=D)
        _assert_exact((idx, dist), want, "n=%d F=%d with the mean" % (n, F))
        m = mean.cpu().numpy().astype(np.float64)
        assert (np.abs(m - want[2]) <= (n + F) * U23 * want[2]).all()


def test_duplicate_rows_and_self_first(hg):
    X = _ints(70, 5, 7)
    X[5] = X[2]
    X[69] = X[2]
    x = _dev(X)
    on, off = hg.ops.knn(x, 3), hg.ops.knn(x, 3, self_first=False)
    _assert_exact(on, kr.knn(X, 3, self_first=True), "duplicates, self_first")
    _assert_exact(off, kr.knn(X, 3, self_first=False), "duplicates, plain order")
    assert on[0][5].tolist() == [5, 2, 69] and off[0][5].tolist() == [2, 5, 69]
    assert on[0][69].tolist() == [69, 2, 5] and off[0][69].tolist() == [2, 5, 69]
    assert on[1][5].tolist() == [0.0, 0.0, 0.0]
    assert torch.equal(on[0][:, 0].cpu(), torch.arange(70, dtype=torch.int32))  # the centre is in its own hyperedge


def test_rows_one_float_off_a_16_byte_boundary(hg):
    n, F, k = 257, 33, 10
    X = _ints(n, F, 11)
    buf = torch.zeros(n * F + 1, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    x = buf[1:].view(n, F)
    x.copy_(torch.from_numpy(X))
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    _assert_exact(hg.ops.knn(x, k), kr.knn(X, k), "offset rows")
    q = torch.zeros(65 * F + 1, dtype=torch.float32, device=DEV)[1:].view(65, F)
    Q = _ints(65, F, 12)
    q.copy_(torch.from_numpy(Q))
    _assert_exact(hg.ops.knn(x, k, queries=q), kr.knn(X, k, queries=Q), "offset rows and queries")


@pytest.mark.parametrize("kind", ["integer", "randn"])
def test_split_invariance(hg, kind):
    n, F, k = 700, 33, 10
    X = _ints(n, F, 5) if kind == "integer" else np.random.default_rng(6).standard_normal((n, F)).astype(np.float32)
    x = _dev(X)
    base = None
    for cs in (1, 2, 3, 7, 0):
        idx, dist, mean = hg.ops.knn(x, k, return_mean=True, cand_slices=cs)
        again = hg.ops.knn(x, k, return_mean=True, cand_slices=cs)
        assert torch.equal(mean.view(torch.int32), again[2].view(torch.int32)), "mean differs between two calls, cand_slices=%d" % cs
        assert torch.equal(idx, again[0]) and torch.equal(dist.view(torch.int32), again[1].view(torch.int32))
        if base is None:
            base = (idx, dist, mean)
        assert torch.equal(idx, base[0]), "idx differs, cand_slices=%d" % cs
        assert torch.equal(dist.view(torch.int32), base[1].view(torch.int32)), "dist differs, cand_slices=%d" % cs
        assert torch.allclose(mean, base[2], rtol=(n + F) * U23, atol=0)
    want = kr.knn(X, k)
    if kind == "integer":
        _assert_exact(base, want, "split, integer")
    for kk in (33, 64):  # two list slots per lane, merged
        a = hg.ops.knn(x, kk, cand_slices=1)
        b = hg.ops.knn(x, kk, cand_slices=3, self_first=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        if kind == "integer":
            _assert_exact(a, kr.knn(X, kk), "k=%d" % kk)


@pytest.mark.parametrize("k", [1, 33, 64])
def test_merge_of_32_slices(hg, k):
    """cand_slices = 32 over 700 candidates: three candidate tiles, so 29 of the 32 slices -- slice 0 among them -- own no
    tile and hand the merge lists of unused slots only; at k = 64 the merge's LDS is the 64 KiB its launch allows for."""
    n, F = 700, 33
    X = _ints(n, F, 5)
    x = _dev(X)
    D = kr.distances(X, X)
    for self_first in (True, False):
        got = hg.ops.knn(x, k, self_first=self_first, cand_slices=32)
        _assert_exact(got, kr.knn(X, k, self_first=self_first, D=D), "32 slices, k=%d self_first=%s" % (k, self_first))
    r = _dev(np.random.default_rng(6).standard_normal((n, F)).astype(np.float32))
    for self_first in (True, False):
        one = hg.ops.knn(r, k, self_first=self_first, cand_slices=1)
        idx, dist, mean = hg.ops.knn(r, k, self_first=self_first, cand_slices=32, return_mean=True)
        assert torch.equal(idx, one[0]), "idx differs from one slice's, k=%d self_first=%s" % (k, self_first)
        assert torch.equal(dist.view(torch.int32), one[1].view(torch.int32)), "dist differs from one slice's, k=%d" % k
        again = hg.ops.knn(r, k, self_first=self_first, cand_slices=32, return_mean=True)
        for a, b in zip((idx, dist, mean), again):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two calls differ, k=%d self_first=%s" % (k, self_first)


def test_merge_of_32_slices_over_short_segments(hg):
    """Segments of 64, 1 and 235 rows under 32 slices at k = 1: a query tile has one candidate tile at the most, so all but one
    of its 32 lists are unused slots."""
    n, F, seg = 300, 33, [0, 64, 65, 300]
    X = _ints(n, F, 31)
    x = _dev(X)
    D = kr.distances(X, X)
    lo, hi = kr.candidate_ranges(n, n, seg)
    for self_first in (True, False):
        idx, dist, mean = hg.ops.knn(x, 1, segments=seg, self_first=self_first, return_mean=True, cand_slices=32)
        want = kr.knn(X, 1, segments=seg, self_first=self_first, D=D)
        _assert_exact((idx, dist), want, "32 slices, seg=%s self_first=%s" % (seg, self_first))
        i = idx.cpu().numpy()
        assert (i >= lo[:, None]).all() and (i < hi[:, None]).all(), "an index left its segment"
        m = mean.cpu().numpy().astype(np.float64)
        assert (np.abs(m - want[2]) <= (n + F) * U23 * np.maximum(want[2], 1e-300)).all()


@pytest.mark.parametrize("F", [3, 64, 260])
def test_float_class(hg, F):
    n, k = 300, 10
    X = np.random.default_rng(20 + F).standard_normal((n, F)).astype(np.float32)
    D = kr.distances(X, X)
    eps = (F + 3) * U23
    idx, dist, mean = hg.ops.knn(_dev(X), k, return_mean=True)
    idx, dist, mean = idx.cpu().numpy().astype(np.int64), dist.cpu().numpy().astype(np.float64), mean.cpu().numpy().astype(np.float64)
    rows = np.arange(n)[:, None]
    assert (idx >= 0).all() and (idx < n).all()
    assert all(len(set(r.tolist())) == k for r in idx), "a neighbour is listed twice"
    Dsel = D[rows, idx]
    err = np.abs(dist - Dsel)
    print("F=%d: max |dist - D| / (eps D) = %.3g" % (F, float((err / np.maximum(eps * Dsel, 1e-300)).max())))
    assert (err <= eps * Dsel).all()
    inside = np.zeros((n, n), bool)
    inside[rows, idx] = True
    worst_in = np.where(inside, D, -np.inf).max(1)
    best_out = np.where(inside, np.inf, D).min(1)
    assert (worst_in <= (1 + 2 * eps) * best_out).all()
    # ascending in the returned (dist, idx), after the row's own index
    assert (idx[:, 0] == np.arange(n)).all() and (dist[:, 0] == 0).all()
    d, j = dist[:, 1:], idx[:, 1:]
    assert ((d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & (j[:, 1:] > j[:, :-1]))).all()
    want_mean = np.sqrt(D).mean(1)
    rel = np.abs(mean - want_mean) / want_mean
    print("F=%d: max mean error / ((n + F) 2^-23) = %.3g" % (F, float(rel.max() / ((n + F) * U23))))
    assert (rel <= (n + F) * U23).all()


@pytest.mark.parametrize("seg,k", [([0, 5, 69, 70, 300], 1), ([0, 64, 65, 300], 1), ([0, 100, 300], 10)])
def test_segments(hg, seg, k):
    n, F = 300, 9
    X = _ints(n, F, 31)
    x = _dev(X)
    D = kr.distances(X, X)
    lo, hi = kr.candidate_ranges(n, n, seg)
    for self_first in (True, False):
        for cs in (0, 1, 3):
            idx, dist, mean = hg.ops.knn(x, k, segments=seg, self_first=self_first, return_mean=True, cand_slices=cs)
            want = kr.knn(X, k, segments=seg, self_first=self_first, D=D)
            _assert_exact((idx, dist), want, "seg=%s self_first=%s cand_slices=%d" % (seg, self_first, cs))
            i = idx.cpu().numpy()
            assert (i >= lo[:, None]).all() and (i < hi[:, None]).all(), "an index left its segment"
            m = mean.cpu().numpy().astype(np.float64)
            assert (np.abs(m - want[2]) <= (n + F) * U23 * np.maximum(want[2], 1e-300)).all()
    # the same through a tensor of offsets
    got = hg.ops.knn(x, k, segments=torch.tensor(seg))
    _assert_exact(got, kr.knn(X, k, segments=seg, D=D), "tensor offsets")


def test_queries_are_not_the_candidates(hg):
    nq, n, F = 65, 257, 33
    X, Q = _ints(n, F, 41), _ints(nq, F, 42)
    Q[:8] = X[100:108]  # queries that coincide with candidates: distance 0, no self rule
    D = kr.distances(Q, X)
    x, q = _dev(X), _dev(Q)
    for k in (1, 10, 64):
        for cs in (0, 1, 2):
            got = hg.ops.knn(x, k, queries=q, cand_slices=cs)
            _assert_exact(got, kr.knn(X, k, queries=Q, D=D), "queries k=%d cand_slices=%d" % (k, cs))
    idx, dist, mean = hg.ops.knn(x, 3, queries=q, return_mean=True)
    assert idx.shape == (nq, 3) and mean.shape == (nq,)
    want = np.sqrt(D).mean(1)
    assert (np.abs(mean.cpu().numpy() - want) <= (n + F) * U23 * want).all()


def test_grad_mode(hg):
    x = _dev(_ints(20, 4, 1)).requires_grad_(True)
    with pytest.raises(RuntimeError, match="no_grad"):
        hg.ops.knn(x, 3)
    with torch.no_grad():
        a = hg.ops.knn(x, 3)
    b = hg.ops.knn(x.detach(), 3)
    assert torch.equal(a[0], b[0]) and not a[1].requires_grad


@pytest.fixture(scope="module")
def knn_graph_case(hg):
    n, F, k = 300, 16, 5
    X = _ints(n, F, 51)
    hyperg = hg.HyperGraph.from_knn(torch.from_numpy(X), k, DEV)
    return X, k, hyperg, kr.knn(X, k)


def test_from_knn_layout(hg, knn_graph_case):
    X, k, hyperg, want = knn_graph_case
    n = X.shape[0]
    assert (hyperg.num_nodes, hyperg.num_edges, hyperg.nnz) == (n, n, n * k)
    assert np.array_equal(hyperg.H_T_csrptr.cpu().numpy(), np.arange(0, n * k + 1, k))
    assert np.array_equal(hyperg.H_T_colind.cpu().numpy(), want[0].reshape(-1))
    assert np.array_equal(hyperg.knn_dist.cpu().numpy().astype(np.float64), want[1])
    assert hyperg.knn_mean.shape == (n,) and hyperg.knn_weights().shape == (n * k,)
    assert torch.equal(hyperg.degE.cpu(), torch.full((n, 1), 1.0 / k).float())


def test_hgnnaggr_on_the_knn_hypergraph(hg, oracle, knn_graph_case):
    from hypergef_amd import knn_graph, synth
    X, k, hyperg, want = knn_graph_case
    inc = knn_graph.incidence_from_knn(want[0])  # the CSR of the reference's table
    F = 32
    feat = synth.features_like_reference(inc.N, F, seed=0)
    W = torch.ones(inc.M, 1, device=DEV)
    y = hg.HGNNAggr(hyperg, torch.from_numpy(feat).to(DEV), hyperg.degE, hyperg.degV, W, "sum")
    H_ptr, H_ind = oracle.transpose_csr(inc.M, inc.N, inc.csrptr, inc.colind)
    degE, degV = oracle.degrees(inc.N, inc.M, inc.csrptr, inc.colind)
    ref = oracle.hgnn_check(inc.N, inc.M, F, H_ptr, H_ind, inc.csrptr, inc.colind, feat, degE, degV, np.ones(inc.M, np.float32))
    got = y.cpu().numpy()
    print("max |got - oracle| = %g" % float(np.abs(got - ref).max()))
    assert np.array_equal(got, ref)


def test_incidence_aggr_with_knn_weights(hg, knn_graph_case):
    from hypergef_amd import knn_graph
    X, k, hyperg, want = knn_graph_case
    inc = knn_graph.incidence_from_knn(want[0])
    F = 16
    feat = torch.from_numpy(np.random.default_rng(52).standard_normal((inc.N, F)).astype(np.float32))
    w = hyperg.knn_weights()
    assert bool(((w > 0) & (w <= 1)).all()) and bool((w.view(-1, k)[:, 0] == 1).all())  # the centre: exp(0)
    W = torch.ones(inc.M, 1, device=DEV)
    y = hg.HGNNAggrIncidence(hyperg, feat.to(DEV), w, w, hyperg.degE, hyperg.degV, W)
    graph = gr.Graph(inc, hyperg.degE, hyperg.degV, W)
    ins = {"x": feat, "v2e": w.cpu(), "e2v": w.cpu()}
    out, _, mass, _ = gr.evaluate(ir.fn, graph, ins, torch.zeros(inc.N, F), ())
    gr.assert_within(y, out, mass, gr.FP32_C, "incidence_aggr with knn weights")


@pytest.mark.parametrize("probabilistic", [False, True])
def test_dynamic_hypergraph_conv(hg, probabilistic):
    n, F_in, F_out, k = 300, 16, 8, 5
    X = _dev(np.random.default_rng(61).standard_normal((n, F_in)).astype(np.float32))
    grads, outs = [], []
    for _ in range(2):
        torch.manual_seed(3)
        layer = hg.DynamicHypergraphConv(F_in, F_out, k, probabilistic=probabilistic, segments=[0, 100, 300]).to(DEV)
        x = X.clone().requires_grad_(True)
        y = layer(x)
        assert y.shape == (n, F_out)
        y.square().sum().backward()
        g = layer.lin.weight.grad
        assert g is not None and bool(torch.isfinite(g).all()) and bool(g.abs().sum() > 0)
        assert x.grad is not None and bool(torch.isfinite(x.grad).all())
        grads.append(g.clone())
        outs.append(y.detach().clone())
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    ind = layer.hyperg.H_T_colind.view(n, k).cpu()
    assert bool((ind[:100] < 100).all()) and bool((ind[100:] >= 100).all())
