"""ops.knn(form="dot") on the device: idx and dist are form="difference"'s, bit for bit, on every input -- through the
shortlist and the certificate where the row is certified, through the exhaustive path where it is not (return_fallback says
which; tests/_knn_dot_ref.py says from the inputs alone which it must be).  The prefilter's tile is 128 query rows by 128
candidates, 32 columns per LDS chunk, two columns per MFMA; the rerank stages 64 rows by 64 columns.  Also: 32 slices over
33 candidate tiles (the workspace size says that 32 were taken), and norms that overflow or pass the bound's 1e37."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_dot_ref as dr  # noqa: E402
import _knn_ref as kr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U23 = 2.0 ** -23


def _ints(n, F, seed):
    return np.random.default_rng(seed).integers(-4, 5, (n, F)).astype(np.float32)


def _randn(n, F, seed):
    return np.random.default_rng(seed).standard_normal((n, F)).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want, what):
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32, what
    assert torch.equal(got[0], want[0]), "%s: idx differs in %d rows" % (what, int((got[0] != want[0]).any(1).sum()))
    assert torch.equal(got[1], want[1]), "%s: dist differs" % what
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), "%s: dist differs in a sign bit" % what


# every n, F and k of the list at least once, and the corners n = 1, k = n, F = 1
SHAPES = [(1, 1, 1), (1, 33, 1), (65, 1, 1), (65, 3, 10), (65, 64, 64), (65, 260, 65), (257, 33, 33), (257, 1028, 10),
          (300, 3, 64), (300, 260, 1), (300, 64, 33), (513, 64, 10), (513, 33, 64), (513, 3, 1), (33, 1028, 33), (10, 260, 10)]


@pytest.mark.parametrize("kind", ["integer", "randn"])
@pytest.mark.parametrize("n,F,k", SHAPES)
def test_bit_identity(hg, n, F, k, kind):
    k = min(k, n, 64)
    X = _ints(n, F, 1000 * n + F) if kind == "integer" else _randn(n, F, 1000 * n + F)
    x = _dev(X)
    for self_first in (True, False):
        want = hg.ops.knn(x, k, self_first=self_first, form="difference")
        got = hg.ops.knn(x, k, self_first=self_first, form="dot")
        _same(got, want, "n=%d F=%d k=%d %s self_first=%s" % (n, F, k, kind, self_first))
        if kind == "integer":
            assert np.array_equal(got[0].cpu().numpy(), kr.knn(X, k, self_first=self_first)[0])
    again = hg.ops.knn(x, k, self_first=False, form="dot")
    _same(again, got, "two calls")


@pytest.mark.parametrize("nq,n", [(70, 300), (300, 70)])
def test_queries_are_not_the_candidates(hg, nq, n):
    F = 33
    for kind, make in (("integer", _ints), ("randn", _randn)):
        X, Q = make(n, F, 41), make(nq, F, 42)
        Q[:8] = X[40:48]  # queries that coincide with candidates: distance 0, no self rule
        x, q = _dev(X), _dev(Q)
        for k in (1, 10, 64):
            want = hg.ops.knn(x, k, queries=q)
            got = hg.ops.knn(x, k, queries=q, form="dot", return_fallback=True)
            _same(got, want, "queries %s nq=%d n=%d k=%d" % (kind, nq, n, k))
            assert got[2].shape == (nq,) and got[2].dtype == torch.int32
            if kind == "integer":
                assert np.array_equal(got[0].cpu().numpy(), kr.knn(X, k, queries=Q)[0])
    x = _dev(_randn(300, F, 43))
    _same(hg.ops.knn(x, 10, self_first=False, form="dot"), hg.ops.knn(x, 10, self_first=False), "self_first=False on X itself")


def test_rows_one_float_off_a_16_byte_boundary(hg):
    n, F, k = 257, 33, 10
    X = _ints(n, F, 11)
    buf = torch.zeros(n * F + 1, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    x = buf[1:].view(n, F)
    x.copy_(torch.from_numpy(X))
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    got = hg.ops.knn(x, k, form="dot")
    _same(got, hg.ops.knn(x, k), "offset rows")
    assert np.array_equal(got[0].cpu().numpy(), kr.knn(X, k)[0])
    q = torch.zeros(65 * F + 1, dtype=torch.float32, device=DEV)[1:].view(65, F)
    q.copy_(torch.from_numpy(_ints(65, F, 12)))
    _same(hg.ops.knn(x, k, queries=q, form="dot"), hg.ops.knn(x, k, queries=q), "offset rows and queries")


@pytest.mark.parametrize("kind", ["integer", "randn"])
def test_cand_slices(hg, kind):
    n, F, k = 700, 33, 10
    X = _ints(n, F, 5) if kind == "integer" else _randn(n, F, 6)
    x = _dev(X)
    want = hg.ops.knn(x, k, cand_slices=1)
    fb0 = None
    for cs in (0, 1, 2, 8):
        idx, dist, mean, fb = hg.ops.knn(x, k, return_mean=True, cand_slices=cs, form="dot", return_fallback=True)
        _same((idx, dist), want, "cand_slices=%d" % cs)
        again = hg.ops.knn(x, k, return_mean=True, cand_slices=cs, form="dot")
        assert torch.equal(mean.view(torch.int32), again[2].view(torch.int32)), "mean differs between two calls, cand_slices=%d" % cs
        fb0 = fb if fb0 is None else fb0
        assert torch.equal(fb, fb0), "the merged shortlist, and so the certificate, does not depend on the slices"
    for kk in (33, 64):  # two and three shortlist slots per lane, merged
        _same(hg.ops.knn(x, kk, cand_slices=8, form="dot"), hg.ops.knn(x, kk, cand_slices=1), "k=%d" % kk)


@pytest.mark.parametrize("kind", ["integer", "randn"])
@pytest.mark.parametrize("nq", [5, 130])
def test_merge_of_32_slices(hg, nq, kind):
    """Few queries against 4100 candidates: 33 candidate tiles of 128 rows, so cand_slices = 32 is not clipped, and the
    default picks it too (512 workgroups over one or two query tiles).  The rerank merges 32 shortlists a row."""
    from hypergef_amd import _lib
    n, F = 4100, 3
    make = _ints if kind == "integer" else _randn
    X, Q = make(n, F, 91), make(nq, F, 92)
    x, q = _dev(X), _dev(Q)
    D = kr.distances(Q, X) if kind == "integer" else None
    L = _lib.lib()
    for k in (10, 64):
        # the workspace says how many slices the call takes: slices nq (8 kp + 4) bytes of lists and partial means, each of
        # the three pieces rounded up by less than 256 bytes, beside what does not depend on the slices
        kp = 32 * dr.slots(k)
        bytes_of = {cs: L.hg_knn_dot_workspace_bytes(nq, n, F, k, cs) for cs in (0, 1, 31, 32)}
        per = nq * (8 * kp + 4)
        assert abs(bytes_of[32] - bytes_of[1] - 31 * per) < 3 * 256, bytes_of
        assert bytes_of[32] > bytes_of[31], "32 slices were clipped"
        assert bytes_of[0] == bytes_of[32], "the default did not pick 32 slices"
        want = hg.ops.knn(x, k, queries=q, form="difference")
        one = hg.ops.knn(x, k, queries=q, form="dot", cand_slices=1, return_fallback=True)
        _same(one, want, "%s nq=%d k=%d, one slice" % (kind, nq, k))
        for cs in (0, 32):
            got = hg.ops.knn(x, k, queries=q, form="dot", cand_slices=cs, return_fallback=True)
            _same(got, want, "%s nq=%d k=%d cand_slices=%d" % (kind, nq, k, cs))
            assert torch.equal(got[2], one[2]), "fallback differs from one slice's, cand_slices=%d" % cs
            if kind == "integer":
                assert np.array_equal(got[0].cpu().numpy(), kr.knn(X, k, queries=Q, D=D)[0])


def _overflow_case(name, n=dr.CASE_N):
    """overflow: randn with row 7 times 1e19 -- its norm is infinite, every difference with it is finite and every distance
    to it +inf, never NaN.  huge: randn times 4e17 -- every norm and every distance is finite, and n2q + n2max >= 1e37."""
    X = np.random.default_rng({"overflow": 6, "huge": 7}[name]).standard_normal((n, dr.CASE_F)).astype(np.float32)
    if name == "overflow":
        X[7] *= np.float32(1e19)
    else:
        X *= np.float32(4e17)
    with np.errstate(over="ignore", invalid="ignore"):
        total = dr._bound(X, X)[1]
        D = dr.d2_f32(X, X)
    assert np.isfinite(X).all() and not np.isnan(D).any()
    if name == "overflow":
        assert np.isinf(total).all() and np.isinf(D[7, np.arange(n) != 7]).all() and D[7, 7] == 0
        assert np.isfinite(np.delete(np.delete(D, 7, 0), 7, 1)).all()
    else:
        assert np.isfinite(total).all() and (total >= 1e37).all() and np.isfinite(D).all()
    return X


@pytest.mark.parametrize("name", ["overflow", "huge"])
def test_norms_that_overflow_take_the_exhaustive_path(hg, name):
    X = _overflow_case(name)
    x = _dev(X)
    n, k = dr.CASE_N, dr.CASE_K
    for self_first in (True, False):
        want = hg.ops.knn(x, k, self_first=self_first)
        got = hg.ops.knn(x, k, self_first=self_first, form="dot", return_fallback=True)
        _same(got, want, "%s self_first=%s" % (name, self_first))
        assert int(got[2].sum()) == n, "%s: %d rows were certified" % (name, n - int(got[2].sum()))
        idx, dist = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert not np.isnan(dist).any()
        if name == "overflow":
            assert not (np.delete(idx, 7, 0) == 7).any(), "row 7, at +inf from every other row, is in another row's list"
            assert np.isfinite(np.delete(dist, 7, 0)).all()
            if self_first:  # all others tie at +inf: the index decides
                assert idx[7].tolist() == [7] + [j for j in range(n) if j != 7][:k - 1]
                assert dist[7, 0] == 0 and np.isposinf(dist[7, 1:]).all()
    # n <= kp: nothing is left out of the shortlist and no certificate is taken
    small = _dev(_overflow_case(name, 20))
    for self_first in (True, False):
        _same(hg.ops.knn(small, k, self_first=self_first, form="dot"), hg.ops.knn(small, k, self_first=self_first),
              "%s, n = 20, self_first=%s" % (name, self_first))


def _run_case(hg, name, self_first=True):
    X = dr.case(name)
    x = _dev(X)
    want = hg.ops.knn(x, dr.CASE_K, self_first=self_first)
    got = hg.ops.knn(x, dr.CASE_K, self_first=self_first, form="dot", return_fallback=True)
    _same(got, want, name)
    return X, got


def test_certified_input_takes_no_fallback(hg):
    for self_first in (True, False):
        X, got = _run_case(hg, "certified", self_first)
        assert dr.certifiable(None, X, dr.CASE_K, self_first=self_first)
        assert int(got[2].sum()) == 0, "%d rows fell back" % int(got[2].sum())
    zeros = hg.ops.knn(_dev(X), dr.CASE_K, return_fallback=True)[2]
    assert zeros.dtype == torch.int32 and zeros.shape == (dr.CASE_N,) and int(zeros.sum()) == 0  # form="difference"


@pytest.mark.parametrize("name", ["identical", "pairs", "offset"])
def test_fallback_input_takes_the_exhaustive_path_on_every_row(hg, name):
    X, got = _run_case(hg, name)
    assert not dr.certifiable(None, X, dr.CASE_K)
    assert int(got[2].sum()) == dr.CASE_N, "%d rows were certified" % (dr.CASE_N - int(got[2].sum()))
    assert torch.equal(got[0][:, 0].cpu(), torch.arange(dr.CASE_N, dtype=torch.int32))  # self_first on the exhaustive path
    if name != "offset":
        assert bool((got[1][:, :2] == 0).all())
    if name == "pairs":  # row 150 + i leads with itself although row i is identical and smaller
        _, off = _run_case(hg, name, self_first=False)
        assert bool((off[0][150:, 0] < 150).all()) and int(off[2].sum()) == dr.CASE_N


def test_mixed_input_takes_both_paths(hg):
    X, got = _run_case(hg, "mixed")
    fb = got[2].cpu().numpy()
    assert fb[:240].sum() == 0, "separated rows fell back: %d" % int(fb[:240].sum())
    assert fb[240:].sum() == 60, "cluster rows certified: %d" % int(60 - fb[240:].sum())


@pytest.mark.parametrize("name", ["certified", "offset", "mixed"])
def test_mean_is_within_the_bound_of_the_float64_mean(hg, name):
    """|sqrt(max(a, 0)) - sqrt(b)| <= sqrt(|a - b|) for b >= 0, so every term is within sqrt(E1) of the truth; a float32 sum of
    n non-negative terms, each the hardware's 1-ulp square root, and one division add (n + 2) 2^-23 relative to the mean;
    a d~ below the smallest normal number counts as 0, at most sqrt(2^-126) per term."""
    X = dr.case(name)
    n = X.shape[0]
    for Qn in (None, X[:70] + np.float32(0.25)):
        Q = X if Qn is None else Qn
        want = kr.knn(X, 1, queries=Qn)[2]
        E1 = dr.bound(Q, X).astype(np.float64)
        tol = np.sqrt(E1) + (n + 2) * U23 * (want + np.sqrt(E1)) + 2.0 ** -63
        for cs in (0, 1, 8):
            mean = hg.ops.knn(_dev(X), 1, queries=None if Qn is None else _dev(Qn), return_mean=True, form="dot", cand_slices=cs)[2]
            err = np.abs(mean.cpu().numpy().astype(np.float64) - want)
            print("%s cand_slices=%d: max |mean - mean_f64| / bound = %.3g" % (name, cs, float((err / tol).max())))
            assert (err <= tol).all()


def test_dynamic_layer_is_captured_and_replayed(hg):
    """One training step (forward, backward) of the device-only layer with the dot-form search, captured once and replayed
    with changed input: the neighbours are searched again, and everything equals the eager step and knn_form="difference"."""
    n, F, k = 100, 32, 4
    inputs = [_dev(_randn(n, F, 70 + i)) for i in range(3)]
    G = _dev(_randn(n, F, 80))

    def fresh(form):
        torch.manual_seed(5)
        return hg.DynamicHypergraphConv(F, F, k, device_graph=True, knn_form=form).to(DEV)

    def eager(layer, X):
        layer.lin.weight.grad = None
        y = layer(X)
        y.backward(G)
        return y.detach().clone(), layer.lin.weight.grad.detach().clone(), layer.hyperg.idx.clone()

    layer, plain = fresh("dot"), fresh("difference")
    want = [eager(layer, X) for X in inputs]
    for got, ref in zip(want, [eager(plain, X) for X in inputs]):
        for u, v in zip(got, ref):
            assert torch.equal(u, v), "knn_form='dot' and 'difference' differ in the eager step"
    assert not torch.equal(want[1][2], want[2][2])  # a stale graph could not pass

    static_x = inputs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            layer.lin.weight.grad = None
            layer(static_x).backward(G)
    torch.cuda.current_stream().wait_stream(side)
    layer.lin.weight.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = layer(static_x)
        static_y.backward(G)
    static_idx = layer.hyperg.idx
    for i in (1, 2):
        static_x.copy_(inputs[i])
        graph.replay()
        torch.cuda.synchronize()
        y, gw, idx = want[i]
        assert torch.equal(static_idx, idx), "replay with input %d: the neighbours were not searched again" % i
        assert torch.equal(static_y, y) and torch.equal(layer.lin.weight.grad, gw), "replay with input %d" % i


def test_from_knn_builds_the_same_hypergraph(hg):
    n, F, k = 300, 16, 5
    for X in (_ints(n, F, 51), _randn(n, F, 52)):
        a = hg.HyperGraph.from_knn(torch.from_numpy(X), k, DEV, form="dot")
        b = hg.HyperGraph.from_knn(torch.from_numpy(X), k, DEV, form="difference")
        assert torch.equal(a.H_T_colind, b.H_T_colind) and torch.equal(a.H_T_csrptr, b.H_T_csrptr)
        assert torch.equal(a.knn_dist.view(torch.int32), b.knn_dist.view(torch.int32))
        assert torch.equal(a.degE, b.degE) and torch.equal(a.degV, b.degV)
    g = hg.KnnHypergraph.build(_dev(X), k, form="dot")
    h = hg.KnnHypergraph.build(_dev(X), k)
    assert torch.equal(g.idx, h.idx) and torch.equal(g.ptr_v, h.ptr_v) and torch.equal(g.pos_v, h.pos_v)
