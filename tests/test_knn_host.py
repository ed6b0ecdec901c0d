"""k-nearest-neighbour construction without a device: the exported names, what ops.knn refuses before a device is touched
and in which order, the C entry's refusal codes (decided before any device call: every pointer here is host memory), the
workspace bound, tests/_knn_ref.py against the definition written as loops, and HyperGraph.from_knn's CSR layout."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_ref as kr  # noqa: E402

SYMBOLS = ("hg_knn_f32", "hg_knn_workspace_bytes")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "hg_aggr.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert "%s(" % name in header, name
    assert "TOTAL ORDER (d2, j)" in header  # the tie rule is part of the contract
    assert L.hg_version() == 410  # detected by symbol: the version does not move
    for name in ("knn", "knn_incidence_weights", "DynamicHypergraphConv"):
        assert hasattr(hg, name), name
    assert hg.knn is hg.ops.knn and hg.knn_incidence_weights is hg.ops.knn_incidence_weights
    assert hg.DynamicHypergraphConv is hg.models.DynamicHypergraphConv
    assert hasattr(hg.HyperGraph, "from_knn") and hasattr(hg.HyperGraph, "knn_weights")
    makefile = open(os.path.join(ROOT, "hypergef_amd", "csrc", "Makefile")).read()
    assert "hg_knn.hip" in makefile.split("SRCS")[1].split("\n")[0] and "hg_knn.h" in makefile.split("HDRS")[1].split("\n")[0]


def test_ops_knn_refusals_and_their_order(hg):
    knn = hg.ops.knn
    x = torch.zeros(10, 4)
    q = torch.zeros(3, 4)
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            knn(x.to(dt), 3)
        with pytest.raises(TypeError, match="float32"):
            knn(x, 3, queries=q.to(dt))
        with pytest.raises(TypeError, match="float32"):  # the dtype before k
            knn(x.to(dt), 0)
    for k in (0, -1, 65, 11):
        with pytest.raises(ValueError, match="k"):
            knn(x, k)
    with pytest.raises(ValueError, match="k"):  # k before segments + queries
        knn(x, 0, queries=q, segments=[0, 10])
    with pytest.raises(ValueError, match="segments cannot be combined with queries"):
        knn(x, 3, queries=q, segments=[0, 10])
    with pytest.raises(ValueError, match="segments cannot be combined with queries"):  # before self_first + queries
        knn(x, 3, queries=q, segments=[0, 10], self_first=True)
    with pytest.raises(ValueError, match="self_first cannot be combined with queries"):
        knn(x, 3, queries=q, self_first=True)
    with pytest.raises(ValueError, match="segment 1 has 2 rows, fewer than k = 3"):
        knn(x, 3, segments=[0, 5, 7, 10])
    with pytest.raises(ValueError, match="segments"):
        knn(x, 3, segments=[0, 5, 9])
    with pytest.raises(ValueError, match="ascend"):
        knn(x, 1, segments=[0, 7, 5, 10])
    with pytest.raises(ValueError, match="cand_slices"):
        knn(x, 3, cand_slices=33)
    xg = torch.zeros(10, 4, requires_grad=True)
    with pytest.raises(RuntimeError, match=r"torch.no_grad\(\) or on X.detach\(\)"):
        knn(xg, 3)
    with pytest.raises(ValueError, match="fewer than k"):  # the short segment before the gradient and the device
        knn(xg, 3, segments=[0, 2, 10])
    # what is left is the device
    for call in (lambda: knn(x, 3), lambda: knn(x, 3, queries=q), lambda: knn(x, 3, segments=[0, 5, 10], return_mean=True),
                 lambda: knn(xg.detach(), 3)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="GPU"):
            knn(xg, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        hg.HyperGraph.from_knn(x, 3, "cpu")
    with pytest.raises(TypeError, match="float32"):
        hg.HyperGraph.from_knn(x.double(), 3, "cpu")


def test_c_entry_refuses_before_any_device_call(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    n, F = 10, 4
    X = np.zeros((n, F), np.float32)
    Q = np.zeros((3, F), np.float32)
    idx, dist = np.zeros((n, 64), np.int32), np.zeros((n, 64), np.float32)
    ws = np.zeros(1 << 16, np.uint8)
    null = ctypes.c_void_p()

    def p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def call(k=3, q=None, nq=n, seg=None, self_first=0, slices=1, x=X, ncand=n, workspace=ws):
        s = None if seg is None else np.asarray(seg, np.int32)
        return L.hg_knn_f32(p(x if q is None else q), nq, p(x), ncand, F, k, null if s is None else p(s),
                            0 if s is None else len(s) - 1, self_first, slices, p(idx), p(dist), null,
                            null if workspace is None else p(workspace), 0 if workspace is None else workspace.nbytes, null)

    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED
    for k in (0, -3, 65):
        assert call(k=k) == INV and b"k must be in 1 .. 64" in L.hg_last_error()
    assert call(k=11) == INV and b"exceeds" in L.hg_last_error()
    assert call(seg=[0, 5, 7, 10]) == INV and b"segment 1 has 2 rows, fewer than k = 3" in L.hg_last_error()
    assert call(k=1, seg=[0, 7, 5, 10]) == INV and b"ascend" in L.hg_last_error()
    assert call(seg=[0, 5, 9]) == INV and b"seg[B] = n" in L.hg_last_error()
    assert call(seg=[1, 5, 10]) == INV and b"seg[0] = 0" in L.hg_last_error()
    assert call(q=Q, nq=3, self_first=1) == INV and b"self_first needs Q == X" in L.hg_last_error()
    assert call(nq=3, self_first=1) == INV and b"self_first needs Q == X" in L.hg_last_error()  # the same pointer, nq != n
    assert call(q=Q, nq=3, seg=[0, 5, 10]) == INV and b"seg needs Q == X" in L.hg_last_error()
    assert call(slices=-1) == INV and b"cand_slices" in L.hg_last_error()
    # the order: k before self_first before seg; the arguments before what is merely not implemented
    assert call(k=0, q=Q, nq=3, self_first=1, seg=[0, 7, 5, 10]) == INV and b"k must be" in L.hg_last_error()
    assert call(q=Q, nq=3, self_first=1, seg=[0, 7, 5, 10]) == INV and b"self_first" in L.hg_last_error()
    assert call(k=0, slices=33) == INV
    assert call(slices=33) == UNS and b"cand_slices above 32" in L.hg_last_error()
    assert L.hg_knn_f32(null, n, p(X), n, F, 3, null, 0, 0, 1, p(idx), p(dist), null, null, 0, null) == INV
    assert b"null" in L.hg_last_error()
    # a workspace is needed by more than one slice and by segments: refused, not launched
    assert call(slices=2, workspace=None) == _lib.HG_ERR_WORKSPACE
    assert call(seg=[0, 5, 10], workspace=None) == _lib.HG_ERR_WORKSPACE
    assert call(slices=4, workspace=np.zeros(8, np.uint8)) == _lib.HG_ERR_WORKSPACE
    assert b"hg_knn_workspace_bytes asks for" in L.hg_last_error()
    assert not idx.any() and not dist.any() and not ws.any()


def test_workspace_bound(hg):
    """The one hard claim: O(nq k + workspace), with workspace <= 16 nq k max(cand_slices, 1) + 4096."""
    from hypergef_amd import _lib
    L = _lib.lib()
    for nq, n in ((1, 1), (1, 100000), (65, 257), (300, 300), (2708, 2708), (12311, 12311), (100000, 100000),
                  (2708 * 1024, 2708 * 1024), (7, 50000), (50000, 64)):
        for k in (1, 2, 10, 64):
            if k > n:
                continue
            for F in (1, 33, 1024):
                for cs in (0, 1, 2, 3, 7, 32):
                    got = L.hg_knn_workspace_bytes(nq, n, F, k, cs)
                    assert got <= 16 * nq * k * max(cs, 1) + 4096, (nq, n, F, k, cs, got)
                    if cs > 1:  # and it really holds the other slices' lists
                        assert got >= 8 * nq * k * (cs - 1), (nq, n, F, k, cs, got)
    # arguments hg_knn_f32 refuses
    for args in ((0, 5, 4, 1, 0), (5, 0, 4, 1, 0), (5, 5, 0, 1, 0), (5, 5, 4, 0, 0), (5, 5, 4, 65, 0), (5, 5, 4, 6, 0),
                 (5, 5, 4, 1, -1), (5, 5, 4, 1, 33)):
        assert L.hg_knn_workspace_bytes(*args) == 0, args


def test_reference_agrees_with_the_loops():
    rng = np.random.default_rng(3)
    X = rng.integers(-2, 3, (7, 3)).astype(np.float32)  # 7 x 3 in {-2 .. 2}: ties and, below, an exact duplicate
    X[5] = X[2]
    Q = rng.integers(-2, 3, (4, 3)).astype(np.float32)
    cases = [dict(), dict(self_first=False), dict(queries=Q), dict(segments=[0, 3, 7]), dict(segments=[0, 3, 7], self_first=False)]
    for kw in cases:
        for k in (1, 2, 3):
            got, want = kr.knn(X, k, **kw), kr.knn_loops(X, k, **kw)
            assert np.array_equal(got[0], want[0]), (kw, k)
            assert np.array_equal(got[1], want[1]), (kw, k)
            assert np.allclose(got[2], want[2], rtol=1e-15, atol=0), (kw, k)
    # the duplicate: row 5 equals row 2.  Without self_first the smaller index leads row 5; with it, row 5 itself
    assert kr.knn(X, 2, self_first=False)[0][5].tolist() == [2, 5]
    assert kr.knn(X, 2, self_first=True)[0][5].tolist() == [5, 2]
    idx, dist, _ = kr.knn(X, 3, segments=[0, 3, 7])
    assert (idx[:3] < 3).all() and (idx[3:] >= 3).all()
    assert (np.diff(dist, axis=1) >= 0).all()
    float_X = rng.standard_normal((7, 3)).astype(np.float32)
    got, want = kr.knn(float_X, 4), kr.knn_loops(float_X, 4)
    assert np.array_equal(got[0], want[0]) and np.allclose(got[1], want[1], rtol=1e-14, atol=0)


def test_from_knn_layout_without_a_device(hg):
    from hypergef_amd import knn_graph
    idx = np.array([[0, 2, 1], [1, 0, 3], [2, 0, 1], [3, 1, 2]], np.int32)  # a hand-made neighbour table, self first
    inc = knn_graph.incidence_from_knn(idx, "hand")
    assert (inc.N, inc.M, inc.nnz, inc.name) == (4, 4, 12, "hand")
    assert inc.csrptr.dtype == np.int32 and inc.csrptr.tolist() == [0, 3, 6, 9, 12]
    assert inc.colind.dtype == np.int32 and inc.colind.tolist() == idx.reshape(-1).tolist()
    with pytest.raises(ValueError):
        knn_graph.incidence_from_knn(np.array([[0, 4]]))
    with pytest.raises(ValueError):
        knn_graph.incidence_from_knn(np.arange(3))
    # the weights line up with those positions: entry (i, s) of dist is H_T position i k + s
    dist = torch.tensor([[0.0, 1.0, 4.0], [0.0, 2.0, 2.0], [0.0, 1.0, 9.0], [0.0, 4.0, 4.0]])
    mean = torch.tensor([1.0, 2.0, 0.5, 4.0])
    w = hg.ops.knn_incidence_weights(dist, mean, m_prob=2.0)
    assert w.shape == (12,)
    want = torch.exp(-dist / (2.0 * mean[:, None]) ** 2).reshape(-1)
    assert torch.equal(w, want) and float(w[0]) == 1.0
    assert abs(float(w[5]) - np.exp(-2.0 / 16.0)) < 1e-7
