"""ops.knn(form="dot") without a device: what is refused before a device is touched, the C entry's refusal codes and
workspace bound, and the certificate's logic on the host model (tests/_knn_dot_ref.py): whatever the estimates are, as long as
each lies within bound(Q, X) of the float64 truth, shortlist + rerank + certify + fall back must return the exhaustive
difference-form selection."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_dot_ref as dr  # noqa: E402
import _knn_ref as kr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "hg_aggr.h")).read()
    for name in ("hg_knn_dot_f32", "hg_knn_dot_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert "%s(" % name in header, name
    assert "BIT FOR BIT" in header
    makefile = open(os.path.join(ROOT, "hypergef_amd", "csrc", "Makefile")).read()
    assert "hg_knn_dot.hip" in makefile.split("SRCS")[1].split("\n")[0]


def test_form_refusals_fire_without_a_device(hg):
    knn = hg.ops.knn
    x = torch.zeros(10, 4)
    q = torch.zeros(3, 4)
    with pytest.raises(ValueError, match="form must be one of"):
        knn(x, 3, form="auto")
    with pytest.raises(ValueError, match="form must be one of"):
        knn(x, 3, form=None)
    with pytest.raises(TypeError, match="float32"):  # the dtype before the form
        knn(x.double(), 3, form="auto")
    with pytest.raises(ValueError, match='form="dot" cannot be combined with segments'):
        knn(x, 3, segments=[0, 5, 10], form="dot")
    with pytest.raises(ValueError, match="k"):  # k before the form's own refusals
        knn(x, 0, segments=[0, 5, 10], form="dot")
    with pytest.raises(ValueError, match="at most 65536 columns"):
        knn(torch.zeros(2, 65537), 1, form="dot")
    with pytest.raises(ValueError, match="self_first cannot be combined with queries"):
        knn(x, 3, queries=q, self_first=True, form="dot")
    # what is left is the device, for both forms and with the new result
    for kw in (dict(form="dot"), dict(form="dot", return_fallback=True, return_mean=True), dict(form="difference", return_fallback=True),
               dict(form="dot", queries=q), dict(form="dot", cand_slices=8)):
        with pytest.raises(RuntimeError, match="GPU"):
            knn(x, 3, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        knn(torch.zeros(2, 65536), 1, form="dot")  # the cap itself is admitted
    # the same keyword through the layers
    with pytest.raises(ValueError, match="form must be one of"):
        hg.HyperGraph.from_knn(x, 3, "cpu", form="fast")
    with pytest.raises(ValueError, match="form must be one of"):
        hg.KnnHypergraph.build(x, 3, form="fast")
    with pytest.raises(ValueError, match="cannot be combined with segments"):
        hg.KnnHypergraph.build(x, 3, segments=[0, 5, 10], form="dot")
    with pytest.raises(RuntimeError, match="GPU"):
        hg.KnnHypergraph.build(x, 3, form="dot")
    layer = hg.DynamicHypergraphConv(4, 4, 3, device_graph=True, knn_form="fast")
    with pytest.raises(ValueError, match="form must be one of"):
        layer(x)


def test_c_entry_refusals_and_workspace(hg):
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

    def call(k=3, q=None, nq=n, self_first=0, slices=1, workspace=ws, F=F):
        return L.hg_knn_dot_f32(p(X if q is None else q), nq, p(X), n, F, k, self_first, slices, p(idx), p(dist), null, null,
                                null if workspace is None else p(workspace), 0 if workspace is None else workspace.nbytes, null)

    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED
    for k in (0, -3, 65):
        assert call(k=k) == INV and b"hg_knn_dot_f32: k must be in 1 .. 64" in L.hg_last_error()
    assert call(k=11) == INV and b"exceeds" in L.hg_last_error()
    assert call(F=65537) == INV and b"above 65536" in L.hg_last_error()
    assert call(F=0) == INV
    assert call(q=Q, nq=3, self_first=1) == INV and b"self_first needs Q == X" in L.hg_last_error()
    assert call(slices=-1) == INV and b"cand_slices" in L.hg_last_error()
    assert call(k=0, slices=33) == INV
    assert call(slices=33) == UNS and b"cand_slices above 32" in L.hg_last_error()
    assert call(workspace=None) == _lib.HG_ERR_WORKSPACE
    assert call(workspace=np.zeros(8, np.uint8)) == _lib.HG_ERR_WORKSPACE
    assert b"hg_knn_dot_workspace_bytes asks for" in L.hg_last_error()
    assert not idx.any() and not dist.any() and not ws.any()
    # O(nq (k + shortlist) + nq + n): never anything of nq x n or nq x tiles
    for nq, n_ in ((1, 1), (1, 100000), (65, 257), (300, 300), (12311, 12311), (50000, 50000), (7, 50000), (50000, 64)):
        for k in (1, 10, 16, 17, 48, 49, 64):
            if k > n_:
                continue
            kp = min(n_, 32 * dr.slots(k))
            assert k <= kp <= 96 and (n_ <= kp or kp - k >= 16)
            for cs in (0, 1, 2, 8, 32):
                got = L.hg_knn_dot_workspace_bytes(nq, n_, 1024, k, cs)
                assert 0 < got <= 4 * (n_ + nq + n_ // 64) + 32 * nq * (8 * kp + 4) + 2048, (nq, n_, k, cs, got)
    for args in ((0, 5, 4, 1, 0), (5, 0, 4, 1, 0), (5, 5, 0, 1, 0), (5, 5, 65537, 1, 0), (5, 5, 4, 0, 0), (5, 5, 4, 65, 0),
                 (5, 5, 4, 6, 0), (5, 5, 4, 1, -1), (5, 5, 4, 1, 33)):
        assert L.hg_knn_dot_workspace_bytes(*args) == 0, args


def _rows(kind, n, F, seed):
    rng = np.random.default_rng(seed)
    if kind == "integer":  # many ties
        X = rng.integers(-2, 3, (n, F))
    elif kind == "identical":
        X = np.repeat(rng.standard_normal((1, F)), n, axis=0)
    elif kind == "offset":  # severe cancellation in the dot form
        X = 1000.0 + 1e-3 * rng.standard_normal((n, F))
    elif kind == "randn":
        X = rng.standard_normal((n, F))
    else:  # randn with a zero row (and a duplicate of it) among them
        X = rng.standard_normal((n, F))
        X[3] = 0.0
        X[n - 2] = 0.0
    return np.ascontiguousarray(X, np.float32)


SEEN = set()


@pytest.mark.parametrize("kind", ["integer", "identical", "offset", "randn", "zero_row"])
def test_adversarial_estimates_never_change_the_result(kind):
    n, F = 90, 6
    X = _rows(kind, n, F, 7)
    Q = _rows(kind, 11, F, 8)
    rng = np.random.default_rng(9)
    for queries in (None, Q):
        Qa = X if queries is None else queries
        D64 = kr.distances(Qa, X)
        D32 = dr.d2_f32(Qa, X)
        E1 = dr.bound(Qa, X)
        assert (E1 > 0).all()
        for self_first in ((True, False) if queries is None else (False,)):
            for k, slack in ((1, 1), (3, 2), (3, None), (10, 5), (10, None), (64, None), (64, 200)):
                want = dr.exhaustive(X, k, queries, self_first, D32=D32)
                ref = kr.knn(X, k, queries=queries, self_first=self_first, D=D64)
                if kind == "integer":  # float32 is exact here: the float64 reference is the same selection
                    assert np.array_equal(want[0], ref[0]) and np.array_equal(want[1].astype(np.float64), ref[1])
                top = np.zeros(D64.shape, bool)
                top[np.arange(D64.shape[0])[:, None], ref[0]] = True
                for mode in ("exclude", "random", "truth"):
                    est = D64 if mode == "truth" else dr.perturbed(D64, E1, top, mode, rng)
                    idx, dist, fb = dr.scheme(X, k, est, queries, self_first, slack=slack, D32=D32)
                    what = (kind, queries is None, self_first, k, slack, mode)
                    assert np.array_equal(idx, want[0]), what
                    assert np.array_equal(dist.view(np.int32), want[1].view(np.int32)), what
                    assert not np.signbit(dist).any(), what
                    SEEN.update(fb.tolist())
                    if k + (dr.default_slack(k) if slack is None else slack) >= n:
                        assert not fb.any(), what  # nothing was left out
    assert SEEN == {0, 1} or kind in ("integer", "identical")  # both paths were taken by the time the float kinds ran


def test_an_estimate_outside_the_bound_is_caught_by_this_test():
    """The test above is not vacuous: estimates far outside the bound -- every one too large, the true neighbours' by more --
    keep the neighbours off the shortlist under a large T, and the certificate passes a wrong row."""
    X = _rows("randn", 90, 6, 7)
    D64, D32 = kr.distances(X, X), dr.d2_f32(X, X)
    want = dr.exhaustive(X, 3, D32=D32)
    top = np.zeros(D64.shape, bool)
    top[np.arange(90)[:, None], want[0]] = True
    est = D64 + np.where(top, 1000.0, 40.0) * D64.max()
    idx, _, fb = dr.scheme(X, 3, est, slack=2, D32=D32)
    assert not np.array_equal(idx, want[0]) and not fb.all()


def test_bound_holds_for_the_float32_dot_form():
    """|d~ - d2_f64| <= E1 for d~ computed as the kernels do (float32 norms, a float32 fma chain for q.x), on the kinds above,
    wide rows included; and the float32 difference form is within (F + 2) u of the truth from below."""
    for kind, n, F in (("integer", 40, 6), ("offset", 40, 6), ("randn", 40, 6), ("zero_row", 40, 6), ("randn", 12, 4099),
                       ("offset", 12, 1028)):
        X = _rows(kind, n, F, 21)
        Q = _rows(kind, 9, F, 22)
        n2q, n2x = dr.norms(Q), dr.norms(X)
        s = np.zeros((9, n), np.float32)
        for c in range(F):
            s = dr._fma32(np.broadcast_to(Q[:, c][:, None], s.shape), np.broadcast_to(X[:, c][None, :], s.shape), s)
        est = ((n2q[:, None] + n2x[None, :]).astype(np.float32) - np.float32(2) * s).astype(np.float32)
        D64 = kr.distances(Q, X)
        E1 = dr.bound(Q, X).astype(np.float64)
        err = np.abs(est.astype(np.float64) - D64)
        print("%s F=%d: max |d~ - d2| / E1 = %.3g" % (kind, F, float((err / E1[:, None]).max())))
        assert (err <= E1[:, None]).all(), (kind, F)
        D32 = dr.d2_f32(Q, X).astype(np.float64)
        assert (D32 >= D64 * (1 - (F + 2) * 2.0 ** -24)).all(), (kind, F)


def test_the_device_tests_inputs_are_what_they_are_named():
    k = dr.CASE_K
    assert dr.certifiable(None, dr.case("certified"), k)
    assert dr.certifiable(None, dr.case("certified"), k, self_first=False)
    for name in ("identical", "pairs", "offset", "mixed"):
        assert not dr.certifiable(None, dr.case(name), k), name
    # no estimate within the bound can certify a row of these two: every row falls back by the reference alone
    assert dr.never_certifiable(None, dr.case("identical"), k)
    assert dr.never_certifiable(None, dr.case("pairs"), k)
    assert not dr.never_certifiable(None, dr.case("certified"), k) and not dr.never_certifiable(None, dr.case("mixed"), k)
    X = dr.case("pairs")
    assert np.array_equal(X[:150], X[150:])
    # offset: E1 is about 1e3 against distances of about 1e-4 -- a certificate needs an estimate above E1, which the float32 dot
    # form, exact to about sqrt(F) ulps of 1.3e8 (about 60), does not produce
    E1 = dr.bound(dr.case("offset"), dr.case("offset"))
    assert E1.min() > 500 and kr.distances(dr.case("offset"), dr.case("offset")).max() < 1e-2
    # mixed: the 240 separated rows are certifiable among themselves and with the cluster present
    M = dr.case("mixed")
    assert dr.certifiable(M[:240], M, k, self_first=False) and not dr.certifiable(M[240:], M, k, self_first=False)
