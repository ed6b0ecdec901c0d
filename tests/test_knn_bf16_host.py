"""ops.knn(form="dot") on bfloat16 rows without a device: the exports and the C entries' refusals, what Python refuses before a
device is touched, the bound E1b against three models of the bf16 matrix unit's accumulation on adversarial rows, and the
certificate's logic under E1b with injected estimates (tests/_knn_bf16_ref.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_bf16_ref as br  # noqa: E402
import _knn_dot_ref as dr  # noqa: E402
import _knn_ref as kr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hg_knn_dot_bf16", "hg_knn_dot_bf16_workspace_bytes", "hg_knn_dot_estimates_bf16")


def test_exports(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "hg_aggr.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert "%s(" % name in header, name
    assert "DIAGNOSTIC" in header and "HYPOTHESIS H" in header
    makefile = open(os.path.join(ROOT, "hypergef_amd", "csrc", "Makefile")).read()
    assert "hg_knn_dot.hip" in makefile.split("SRCS")[1].split("\n")[0]
    assert L.hg_version() == 410


def test_c_entry_refusals_and_workspace(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    n, F = 10, 4
    X = np.zeros((n, F), np.uint16)
    Q = np.zeros((3, F), np.uint16)
    idx, dist = np.zeros((n, 64), np.int32), np.zeros((n, 64), np.float32)
    ws = np.zeros(1 << 16, np.uint8)
    null = ctypes.c_void_p()

    def p(a, off=0):
        return ctypes.c_void_p(a.ctypes.data + off)

    def call(k=3, q=None, nq=n, self_first=0, slices=1, workspace=ws, F=F, x_off=0, idx_off=0):
        return L.hg_knn_dot_bf16(p(X if q is None else q, x_off if q is None else 0), nq, p(X, x_off), n, F, k, self_first, slices,
                                 p(idx, idx_off), p(dist), null, null, null if workspace is None else p(workspace),
                                 0 if workspace is None else workspace.nbytes, null)

    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED
    for k in (0, -3, 65):
        assert call(k=k) == INV and b"hg_knn_dot_bf16: k must be in 1 .. 64" in L.hg_last_error()
    assert call(k=11) == INV and b"exceeds" in L.hg_last_error()
    assert call(F=65537) == INV and b"above 65536" in L.hg_last_error()
    assert call(F=0) == INV
    assert call(q=Q, nq=3, self_first=1) == INV and b"self_first needs Q == X" in L.hg_last_error()
    assert call(slices=-1) == INV and b"cand_slices" in L.hg_last_error()
    assert call(k=0, slices=33) == INV
    assert call(slices=33) == UNS and b"cand_slices above 32" in L.hg_last_error()
    assert call(x_off=1) == UNS and b"2-byte aligned" in L.hg_last_error()
    assert call(idx_off=2) == UNS and b"4-byte aligned" in L.hg_last_error()
    assert call(workspace=None) == _lib.HG_ERR_WORKSPACE
    assert call(workspace=np.zeros(8, np.uint8)) == _lib.HG_ERR_WORKSPACE
    assert b"hg_knn_dot_bf16_workspace_bytes asks for" in L.hg_last_error()
    assert not idx.any() and not dist.any() and not ws.any()
    # the workspace is the host formula's, and the float32 entry's: the same pieces
    for nq, n_ in ((1, 1), (1, 100000), (65, 257), (300, 300), (12311, 12311), (7, 50000), (50000, 64)):
        for k in (1, 10, 16, 17, 48, 49, 64):
            if k > n_:
                continue
            for cs in (0, 1, 2, 8, 32):
                got = L.hg_knn_dot_bf16_workspace_bytes(nq, n_, 1024, k, cs)
                assert got == dr.dot_workspace_bytes(nq, n_, k, dr.dot_slices(nq, n_, cs)), (nq, n_, k, cs)
                assert got == L.hg_knn_dot_workspace_bytes(nq, n_, 1024, k, cs)
    for args in ((0, 5, 4, 1, 0), (5, 0, 4, 1, 0), (5, 5, 0, 1, 0), (5, 5, 65537, 1, 0), (5, 5, 4, 0, 0), (5, 5, 4, 65, 0),
                 (5, 5, 4, 6, 0), (5, 5, 4, 1, -1), (5, 5, 4, 1, 33)):
        assert L.hg_knn_dot_bf16_workspace_bytes(*args) == 0, args
    # the diagnostic entry
    est, e1 = np.zeros((n, n), np.float32), np.zeros(n, np.float32)

    def diag(nq=n, n_=n, F=F, x_off=0, e=est):
        return L.hg_knn_dot_estimates_bf16(p(X, x_off), nq, p(X, x_off), n_, F, null if e is None else p(e), p(e1), null)

    assert diag(e=None) == INV and b"hg_knn_dot_estimates_bf16: null" in L.hg_last_error()
    assert diag(nq=0) == INV and diag(F=0) == INV
    assert diag(F=65537) == INV and b"above 65536" in L.hg_last_error()
    assert diag(nq=2049, n_=2048) == UNS and b"diagnostic" in L.hg_last_error()
    assert diag(x_off=1) == UNS and b"aligned" in L.hg_last_error()
    assert not est.any() and not e1.any()


def test_python_refusals_fire_without_a_device(hg):
    knn = hg.ops.knn
    x = torch.zeros(10, 4)
    xb, qb = x.bfloat16(), torch.zeros(3, 4).bfloat16()
    # bfloat16 rows under "dot" now get as far as the device
    for kw in (dict(), dict(queries=qb), dict(return_mean=True, return_fallback=True, cand_slices=8)):
        with pytest.raises(RuntimeError, match="GPU"):
            knn(xb, 3, form="dot", **kw)
    # the refusals after the dtype, in their order
    with pytest.raises(ValueError, match="k"):
        knn(xb, 0, segments=[0, 5, 10], form="dot")
    with pytest.raises(ValueError, match='form="dot" cannot be combined with segments'):
        knn(xb, 3, segments=[0, 5, 10], form="dot")
    with pytest.raises(ValueError, match="at most 65536 columns"):
        knn(torch.zeros(2, 65537).bfloat16(), 1, form="dot")
    with pytest.raises(ValueError, match="self_first cannot be combined with queries"):
        knn(xb, 3, queries=qb, self_first=True, form="dot")
    # every other form, and every other dtype, as before: the dtype first
    for form in ("difference", "auto", None):
        with pytest.raises(TypeError, match="float32"):
            knn(xb, 3, form=form)
    with pytest.raises(TypeError, match="float32"):
        knn(xb, 3)
    with pytest.raises(TypeError, match="float32"):
        knn(xb, 3, queries=qb.float(), form="dot")
    with pytest.raises(TypeError, match="float32"):
        knn(x, 3, queries=qb, form="dot")
    with pytest.raises(TypeError, match="float32"):
        knn(xb, 0, queries=qb.float(), form="dot")  # the dtype before k
    for t in (x.half(), x.double()):
        for form in ("dot", "difference"):
            with pytest.raises(TypeError, match="float32"):
                knn(t, 3, form=form)
    with pytest.raises(TypeError, match="float32"):
        knn(xb, 3, queries=qb.half(), form="dot")
    # the layers
    with pytest.raises(RuntimeError, match="GPU"):
        hg.HyperGraph.from_knn(xb, 3, "cpu", form="dot")
    with pytest.raises(RuntimeError, match="GPU"):
        hg.KnnHypergraph.build(xb, 3, form="dot")
    for build in (lambda **kw: hg.HyperGraph.from_knn(xb, 3, "cpu", **kw), lambda **kw: hg.KnnHypergraph.build(xb, 3, **kw)):
        with pytest.raises(TypeError, match="float32"):
            build()
        with pytest.raises(TypeError, match="float32"):
            build(form="auto")
    with pytest.raises(TypeError, match="float32"):
        hg.HyperGraph.from_knn(x.half(), 3, "cpu", form="dot")
    for device_graph in (False, True):
        layer = hg.DynamicHypergraphConv(4, 4, 3, device_graph=device_graph, knn_form="dot").to(torch.bfloat16)
        with pytest.raises(RuntimeError, match="GPU"):
            layer(xb)
        layer = hg.DynamicHypergraphConv(4, 4, 3, device_graph=device_graph).to(torch.bfloat16)
        with pytest.raises(TypeError, match="float32"):
            layer(xb)


WIDTHS = (1, 15, 16, 17, 33, 200, 1024, 4096)


@pytest.mark.parametrize("kind", br.KINDS)
def test_bound_holds_under_every_model_of_the_accumulation(kind):
    """|d~ - d2_f64| <= E1b for d~ formed as the kernels form it, with the 16-column step emulated three ways, each with and
    without flushing subnormals: nothing here is tuned to the result, E1b is hg_aggr.h's."""
    worst = 0.0
    for F in WIDTHS:
        nq, n = (6, 12) if F <= 1024 else (3, 6)
        X, Q = br.rows(kind, n, F, 100 + F), br.rows(kind, nq, F, 200 + F)
        assert np.array_equal(X, br.to_bf16(X))
        D64 = br.distances(Q, X)
        E1 = br.bound_bf16(Q, X).astype(np.float64)
        assert np.isfinite(E1).all() and (E1 > 0).all()
        for model in br.MODELS:
            for flush in (False, True):
                est = br.estimates(Q, X, model, flush)
                err = np.abs(est.astype(np.float64) - D64)
                worst = max(worst, float((err / E1[:, None]).max()))
                assert (err <= E1[:, None]).all(), (kind, F, model, flush, float((err / E1[:, None]).max()))
    print("%s: max |d~ - d2| / E1b = %.3g" % (kind, worst))


def test_the_models_are_not_the_same_and_flushing_matters():
    """The emulation is not vacuous: the three models disagree in the last bits on wide randn rows, the truncating one errs
    most, and on the tiny rows flushing loses every product -- s~ is exactly 0 -- while the unflushed models keep them."""
    X = br.rows("randn", 8, 1024, 5)
    S = X.astype(np.float64) @ X.astype(np.float64).T
    s = {m: br.dots(X, X, m) for m in br.MODELS}
    assert not np.array_equal(s["sequential"], s["tree"]) and not np.array_equal(s["sequential"], s["truncate"])
    err = {m: np.abs(s[m].astype(np.float64) - S).max() for m in br.MODELS}
    assert err["truncate"] > err["tree"]
    T = br.rows("tiny", 4, 33, 6)
    assert not br.dots(T, T, "sequential", flush=True).any() and br.dots(T, T, "sequential", flush=False).any()
    # integer rows: every model is exact
    Z = br.to_bf16(np.random.default_rng(7).integers(-4, 5, (5, 40)))
    for m in br.MODELS:
        assert np.array_equal(br.dots(Z, Z, m, True).astype(np.float64), Z.astype(np.float64) @ Z.astype(np.float64).T)


def _rows(kind, n, F, seed):
    rng = np.random.default_rng(seed)
    if kind == "integer":  # many ties
        X = rng.integers(-2, 3, (n, F))
    elif kind == "duplicates":  # every row twice
        X = np.tile(rng.standard_normal((n // 2, F)), (2, 1))
    elif kind == "offset":  # bfloat16 spacing 0.5 at 100: ties at the shortlist's edge, severe cancellation
        X = 100.0 + rng.standard_normal((n, F))
    else:
        X = rng.standard_normal((n, F))
    return br.to_bf16(X)


@pytest.mark.parametrize("kind", ["integer", "duplicates", "offset", "randn"])
def test_adversarial_estimates_never_change_the_result(kind):
    """_knn_dot_ref.scheme and perturbed, under E1b: estimates moved by up to E1b against the true neighbours and at random
    return the exhaustive float32 selection; ties, duplicate rows and n <= kp included."""
    F = 6
    rng = np.random.default_rng(9)
    for n in (90, 30):  # 30 <= kp = 32
        X, Q = _rows(kind, n, F, 7), _rows(kind, 11, F, 8)
        for queries in (None, Q):
            Qa = X if queries is None else queries
            D64, D32 = kr.distances(Qa, X), dr.d2_f32(Qa, X)
            E1 = br.bound_bf16(Qa, X)
            assert (E1 > 0).all()
            for self_first in ((True, False) if queries is None else (False,)):
                for k, slack in ((1, 1), (3, 2), (3, None), (10, 5), (10, None), (30, None)):
                    want = dr.exhaustive(X, k, queries, self_first, D32=D32)
                    ref = kr.knn(X, k, queries=queries, self_first=self_first, D=D64)
                    top = np.zeros(D64.shape, bool)
                    top[np.arange(D64.shape[0])[:, None], ref[0]] = True
                    for mode in ("exclude", "random", "truth"):
                        est = D64 if mode == "truth" else dr.perturbed(D64, E1, top, mode, rng)
                        idx, dist, fb = br.scheme(X, k, est, queries, self_first, slack=slack, D32=D32)
                        what = (kind, n, queries is None, self_first, k, slack, mode)
                        assert np.array_equal(idx, want[0]), what
                        assert np.array_equal(dist.view(np.int32), want[1].view(np.int32)), what
                        if k + (dr.default_slack(k) if slack is None else slack) >= n:
                            assert not fb.any(), what


def test_the_scheme_runs_under_e1b_and_restores_the_float32_bound():
    X = _rows("randn", 40, 200, 3)
    assert not np.array_equal(br.bound_bf16(X, X), dr.bound(X, X))
    f32_bound = dr._bound
    with br._bf16_bound():
        assert dr._bound is br._bound_bf16 and np.array_equal(dr.bound(X, X), br.bound_bf16(X, X))
    assert dr._bound is f32_bound
    # E1b over E1 tends to (F + 34 F / 16) / (2 F) = 1.5625 on wide rows
    assert 1.5 < float((br.bound_bf16(X, X) / dr.bound(X, X)).max()) < 1.7


def test_the_device_tests_inputs_are_what_they_are_named():
    """The device test's fallback expectations come from here: randn 1000 x 64 in bfloat16, k = 10, is certified row by row
    whatever the estimates within E1b; identical rows with n > kp never are."""
    X = br.to_bf16(np.random.default_rng(1).standard_normal((1000, 64)))
    assert br.certifiable(None, X, 10) and not br.never_certifiable(None, X, 10)
    I = np.repeat(br.to_bf16(np.random.default_rng(2).standard_normal((1, 64))), 300, axis=0)
    assert br.never_certifiable(None, I, 10) and not br.certifiable(None, I, 10)
