"""ops.knn(form="dot_split") without a device: the exports, the C entry's refusals and workspace against hg_knn_dot_f32's, what
Python refuses before a device is touched, and the bound E1s against a numpy model of the split and of the estimate under
three models of the bf16 matrix unit's accumulation (tests/_knn_split_ref.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_bf16_ref as br  # noqa: E402
import _knn_split_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hg_knn_dot_split_f32", "hg_knn_dot_estimates_split_f32")


def test_exports(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "hg_aggr.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert "%s(" % name in header, name
    assert "E1s" in header and "dot_split" in hg.knn_graph.FORMS
    assert L.hg_version() == 410


def test_c_entry_refuses_what_the_float32_dot_entry_refuses(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    n, F = 10, 4
    X, Q = np.zeros((n, F), np.float32), np.zeros((3, F), np.float32)
    idx, dist = np.zeros((n, 64), np.int32), np.zeros((n, 64), np.float32)
    ws = np.zeros(1 << 16, np.uint8)
    null = ctypes.c_void_p()

    def p(a, off=0):
        return ctypes.c_void_p(a.ctypes.data + off)

    def call(entry, k=3, q=None, nq=n, self_first=0, slices=1, workspace=ws, F=F, x_off=0, idx_off=0):
        st = entry(p(X if q is None else q, x_off if q is None else 0), nq, p(X, x_off), n, F, k, self_first, slices, p(idx, idx_off),
                   p(dist), null, null, null if workspace is None else p(workspace), 0 if workspace is None else workspace.nbytes, null)
        return st, L.hg_last_error().split(b": ", 1)[-1]  # the text after the entry's name

    cases = [dict(k=0), dict(k=65), dict(k=11), dict(F=65537), dict(F=0), dict(q=Q, nq=3, self_first=1), dict(slices=-1),
             dict(k=0, slices=33), dict(slices=33), dict(x_off=2), dict(idx_off=2), dict(workspace=None),
             dict(workspace=np.zeros(8, np.uint8)), dict(F=65537, slices=33, workspace=None)]
    for kw in cases:
        got, want = call(L.hg_knn_dot_split_f32, **kw), call(L.hg_knn_dot_f32, **kw)
        assert got == want and got[0] != _lib.HG_OK, (kw, got, want)
    assert call(L.hg_knn_dot_split_f32, k=0)[0] == _lib.HG_ERR_INVALID and b"hg_knn_dot_split_f32: k must be" in L.hg_last_error()
    assert call(L.hg_knn_dot_split_f32, workspace=None)[0] == _lib.HG_ERR_WORKSPACE
    assert b"hg_knn_dot_workspace_bytes asks for %d" % L.hg_knn_dot_workspace_bytes(n, n, F, 3, 1) in L.hg_last_error()
    assert not idx.any() and not dist.any() and not ws.any()
    # the diagnostic entry: hg_knn_dot_estimates_bf16's refusals on float rows
    est, e1 = np.zeros((n, n), np.float32), np.zeros(n, np.float32)

    def diag(nq=n, n_=n, F=F, x_off=0, e=est):
        return L.hg_knn_dot_estimates_split_f32(p(X, x_off), nq, p(X, x_off), n_, F, null if e is None else p(e), p(e1), null)

    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED
    assert diag(e=None) == INV and b"hg_knn_dot_estimates_split_f32: null" in L.hg_last_error()
    assert diag(nq=0) == INV and diag(F=0) == INV
    assert diag(F=65537) == INV and b"above 65536" in L.hg_last_error()
    assert diag(nq=2049, n_=2048) == UNS and b"diagnostic" in L.hg_last_error()
    assert diag(x_off=2) == UNS and b"4-byte aligned" in L.hg_last_error()
    assert not est.any() and not e1.any()


def test_python_refusals_fire_without_a_device(hg):
    knn = hg.ops.knn
    x, q = torch.zeros(10, 4), torch.zeros(3, 4)
    for kw in (dict(), dict(queries=q), dict(return_mean=True, return_fallback=True, cand_slices=3), dict(self_first=False)):
        with pytest.raises(RuntimeError, match="GPU"):  # the form gets as far as the device
            knn(x, 3, form="dot_split", **kw)
    # in order: the dtype before the form, k before the form's own
    for t in (x.bfloat16(), x.half(), x.double()):
        with pytest.raises(TypeError, match="float32"):
            knn(t, 0, form="dot_split", segments=[0, 5, 10])
    with pytest.raises(TypeError, match="float32"):
        knn(x, 3, queries=q.bfloat16(), form="dot_split")
    with pytest.raises(ValueError, match="k must be"):
        knn(x, 0, segments=[0, 5, 10], form="dot_split")
    with pytest.raises(ValueError, match='form="dot_split" cannot be combined with segments'):
        knn(x, 3, segments=[0, 5, 10], set_rows=5, form="dot_split")
    with pytest.raises(ValueError, match='form="dot_split" cannot be combined with set_rows'):
        knn(torch.zeros(10, 65537), 3, set_rows=5, form="dot_split")
    with pytest.raises(ValueError, match='form="dot_split" takes rows of at most 65536 columns'):
        knn(torch.zeros(2, 65537), 1, form="dot_split", cand_slices=99)
    with pytest.raises(ValueError, match="cand_slices"):
        knn(x, 3, form="dot_split", cand_slices=33)
    # passed on unchanged by the layers
    with pytest.raises(RuntimeError, match="GPU"):
        hg.HyperGraph.from_knn(x, 3, "cpu", form="dot_split")
    with pytest.raises(RuntimeError, match="GPU"):
        hg.KnnHypergraph.build(x, 3, form="dot_split")
    with pytest.raises(ValueError, match="cannot be combined with set_rows"):
        hg.KnnHypergraph.build(x, 3, form="dot_split", set_rows=5)
    for device_graph in (False, True):
        with pytest.raises(RuntimeError, match="GPU"):
            hg.DynamicHypergraphConv(4, 4, 3, device_graph=device_graph, knn_form="dot_split")(x)


def test_the_split_is_two_roundings_and_leaves_a_remainder_below_two_to_the_minus_sixteen():
    x = sr.rows("full24", 8, 64, 1)
    hi, lo = sr.split(x)
    assert np.array_equal(hi, br.to_bf16(hi)) and np.array_equal(lo, br.to_bf16(lo))
    rem = x.astype(np.float64) - hi - lo
    assert rem.any() and (np.abs(rem) <= 2.0 ** -16 * np.abs(x)).all()
    assert (np.abs(lo) <= 2.0 ** -8 * (1 + 2.0 ** -8) * np.abs(x)).all()


@pytest.mark.parametrize("kind", sr.KINDS)
def test_bound_holds_under_every_model_of_the_accumulation(kind):
    """|d~ - d2_f64| <= E1s for d~ formed as the kernels form it, the instruction emulated three ways, each with and without
    flushing subnormal parts, products and partial sums: nothing is tuned to the result, E1s is hg_aggr.h's."""
    worst = 0.0
    for F in sr.WIDTHS:
        X, Q = sr.rows(kind, 12, F, 100 + F), sr.rows(kind, 6, F, 200 + F)
        D64 = br.distances(Q, X)
        E1 = sr.bound_split(Q, X).astype(np.float64)
        assert np.isfinite(E1).all() and (E1 > 0).all()
        for model in br.MODELS:
            for flush in (False, True):
                err = np.abs(sr.estimates(Q, X, model, flush).astype(np.float64) - D64)
                worst = max(worst, float((err / E1[:, None]).max()))
                assert (err <= E1[:, None]).all(), (kind, F, model, flush, float((err / E1[:, None]).max()))
    print("%s: max |d~ - d2| / E1s = %.3g" % (kind, worst))
