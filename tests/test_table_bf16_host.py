"""bfloat16 rows over a neighbour table without a device: the exports, the default that still refuses, what
Options.incidence_bf16 = 'rows' lets through and what it does not, and the C entries' refusals in their order (every pointer
is host memory: nothing is launched)."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hg_table_gather_bf16", "hg_table_gather_t_bf16", "hg_table_dist_bf16", "hg_table_dot_bf16")
BF = torch.bfloat16


def test_exports(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "hg_aggr.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert "%s(" % name in header, name
    assert "THE CONTRACT" in header and "LONG ROWS" in header
    assert L.hg_version() == 410


def test_python_lets_bfloat16_rows_through_under_the_option_only(hg):
    ops = hg.ops
    idx = torch.zeros(6, 3, dtype=torch.int32)
    X, w = torch.zeros(6, 8), torch.zeros(18)
    rows = ops.current_options().replace(incidence_bf16="rows")
    for call in (lambda **kw: ops.knn_aggr(idx, X.to(BF), **kw), lambda **kw: ops.knn_dist(idx, X.to(BF), **kw),
                 lambda **kw: ops.knn_dist(idx, X.to(BF), queries=X.to(BF), **kw)):
        with pytest.raises(TypeError, match="float32"):  # the default stays
            call()
        with pytest.raises(RuntimeError, match="GPU"):
            call(options=rows)
        with ops.options(incidence_bf16="rows"), pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(TypeError, match="ops.Options"):
        ops.knn_aggr(idx, X, options="rows")
    # still TypeError under the option: a mixed pair, bfloat16 weights and scales, the other dtypes
    for kw in (dict(X=X.to(BF), queries=X), dict(X=X, queries=X.to(BF))):
        with pytest.raises(TypeError, match="float32"):
            ops.knn_dist(idx, options=rows, **kw)
    for kw in (dict(weight=w.to(BF)), dict(degE=torch.zeros(6, dtype=BF)), dict(degV=torch.zeros(6, dtype=BF))):
        with pytest.raises(TypeError, match="float32"):
            ops.knn_aggr(idx, X.to(BF), options=rows, **kw)
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            ops.knn_aggr(idx, X.to(dt), options=rows)
        with pytest.raises(TypeError, match="float32"):
            ops.knn_dist(idx, X.to(dt), options=rows)
        with pytest.raises(TypeError, match="float32"):
            ops.knn_dist(idx, X.to(BF), queries=X.to(dt), options=rows)


def test_c_refusals_before_any_device_call(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    rows, k, n, F = 4, 3, 4, 8
    idx = np.zeros((rows, k), np.int32)
    ptr, pos = np.zeros(n + 1, np.int32), np.zeros(rows * k, np.int32)
    pool = np.zeros(4 * rows * F * 4 + 64, np.uint8)
    base = -pool.ctypes.data % 16  # three 16-byte aligned row arrays, wide enough for either type
    src, ctr, dst = (pool[base + i * rows * F * 4:][:rows * F * 4] for i in range(3))
    out = np.zeros(rows * k, np.float32)
    null = ctypes.c_void_p()
    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED
    SRC, DST = _lib.HG_ROWS_SRC_BF16, _lib.HG_ROWS_DST_BF16

    def p(a, off=0):
        return null if a is None else ctypes.c_void_p(a.ctypes.data + off)

    def gather(i=idx, s=src, c=None, d=dst, r=rows, kk=k, nn=n, f=F, io=SRC, off=0):
        return L.hg_table_gather_bf16(p(i), r, kk, nn, f, p(s, off), null, null, null, p(c), p(d), io, null)

    def gather_t(i=ptr, s=src, c=None, d=dst, r=rows, kk=k, nn=n, f=F, io=SRC, off=0):
        return L.hg_table_gather_t_bf16(p(i), p(pos), r, kk, nn, f, p(s, off), null, null, null, p(c), p(d), io, null)

    def dist(i=idx, s=src, d=out, r=rows, kk=k, nn=n, f=F, off=0):
        return L.hg_table_dist_bf16(p(i), r, kk, nn, f, p(s, off), p(ctr), p(d), null)

    def dot(i=idx, s=src, d=out, r=rows, kk=k, nn=n, f=F, off=0):
        return L.hg_table_dot_bf16(p(i), r, kk, nn, f, p(s, off), null, p(ctr), null, null, p(d), null)

    for call in (gather, gather_t, dist, dot):
        assert call(i=None) == INV and b"null" in L.hg_last_error()
        assert call(s=None) == INV and call(d=None) == INV and b"null" in L.hg_last_error()
        assert call(s=None, f=0) == INV and b"null" in L.hg_last_error()  # the pointers before the sizes
        assert call(f=0) == INV and call(r=0) == INV and call(nn=0) == INV and b"at least 1" in L.hg_last_error()
        assert call(kk=65) == INV and b"k must be in 1 .. 64" in L.hg_last_error()
        assert call(r=2 ** 25, kk=64) == INV and b"2^31" in L.hg_last_error()
        assert call(f=12) == UNS and b"F % 8" in L.hg_last_error()
        assert call(off=8) == UNS and b"16-byte aligned rows" in L.hg_last_error()
        assert call(off=1) == UNS and b"2-byte aligned" in L.hg_last_error()
    for call in (gather, gather_t):
        for io in (0, 3, 4):
            assert call(io=io) == INV and b"io must be" in L.hg_last_error()
        assert call(io=0, kk=65) == INV and b"k must be" in L.hg_last_error()  # the sizes before io
        assert call(io=0, f=12) == INV  # io before the width
        assert call(c=ctr, io=DST) == INV and b"HG_ROWS_SRC_BF16 only" in L.hg_last_error()
        assert call(c=ctr, io=DST, f=12) == INV
    assert L.hg_table_dot_bf16(p(idx), rows, k, n, F, p(src), null, p(ctr), p(src), null, p(out), null) == INV
    assert b"both" in L.hg_last_error()
    assert not pool.any() and not out.any()
