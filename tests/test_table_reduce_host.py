"""Max, min and mean over a neighbour table without a device: the exports, ops.knn_gather's and knn_aggr(first=, second=)'s
refusals in their order, the C entries' refusals (host pointers: nothing is launched), and the defaults that stay."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

NEW = ("hg_table_reduce_f32", "hg_table_reduce_t_f32", "hg_table_select_f32", "hg_table_select_t_f32")


def test_exports_and_c_refusals(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    assert all(name in _lib.SYMBOLS and hasattr(L, name) for name in NEW) and L.hg_version() == 410
    assert hg.knn_gather is hg.ops.knn_gather
    rows, k, n, F = 4, 3, 4, 8
    idx, ptr, pos = np.zeros((rows, k), np.int32), np.zeros(n + 1, np.int32), np.zeros(rows * k, np.int32)
    a, b, c = (np.zeros(rows * F + 1, np.float32) for _ in range(3))
    null = ctypes.c_void_p()
    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED

    def p(x, off=0):
        return null if x is None else ctypes.c_void_p(x.ctypes.data + off)

    def reduce(i=idx, s=a, d=b, g=c, r=rows, kk=k, f=F, op=1, off=0):
        return L.hg_table_reduce_f32(p(i), r, kk, n, f, op, p(s, off), null, p(d), p(g), null)

    def reduce_t(i=ptr, s=a, d=b, g=c, r=rows, kk=k, f=F, op=2, off=0):
        return L.hg_table_reduce_t_f32(p(i), p(pos), r, kk, n, f, op, p(s, off), null, p(d), p(g), null)

    def select(i=idx, s=a, d=b, g=c, r=rows, kk=k, f=F, op=None, off=0):
        return L.hg_table_select_f32(p(i), r, kk, n, f, p(s, off), p(g), p(d), null)

    def select_t(i=ptr, s=a, d=b, g=c, r=rows, kk=k, f=F, op=None, off=0):
        return L.hg_table_select_t_f32(p(i), p(pos), r, kk, n, f, p(s, off), p(g), p(d), null)

    for call in (reduce, reduce_t, select, select_t):
        assert call(i=None) == INV and b"null" in L.hg_last_error()
        assert call(s=None, f=0) == INV and call(d=None) == INV and b"null" in L.hg_last_error()  # the pointers before the sizes
        assert call(f=0) == INV and call(r=0) == INV and b"at least 1" in L.hg_last_error()
        assert call(kk=65) == INV and b"k must be in 1 .. 64" in L.hg_last_error()
        assert call(r=2 ** 25, kk=64) == INV and b"2^31" in L.hg_last_error()
        assert call(off=1) == UNS and b"4-byte aligned" in L.hg_last_error()
    for call in (select, select_t):
        assert call(g=None) == INV and b"null gs, arg or dsrc" in L.hg_last_error()
    for call in (reduce, reduce_t):
        assert call(op=0) == INV and call(op=3) == INV and b"HG_REDUCE_MAX or HG_REDUCE_MIN" in L.hg_last_error()
        assert call(op=0, kk=65) == INV and b"k must be" in L.hg_last_error()  # the sizes before the op
        assert call(op=0, off=1) == INV  # the op before the alignment
    assert not (a.any() or b.any() or c.any())


def test_knn_gather_refuses_in_order(hg):
    g = hg.ops.knn_gather
    idx, src, sc = torch.zeros(6, 3, dtype=torch.int32), torch.zeros(6, 8), torch.ones(6)
    tp = (torch.zeros(7, dtype=torch.int32), torch.zeros(18, dtype=torch.int32))
    with pytest.raises(TypeError, match="idx must be an int32"):
        g(idx.long(), src.double(), to="nowhere")
    for bad in (src.double(), src.to(torch.bfloat16)):
        with pytest.raises(TypeError, match="src must be a float32"), hg.ops.options(incidence_bf16="rows"):
            g(idx, bad, reduce="median")
    with pytest.raises(TypeError, match="scale must be a float32"):
        g(idx, src, scale=sc.double(), to="nowhere")
    with pytest.raises(TypeError, match="ptr_v must be an int32"):
        g(idx, src, transpose=(tp[0].long(), tp[1]), to="nowhere")
    with pytest.raises(ValueError, match="to must be 'hyperedge' or 'vertex'"):
        g(idx, src, to="nowhere", reduce="median")
    with pytest.raises(ValueError, match="reduce must be one of 'sum', 'mean', 'max', 'min'"):
        g(idx, src[:, :0], reduce="median")
    with pytest.raises(ValueError, match="k must be in 1 .. 64"):
        g(torch.zeros(6, 65, dtype=torch.int32), src)
    with pytest.raises(ValueError, match=r"src must be \[n >= 1, F >= 1\]"):
        g(idx, src[:, :0], return_index=True)
    with pytest.raises(ValueError, match="one row of src per row of idx"):
        g(idx, src[:5], to="vertex")
    with pytest.raises(ValueError, match="num_nodes"):
        g(idx, src, to="vertex", num_nodes=0)
    with pytest.raises(ValueError, match=r"scale must be \[9\] or \[9, 1\]"):
        g(idx, src, to="vertex", num_nodes=9, scale=sc)
    with pytest.raises(ValueError, match=r"transpose must be \(ptr_v \[10\]"):
        g(idx, src, to="vertex", num_nodes=9, transpose=tp)
    for r in ("sum", "mean"):
        with pytest.raises(ValueError, match="return_index needs reduce='max' or 'min'"):
            g(idx, src, reduce=r, return_index=True, scale=sc.requires_grad_(True))
    with pytest.raises(RuntimeError, match="scale gets no gradient from knn_gather"):
        g(idx, src, reduce="max", scale=sc)
    for r in ("sum", "mean", "max", "min"):
        with pytest.raises(RuntimeError, match="idx must be on a GPU"):
            g(idx, src, reduce=r, scale=sc.detach(), transpose=tp)


def test_knn_aggr_and_layer_refusals_and_defaults(hg):
    ops = hg.ops
    idx, X, w = torch.zeros(6, 3, dtype=torch.int32), torch.zeros(6, 8), torch.ones(18)
    names = list(inspect.signature(ops.knn_aggr).parameters)
    assert names == ["idx", "X", "weight", "degE", "degV", "transpose", "weight_grad", "options", "first", "second"]
    rows = ops.current_options().replace(incidence_bf16="rows")
    with pytest.raises(TypeError, match="no bfloat16 form"):
        ops.knn_aggr(idx, X.to(torch.bfloat16), weight=w, first="max", options=rows)
    with pytest.raises(ValueError, match="second must be one of"):
        ops.knn_aggr(idx, X, weight=w, second="median")
    with pytest.raises(ValueError, match="take no weight"):
        ops.knn_aggr(idx, X, weight=w, first="max")
    with pytest.raises(RuntimeError, match="degE gets no gradient from knn_aggr"):
        ops.knn_aggr(idx, X, degE=torch.ones(6, requires_grad=True), second="mean")
    for kw in (dict(first="max"), dict(second="min"), dict(first="mean", second="mean"), dict(), dict(first="sum", second="sum")):
        with pytest.raises(RuntimeError, match="idx must be on a GPU"):
            ops.knn_aggr(idx, X, **kw)
    assert [p.default for p in list(inspect.signature(hg.KnnHypergraph.aggregate).parameters.values())[-2:]] == ["sum", "sum"]
    layer = hg.DynamicHypergraphConv(8, 8, k=3)
    assert (layer.first_aggr, layer.second_aggr, layer.device_graph, layer.probabilistic) == ("sum", "sum", False, False)
    assert [n for n, _ in layer.named_parameters()] == ["lin.weight"]
    assert hg.DynamicHypergraphConv(8, 8, 3, True, None, 1.0, None, True, "dot", True).learn_distances  # the old positions
    with pytest.raises(ValueError, match="first_aggr must be"):
        hg.DynamicHypergraphConv(8, 8, k=3, first_aggr="median")
    for dg in (False, True):
        with pytest.raises(ValueError, match="probabilistic=True needs"):
            hg.DynamicHypergraphConv(8, 8, k=3, probabilistic=True, second_aggr="max", device_graph=dg)
