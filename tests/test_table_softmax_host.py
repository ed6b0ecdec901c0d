"""The attention softmax over a neighbour table without a device: the exports, the C entries' refusals in their order (host
pointers: nothing is launched, nothing written), ops.knn_softmax's refusals in their order, and the layer's."""
import ctypes

import numpy as np
import pytest
import torch

NEW = ("hg_table_softmax_f32", "hg_table_softmax_bwd_f32", "hg_table_sum_f32")


def test_exports_and_c_refusals(hg):
    from hypergef_amd import _lib, knn_graph
    L = _lib.lib()
    assert all(name in _lib.SYMBOLS and hasattr(L, name) for name in NEW) and L.hg_version() == 410
    assert hg.knn_softmax is hg.ops.knn_softmax is knn_graph.knn_softmax
    assert all(hasattr(knn_graph, name) for name in ("table_softmax", "table_softmax_bwd", "table_sum"))
    rows, k, n = 4, 3, 5
    idx, ptr, pos = np.zeros((rows, k), np.int32), np.zeros(n + 1, np.int32), np.zeros(rows * k, np.int32)
    sc, a, b, c = (np.zeros(rows * k + 1, np.float32) for _ in range(4))
    null = ctypes.c_void_p()
    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED

    def p(x, off=0):
        return null if x is None else ctypes.c_void_p(x.ctypes.data + off)

    def fwd(i=idx, s=sc, out=a, r=rows, kk=k, g=0, tp=ptr, off=0):
        return L.hg_table_softmax_f32(p(i), r, kk, n, g, p(s), null, null, 0.2, p(tp), p(pos), p(out, off), null)

    def bwd(i=idx, s=sc, out=a, r=rows, kk=k, g=0, tp=ptr, off=0):
        return L.hg_table_softmax_bwd_f32(p(i), r, kk, n, g, null, p(s), null, 0.2, p(tp), p(pos), p(b), p(c), p(out, off), null, null)

    def tsum(i=idx, s=sc, out=a, r=rows, kk=k, g=0, tp=ptr, off=0):
        return L.hg_table_sum_f32(p(i), r, kk, n, g, p(tp), p(pos), p(s), p(out, off), null)

    for call in (fwd, bwd, tsum):
        assert call(i=None, out=None) == INV and b"null idx" in L.hg_last_error()
        assert call(out=None, r=0) == INV and call(s=None, kk=65) == INV and b"null" in L.hg_last_error()  # pointers before sizes
        assert call(g=1, tp=None, r=0) == INV and b"null ptr_v or pos_v" in L.hg_last_error()
        assert call(g=0, tp=None, r=0) == INV and b"at least 1" in L.hg_last_error()  # the transpose: the vertex side's only
        assert call(kk=65, g=7) == INV and b"k must be in 1 .. 64" in L.hg_last_error()  # the sizes before the enum
        assert call(r=2 ** 25, kk=64) == INV and b"2^31" in L.hg_last_error()
        assert call(g=2, off=1) == INV and b"HG_TABLE_HYPEREDGE or HG_TABLE_VERTEX" in L.hg_last_error()  # the enum before alignment
        assert call(off=1) == UNS and call(g=1, off=2) == UNS and b"4-byte aligned" in L.hg_last_error()
    assert fwd(s=None) == INV and b"all null" in L.hg_last_error()  # no score at all
    assert not (sc.any() or a.any() or b.any() or c.any())


def test_knn_softmax_refuses_in_order(hg):
    f = hg.ops.knn_softmax
    idx, sv, se = torch.zeros(6, 3, dtype=torch.int32), torch.zeros(9), torch.zeros(6)
    tp = (torch.zeros(7, dtype=torch.int32), torch.zeros(18, dtype=torch.int32))
    with pytest.raises(TypeError, match="idx must be an int32"):
        f(idx.long(), sv.double(), group="nowhere")
    for bad in (sv.double(), sv.to(torch.bfloat16)):
        with pytest.raises(TypeError, match="node_score must be a float32"), hg.ops.options(incidence_bf16="rows"):
            f(idx, bad, group="nowhere")
    with pytest.raises(TypeError, match="entry_score must be a float32"):
        f(idx, sv, se, entry_score=torch.zeros(18).half(), group="nowhere")
    with pytest.raises(TypeError, match="ptr_v must be an int32"):
        f(idx, sv, transpose=(tp[0].long(), tp[1]), group="nowhere")
    with pytest.raises(ValueError, match="group must be 'hyperedge' or 'vertex'"):
        f(torch.zeros(6, 65, dtype=torch.int32), sv, group="nowhere")
    with pytest.raises(ValueError, match="k must be in 1 .. 64"):
        f(torch.zeros(6, 65, dtype=torch.int32))
    with pytest.raises(ValueError, match="at least one of node_score, edge_score and entry_score"):
        f(idx, num_nodes=0)
    with pytest.raises(ValueError, match=r"node_score must be \[n >= 1\]"):
        f(idx, sv[:, None], se[:5])
    with pytest.raises(ValueError, match="num_nodes"):
        f(idx, None, se, num_nodes=0)
    with pytest.raises(ValueError, match=r"edge_score must be \[rows\] = \[6\]"):
        f(idx, sv, se[:5], entry_score=torch.zeros(17))
    with pytest.raises(ValueError, match=r"entry_score must be \[rows, k\] = \[6, 3\] or \[rows \* k\] = \[18\]"):
        f(idx, sv, se, entry_score=torch.zeros(17), transpose=tp)
    with pytest.raises(ValueError, match=r"transpose must be \(ptr_v \[10\]"):
        f(idx, sv, se, transpose=tp)
    for group in ("hyperedge", "vertex"):
        with pytest.raises(RuntimeError, match="idx must be on a GPU"):
            f(idx, sv[:6].requires_grad_(True), se, group=group, entry_score=torch.zeros(6, 3), transpose=tp)


def test_layer_refusals_and_defaults(hg):
    conv = hg.DynamicHypergraphConv
    for kw, text in ((dict(), "needs device_graph=True"), (dict(device_graph=True, second_aggr="max"), "needs first_aggr = second_aggr"),
                     (dict(device_graph=True, probabilistic=True), "needs probabilistic=False")):
        with pytest.raises(ValueError, match=text):
            conv(8, 8, k=3, attention="vertex", **kw)
    with pytest.raises(ValueError, match="attention must be None, 'hyperedge' or 'vertex'"):
        conv(8, 8, k=3, device_graph=True, attention="edge")
    plain = conv(8, 8, k=3, device_graph=True)
    assert plain.attention is None and not hasattr(plain, "a_v") and list(plain.state_dict()) == ["lin.weight"]
    layer = conv(8, 8, k=3, device_graph=True, attention="hyperedge")
    assert sorted(layer.state_dict()) == ["a_e", "a_v", "lin.weight"] and layer.a_v.shape == (8,) and layer.negative_slope == 0.2
    with pytest.raises(TypeError, match="float32 rows"):
        layer.to(torch.bfloat16)(torch.zeros(9, 8, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="exclude each other"):
        hg.KnnHypergraph.aggregate(None, None, probabilistic=True, weight=torch.ones(3))
