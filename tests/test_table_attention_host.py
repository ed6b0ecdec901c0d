"""Fused attention aggregation over a neighbour table without a device: the exports, the C entries' refusals in their documented
order (host pointers: nothing is launched), ops.knn_attention_aggr's refusals in their order on CPU tensors, and the layer's flag."""
import ctypes

import numpy as np
import pytest
import torch

NEW = ("hg_table_attention_stats_heads_f32", "hg_table_attention_gather_heads_f32", "hg_table_attention_gather_t_heads_f32")
IDX = torch.zeros(6, 3, dtype=torch.int32)


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def test_exports_and_c_refusals(hg):
    from hypergef_amd import _lib, knn_graph
    L = _lib.lib()
    assert all(name in _lib.SYMBOLS and getattr(L, name).argtypes for name in NEW) and L.hg_version() == 410
    assert hg.knn_attention_aggr is hg.ops.knn_attention_aggr is knn_graph.knn_attention_aggr
    rows, k, n, F = 4, 3, 5, 8
    idx, ptr, pos = np.zeros((rows, k), np.int32), np.zeros(n + 1, np.int32), np.zeros(rows * k, np.int32)
    sc, m, inv, src, dst = (np.zeros(rows * F + 1, np.float32) for _ in range(5))
    null = ctypes.c_void_p()
    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED

    def p(x, off=0):
        return null if x is None else ctypes.c_void_p(x.ctypes.data + off)

    def stats(i=idx, s=sc, out=m, r=rows, kk=k, h=2, g=0, tp=ptr, off=0):
        return L.hg_table_attention_stats_heads_f32(p(i), r, kk, n, h, g, p(s), null, 0.2, p(tp), p(pos), p(out, off), p(inv), null)

    assert stats(i=None, out=None) == INV and b"null idx" in L.hg_last_error()
    assert stats(out=None, r=0) == INV and stats(s=None, kk=65) == INV and b"both null" in L.hg_last_error()  # pointers before sizes
    assert stats(g=1, tp=None, r=0) == INV and b"null ptr_v or pos_v" in L.hg_last_error()
    assert stats(kk=65, h=0) == INV and b"k must be in 1 .. 64" in L.hg_last_error()
    assert stats(h=0, g=7) == INV and b"heads must be at least 1" in L.hg_last_error()  # the heads before the enum
    assert stats(g=2, off=1) == INV and b"HG_TABLE_HYPEREDGE or HG_TABLE_VERTEX" in L.hg_last_error()  # the enum before alignment
    assert stats(off=1) == UNS and b"4-byte aligned" in L.hg_last_error()

    def hop1(i=idx, x=src, s=sc, mx=m, r=rows, kk=k, h=2, g=0, off=0, f=F):
        return L.hg_table_attention_gather_heads_f32(p(i), r, kk, n, f, h, g, p(x), p(s), null, 0.2, p(mx), p(inv), null, null,
                                                     p(dst, off), null)

    def hop2(i=idx, x=src, s=sc, mx=m, r=rows, kk=k, h=2, g=0, off=0, f=F):
        return L.hg_table_attention_gather_t_heads_f32(p(ptr), p(pos), p(i), r, kk, n, f, h, g, p(x), null, p(s), 0.2, p(mx), p(inv),
                                                       null, null, p(dst, off), null)

    for call in (hop1, hop2):
        assert call(i=None, x=None) == INV and b"null" in L.hg_last_error() and b"idx" in L.hg_last_error()
        assert call(x=None, r=0) == INV and b"null src or dst" in L.hg_last_error()  # pointers before sizes
        assert call(kk=65, h=0) == INV and b"k must be in 1 .. 64" in L.hg_last_error()
        assert call(h=0, f=7) == INV and b"heads must be at least 1" in L.hg_last_error()
        assert call(h=3, off=1) == INV and b"no multiple of heads" in L.hg_last_error()  # F % heads before alignment
        assert call(off=1, mx=None) == UNS and b"4-byte aligned" in L.hg_last_error()  # the heads gathers' set first
        assert call(mx=None, s=None) == INV and b"null seg_max or seg_inv" in L.hg_last_error()  # then the coefficients'
        assert call(s=None, g=7) == INV and b"both null" in L.hg_last_error()
        assert call(g=2) == INV and b"HG_TABLE_HYPEREDGE or HG_TABLE_VERTEX" in L.hg_last_error()
    assert not (m.any() or inv.any() or dst.any())


# every case carries a later refusal as well: the one named must come first
CALLS = [
    (dict(idx=IDX.long(), X=z(9, 8).double()), TypeError, "idx must be an int32"),
    (dict(X=z(9, 8, dtype=torch.bfloat16), node_score=z(9).double()), TypeError, "X must be a float32"),
    (dict(X=z(9, 8), node_score=z(9).double(), group="nowhere"), TypeError, "node_score must be a float32"),
    (dict(X=z(9, 8), node_score=z(9), degV=z(9).half(), group="nowhere"), TypeError, "degV must be a float32"),
    (dict(X=z(9, 8), node_score=z(9), transpose=(IDX, IDX.long()), group="nowhere"), TypeError, "pos_v must be an int32"),
    (dict(X=z(9, 8), node_score=z(9), group="nowhere", heads=0), ValueError, "group must be"),
    (dict(X=z(9, 8), node_score=z(9), heads=0), ValueError, "heads must be an integer >= 1"),
    (dict(idx=z(6, 65, dtype=torch.int32), X=z(9), node_score=z(9), heads=3), ValueError, "k must be in 1 .. 64"),
    (dict(X=z(9), heads=3), ValueError, "X must be"),
    (dict(X=z(9, 8), heads=3), ValueError, "no multiple of heads = 3"),
    (dict(X=z(9, 8), degE=z(5)), ValueError, "at least one of node_score and edge_score"),
    (dict(X=z(9, 8), node_score=z(9), edge_score=z(6), heads=2), ValueError, "node_score must be"),
    (dict(X=z(9, 8), node_score=z(9, 2), edge_score=z(5, 2), heads=2, degE=z(5)), ValueError, "edge_score must be"),
    (dict(X=z(9, 8), node_score=z(9), degE=z(5), degV=z(9).requires_grad_(True)), ValueError, "degE must be"),
    (dict(X=z(9, 8), node_score=z(9), transpose=(z(9, dtype=torch.int32), z(18, dtype=torch.int32))), ValueError, "transpose must be"),
    (dict(X=z(9, 8), node_score=z(9), degV=z(9, 1).requires_grad_(True)), RuntimeError, "degV gets no gradient"),
    (dict(X=z(9, 8), node_score=z(9, 2), edge_score=z(6, 2), heads=2, degE=z(6, 1)), RuntimeError, "idx must be on a GPU"),
]


@pytest.mark.parametrize("kw,error,text", CALLS)
def test_knn_attention_aggr_refuses_in_order(hg, kw, error, text):
    kw = dict(kw)
    with pytest.raises(error, match=text):
        hg.ops.knn_attention_aggr(kw.pop("idx", IDX), kw.pop("X"), **kw)


@pytest.mark.parametrize("kw,text", [(dict(fused_attention=True), "fused_attention=True needs attention="),
                                     (dict(fused_attention=True, attention="vertex", dropout=0.5), "fused_attention=False")])
def test_layer_flag_refusals_and_parameters(hg, kw, text):
    conv = hg.DynamicHypergraphConv
    with pytest.raises(ValueError, match=text):
        conv(8, 4, k=3, device_graph=True, **kw)
    torch.manual_seed(0)
    plain = conv(8, 4, k=3, device_graph=True, attention="vertex", heads=2)
    torch.manual_seed(0)
    fused = conv(8, 4, k=3, device_graph=True, attention="vertex", heads=2, fused_attention=True)
    assert list(plain.state_dict()) == list(fused.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), fused.state_dict().values()))
