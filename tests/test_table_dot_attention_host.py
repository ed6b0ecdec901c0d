"""Dot-product attention over a neighbour table without a device: the exports, the C entries' refusals in their documented order
(host pointers: nothing is launched), ops.knn_dot_attention_aggr's refusals in their order on CPU tensors, and the layer's option."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

NEW = ("hg_table_dot_attention_f32", "hg_table_dot_attention_bwd_f32", "hg_table_dot_attention_gather_t_f32")
IDX = torch.zeros(6, 3, dtype=torch.int32)


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def test_exports_and_c_refusals(hg):
    from hypergef_amd import _lib, knn_graph
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hg_aggr.h")).read()
    assert all(re.search(r"HG_API int %s\(" % name, header) and name in _lib.SYMBOLS and getattr(L, name).argtypes for name in NEW)
    assert L.hg_version() == 410
    assert hg.knn_dot_attention_aggr is hg.ops.knn_dot_attention_aggr is knn_graph.knn_dot_attention_aggr
    rows, k, n, F = 4, 3, 5, 8
    idx = np.zeros((rows, k), np.int32)
    q, x, al, dd, dst, ds = (np.zeros(rows * 1024 + 1, np.float32) for _ in range(6))
    null = ctypes.c_void_p()
    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED

    def p(a, off=0):
        return null if a is None else ctypes.c_void_p(a.ctypes.data + off)

    def fwd(i=idx, src=x, r=rows, kk=k, f=F, h=2, off=0):
        return L.hg_table_dot_attention_f32(p(i), r, kk, n, f, h, p(q), p(src), 0.5, 0.2, null, p(dst, off), null, null)

    def bwd(i=idx, src=x, r=rows, kk=k, f=F, h=2, off=0):
        return L.hg_table_dot_attention_bwd_f32(p(i), r, kk, n, f, h, p(q), p(src), 0.5, 0.2, null, p(al), p(dd), null,
                                                p(dst, off), p(ds), null)

    def hop1(i=idx, src=x, r=rows, kk=k, f=F, h=2, off=0, s2=None):
        return L.hg_table_dot_attention_gather_t_f32(p(i), p(i), r, kk, n, f, h, p(src), p(al), null, p(s2), null, null, p(dst, off), null)

    assert hop1(src=None, s2=q) == INV and b"null src, w or dst" in L.hg_last_error()
    assert hop1(s2=q, r=0) == INV and b"both be given" in L.hg_last_error()
    for call in (fwd, bwd, hop1):
        assert call(i=None, src=None) == INV and (b"null idx" in L.hg_last_error() or b"null ptr_v" in L.hg_last_error())
        assert call(src=None, r=0) == INV and b"src" in L.hg_last_error() and b"null" in L.hg_last_error()  # pointers before sizes
        assert call(r=0, kk=65) == INV and b"at least 1" in L.hg_last_error()
        assert call(kk=65, h=0) == INV and b"k must be in 1 .. 64" in L.hg_last_error()
        assert call(h=0, f=7) == INV and b"heads must be at least 1" in L.hg_last_error()
        assert call(h=3, f=1024) == INV and b"no multiple of heads" in L.hg_last_error()  # F % heads before the width
        assert call(f=1024, off=1) == UNS and b"above 256" in L.hg_last_error()           # the width before alignment
        assert call(off=1) == UNS and b"4-byte aligned" in L.hg_last_error()
    assert not (dst.any() or ds.any())


# every case carries a later refusal as well: the one named must come first
CALLS = [
    (dict(idx=IDX.long(), X=z(9, 8).double()), TypeError, "idx must be an int32"),
    (dict(X=z(9, 8, dtype=torch.bfloat16), query=z(6, 8).double()), TypeError, "X must be a float32"),
    (dict(X=z(9, 8), query=z(6, 8).double(), heads=0), TypeError, "query must be a float32"),
    (dict(X=z(9, 8), degV=z(9).half(), heads=0), TypeError, "degV must be a float32"),
    (dict(X=z(9, 8), scale="1", heads=0), TypeError, "scale must be None or a number"),
    (dict(X=z(9, 8), transpose=(IDX, IDX.long()), heads=0), TypeError, "pos_v must be an int32"),
    (dict(idx=z(6, 65, dtype=torch.int32), X=z(9), heads=0), ValueError, "heads must be an integer >= 1"),
    (dict(idx=z(6, 65, dtype=torch.int32), X=z(9), heads=3), ValueError, "k must be in 1 .. 64"),
    (dict(X=z(9), heads=3), ValueError, "X must be"),
    (dict(X=z(9, 8), heads=3, query=z(5, 8)), ValueError, "no multiple of heads = 3"),
    (dict(X=z(9, 600), heads=2, query=z(5, 8)), ValueError, "above 256"),
    (dict(X=z(9, 8), query=z(5, 8), degE=z(5)), ValueError, "query must be \\[rows, F\\]"),
    (dict(X=z(9, 8), degE=z(5), degV=z(9).requires_grad_(True)), ValueError, "degE must be"),
    (dict(X=z(9, 8), transpose=(z(9, dtype=torch.int32), z(18, dtype=torch.int32)), scale=z(1).requires_grad_(True)),
     ValueError, "transpose must be"),
    (dict(X=z(9, 8), scale=z(1).requires_grad_(True), degV=z(9, 1).requires_grad_(True)), RuntimeError, "scale gets no gradient"),
    (dict(X=z(9, 8), degV=z(9, 1).requires_grad_(True)), RuntimeError, "degV gets no gradient"),
    (dict(X=z(9, 8), heads=2, degE=z(6, 1)), RuntimeError, "idx must be on a GPU"),
]


@pytest.mark.parametrize("kw,error,text", CALLS)
def test_knn_dot_attention_aggr_refuses_in_order(hg, kw, error, text):
    kw = dict(kw)
    X = kw.pop("X")
    query = kw.pop("query", z(6, X.shape[1]) if X.dim() == 2 else z(6, 8))
    with pytest.raises(error, match=text):
        hg.ops.knn_dot_attention_aggr(kw.pop("idx", IDX), X, query, **kw)


@pytest.mark.parametrize("kw,text", [(dict(attention="vertex"), "hyperedge group"),
                                     (dict(attention="hyperedge", device_graph=False), "device_graph=True"),
                                     (dict(attention="hyperedge", dropout=0.5), "no attention dropout"),
                                     (dict(attention="hyperedge", fused_attention=True), "fused_attention=False")])
def test_layer_option_refusals(hg, kw, text):
    with pytest.raises(ValueError, match=text):
        hg.DynamicHypergraphConv(8, 4, k=3, **dict(dict(device_graph=True, score="dot"), **kw))


def test_layer_parameters_and_the_positional_call(hg):
    conv = hg.DynamicHypergraphConv
    dot = conv(8, 4, k=3, device_graph=True, attention="hyperedge", heads=2, score="dot")
    assert sorted(dot.state_dict()) == ["lin.weight", "lin_k.weight"] and tuple(dot.lin_k.weight.shape) == (8, 8)
    torch.manual_seed(0)
    old = conv(8, 4, k=3, device_graph=True, attention="hyperedge", heads=2)
    torch.manual_seed(0)
    new = conv(8, 4, k=3, device_graph=True, attention="hyperedge", heads=2, score="additive")
    assert sorted(old.state_dict()) == sorted(new.state_dict()) == ["a_e", "a_v", "lin.weight"]
    assert all(torch.equal(a, b) for a, b in zip(old.state_dict().values(), new.state_dict().values()))
    with pytest.raises(ValueError, match="score must be"):
        conv(8, 4, k=3, score="cosine")
    # tests/test_table_reduce_host.py's positional call: the first ten parameters keep their places
    layer = conv(8, 4, 3, False, None, 1.0, None, True, "difference", False)
    assert layer.device_graph and layer.score == "additive" and sorted(layer.state_dict()) == ["lin.weight"]
