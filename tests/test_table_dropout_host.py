"""Attention dropout over a neighbour table without a device: the exports, the two C entries' refusals in their order (host
pointers: nothing is launched or written) and those of ops.knn_softmax(dropout=) and DynamicHypergraphConv(dropout=)."""
import ctypes
import os

import numpy as np
import pytest
import torch

NEW = ("hg_table_softmax_dropout_heads_f32", "hg_table_softmax_dropout_bwd_heads_f32")


@pytest.mark.parametrize("bwd", [False, True])
def test_c_entry_is_declared_and_refuses_in_order(hg, bwd):
    from hypergef_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hg_aggr.h")).read()
    assert NEW[bwd] in _lib.SYMBOLS and hasattr(L, NEW[bwd]) and "HG_API int %s(" % NEW[bwd] in header and L.hg_version() == 410
    rows, k, n = 4, 3, 5
    idx, ptr, pos = np.zeros((rows, k), np.int32), np.zeros(n + 1, np.int32), np.zeros(rows * k, np.int32)
    sc, a, b, c = (np.zeros(rows * k + 2, np.float32) for _ in range(4))
    state = np.zeros(3, np.uint64)
    null = ctypes.c_void_p()
    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED

    def p(x, off=0):
        return null if x is None else ctypes.c_void_p(x.ctypes.data + off)

    def call(pd=0.5, st=state, soff=0, drop=b, r=rows, tp=ptr, g=0, off=0):  # drop: alpha_drop_out / ds; a: alpha_out / dout
        head = (p(idx), r, k, n, 1, g, null, p(sc), null, 0.2, pd, p(st, soff), p(tp), p(pos))
        return getattr(L, NEW[bwd])(*head, *((p(c), p(a, off), p(drop), null, null) if bwd else (p(a, off), p(drop), null)))

    # every call carries a later fault as well, and the earlier one must win: the null pointers before p_drop
    assert call(drop=None, pd=1.0) == INV and b"null" in L.hg_last_error() and b"p_drop" not in L.hg_last_error()
    assert call(g=1, tp=None, pd=1.0) == INV and b"null ptr_v or pos_v" in L.hg_last_error()
    for pd in (1.0, -0.25, float("nan")):  # p_drop before the state and the sizes
        assert call(pd=pd, st=None, r=0) == INV and b"p_drop must lie in [0, 1)" in L.hg_last_error(), pd
    assert call(st=None, r=0) == INV and b"rng_dev" in L.hg_last_error()  # the state before the sizes ..
    assert call(soff=4, g=7, off=1) == INV and b"rng_dev" in L.hg_last_error()  # .. the enum and the 4-byte alignment
    assert call(r=0, g=7) == INV and b"at least 1" in L.hg_last_error()  # from here the several-heads entries' order
    assert call(g=7, off=1) == INV and b"HG_TABLE_HYPEREDGE or HG_TABLE_VERTEX" in L.hg_last_error()
    assert call(off=1) == UNS and b"4-byte aligned" in L.hg_last_error()
    assert not (sc.any() or a.any() or b.any() or c.any())


z = torch.zeros


# CPU tensors; every case carries a later refusal as well: the one named must come first
@pytest.mark.parametrize("kw,error,text", [
    (dict(node_score=z(9, dtype=torch.bfloat16), dropout=1.0), ValueError, "infinite"),
    (dict(node_score=z(9, dtype=torch.bfloat16), dropout=True), ValueError, "dropout must be a real number"),
    (dict(node_score=z(9), group="nowhere", dropout=0.5, rng_state=z(2)), TypeError, "rng_state must be an int64"),
    (dict(node_score=z(9), dropout=0.5, rng_state=z(3, dtype=torch.int64)), ValueError, "rng_state must have 2 elements"),
    (dict(node_score=z(9), dropout=0.5, rng_state=z(2, dtype=torch.int64)), RuntimeError, "idx must be on a GPU"),
])
def test_knn_softmax_dropout_refuses_in_order(hg, kw, error, text):
    with pytest.raises(error, match=text):
        hg.ops.knn_softmax(torch.zeros(6, 3, dtype=torch.int32), **kw)


@pytest.mark.parametrize("kw,text", [(dict(dropout=0.5), "needs attention="), (dict(attention="vertex", dropout=1.0), "infinite")])
def test_layer_dropout_refusals(hg, kw, text):
    with pytest.raises(ValueError, match=text):
        hg.DynamicHypergraphConv(8, 4, k=3, device_graph=True, **kw)
