"""The fused attention aggregation (hg_aggr_incidence_attention_heads_f32 and its two companions), host side (no GPU):
declared, exported, and refusing what it cannot run -- in the order include/hg_aggr.h documents -- before a device is
touched; the operator's argument errors; the layer's fuse_attention switch adds no parameter."""
import os
import re

import pytest
import torch

from conftest import ROOT
from hypergef_amd import synth

SYMBOLS = ("hg_incidence_attention_stats_heads_f32", "hg_aggr_incidence_attention_heads_f32",
           "hg_gather_rows_attention_heads_f32")


def test_the_three_symbols_are_declared_and_exported(hg):
    from hypergef_amd import _lib
    header = open(os.path.join(ROOT, "include", "hg_aggr.h")).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"HG_API int %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name


def _host_plan():
    from hypergef_amd import plan as planmod
    inc = synth.cora_shape()
    return inc, planmod.Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, planmod.make_opts(host_only=True))


def _stats(L, plan, group=0, heads=1, ptr=1, ind=1, sv=8, se=8, slope=0.2, mx=16, inv=16):
    """hg_incidence_attention_stats_heads_f32 with made-up addresses (never dereferenced: every case is refused first)."""
    return L.hg_incidence_attention_stats_heads_f32(plan, group, heads, ptr, ind, sv, se, slope, mx, inv, None)


def _aggr(L, plan, F=32, heads=1, group=0, ptr=1, ind=1, X=16, sv=8, se=8, slope=0.2, mx=16, inv=16, Xe=None, Y=16,
          ws=256, nbytes=1 << 40):
    return L.hg_aggr_incidence_attention_heads_f32(plan, F, heads, group, ptr, ind, X, sv, se, slope, mx, inv, None, None,
                                                   None, Xe, Y, ws, nbytes, None)


def _hop(L, plan, hop=0, group=0, F=32, heads=1, ptr=1, ind=1, src=16, sv=8, se=8, slope=0.2, mx=16, inv=16, dst=16,
         ws=256, nbytes=1 << 40):
    return L.hg_gather_rows_attention_heads_f32(plan, hop, group, F, heads, ptr, ind, src, sv, se, slope, mx, inv, None,
                                                None, dst, ws, nbytes, None)


def test_refusal_order_of_the_stats_entry(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    _, plan = _host_plan()
    h = plan._h
    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED
    assert _stats(L, None, group=7, heads=0) == INV and b"null plan" in L.hg_last_error()
    assert _stats(L, h, group=2, heads=0, ptr=None) == INV and b"group" in L.hg_last_error()
    assert _stats(L, h, group=-1) == INV and b"group" in L.hg_last_error()
    assert _stats(L, h, heads=0, ptr=None) == INV and b"heads" in L.hg_last_error()
    for kw in (dict(ptr=None), dict(ind=None), dict(mx=None), dict(inv=None)):
        assert _stats(L, h, **kw) == INV, kw
        assert b"null array" in L.hg_last_error()
    assert _stats(L, h, slope=float("nan")) == INV and b"slope" in L.hg_last_error()
    # both scores may be absent: the call gets as far as the host-only plan
    for kw in (dict(), dict(sv=None), dict(se=None), dict(sv=None, se=None), dict(group=1, heads=8)):
        assert _stats(L, h, **kw) == UNS, kw
        assert b"HG_PLAN_HOST_ONLY" in L.hg_last_error()


@pytest.mark.parametrize("entry", ["two_hop", "one_hop"])
def test_refusal_order_of_the_gather_entries(hg, entry):
    from hypergef_amd import _lib
    L = _lib.lib()
    _, plan = _host_plan()
    h = plan._h
    INV, WS, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_WORKSPACE, _lib.HG_ERR_UNSUPPORTED
    call = _aggr if entry == "two_hop" else _hop
    data = "X" if entry == "two_hop" else "src"
    out = "Y" if entry == "two_hop" else "dst"
    # 1. INVALID, each decided before the ones after it
    assert call(L, None, group=5, heads=0, F=33) == INV and b"null plan" in L.hg_last_error()
    if entry == "one_hop":
        for hop in (-1, 2):
            assert call(L, h, hop=hop, group=5, heads=0) == INV and b"hop" in L.hg_last_error()
    for group in (-1, 2):
        assert call(L, h, group=group, heads=0, F=33) == INV and b"group" in L.hg_last_error()
    for heads in (0, -3):
        assert call(L, h, heads=heads, F=33, ptr=None) == INV and b"heads" in L.hg_last_error()
    for F, heads in ((33, 2), (6, 4), (0, 1), (-4, 2)):
        assert call(L, h, F=F, heads=heads, ptr=None, nbytes=0) == INV, (F, heads)
        assert b"multiple of heads" in L.hg_last_error()
    for kw in (dict(ptr=None), dict(ind=None), {data: None}, {out: None}, dict(mx=None), dict(inv=None)):
        assert call(L, h, nbytes=0, **kw) == INV, kw
        assert b"null array" in L.hg_last_error()
    # 2. the workspace, before the host-only plan is noticed
    need = L.hg_aggr_incidence_workspace_bytes(h, 32)
    assert need > 0
    for kw in (dict(nbytes=0), dict(nbytes=need - 1), dict(ws=None)):
        assert call(L, h, **kw) == WS, kw
        assert b"workspace too small" in L.hg_last_error()
    # 3. the host-only plan; neither score is required
    for kw in (dict(nbytes=need), dict(sv=None), dict(se=None), dict(sv=None, se=None), dict(F=64, heads=8, group=1)):
        assert call(L, h, **kw) == UNS, kw
        assert b"HG_PLAN_HOST_ONLY" in L.hg_last_error()


def test_operator_refuses_before_a_device_is_touched(hg):
    from hypergef_amd import ops
    inc = synth.cora_shape()
    ptr, ind = torch.from_numpy(inc.csrptr), torch.from_numpy(inc.colind)
    X, sv, se = torch.zeros(inc.N, 32), torch.zeros(inc.N), torch.zeros(inc.M)
    f = ops.incidence_attention_aggr
    for args in ((X.bfloat16(), sv, se), (X, sv.bfloat16(), se), (X, sv, se.bfloat16())):
        with pytest.raises(TypeError, match="no bfloat16 form"):
            f(ptr, ind, *args)
    with pytest.raises(ValueError, match="'hyperedge' or 'vertex'"):
        f(ptr, ind, X, sv, se, group="edge")
    for heads in (0, -1, 1.0, True):
        with pytest.raises(ValueError, match="heads must be an integer"):
            f(ptr, ind, X, sv, se, heads=heads)
    with pytest.raises(ValueError, match="no multiple of heads"):
        f(ptr, ind, torch.zeros(inc.N, 33), sv, se, heads=2)
    with pytest.raises(ValueError, match="node_score must have"):
        f(ptr, ind, X, sv[:-1], se)
    with pytest.raises(ValueError, match="edge_score must have"):
        f(ptr, ind, X, sv, torch.zeros(inc.M + 1))
    with pytest.raises(ValueError, match="node_score must have"):
        f(ptr, ind, X, sv, torch.zeros(inc.M, 4), heads=4)
    with pytest.raises(ValueError, match="num_nodes"):
        f(ptr, ind, X, sv, se, num_nodes=inc.N + 1)
    for variant in ("fused", "push_atomic", "push_groups"):
        with pytest.raises(ValueError, match="variant must be 'auto' or 'pull'"):
            f(ptr, ind, X, sv, se, options=ops.Options(variant=variant))
    # the variant is looked at first, the dtype before any length
    with pytest.raises(ValueError, match="variant"):
        f(ptr, ind, X.bfloat16(), sv, se, options=ops.Options(variant="fused"))
    with pytest.raises(TypeError, match="bfloat16"):
        f(ptr, ind, X.bfloat16(), sv[:-1], se)
    # everything the host can decide is in order: only now is the tensors' place looked at
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        f(ptr, ind, X, sv, se)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        f(ptr, ind, X, None, None, heads=8)


def test_plan_methods_exist(hg):
    from hypergef_amd.plan import Plan
    for name in ("incidence_attention_stats", "aggregate_incidence_attention", "gather_rows_attention"):
        assert callable(getattr(Plan, name)), name


@pytest.mark.parametrize("heads", [1, 4])
def test_fuse_attention_adds_no_parameter(hg, heads):
    import hypergef_amd as hgm
    hyperg = hgm.HyperGraph.from_incidence(synth.cora_shape(), "cpu")
    kw = dict(heads=heads, learn_hyperedge_weight=True)
    a = hgm.HypergraphAttnConv(hyperg, 8, 4, fuse_attention=False, **kw)
    b = hgm.HypergraphAttnConv(hyperg, 8, 4, fuse_attention=True, **kw)
    assert hgm.HypergraphAttnConv(hyperg, 8, 4, **kw).fuse_attention is False
    assert list(a.state_dict()) == list(b.state_dict())
    assert [tuple(t.shape) for t in a.state_dict().values()] == [tuple(t.shape) for t in b.state_dict().values()]
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    b.load_state_dict(a.state_dict())
