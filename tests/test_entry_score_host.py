"""Per-incidence logits, the one-hop weighted gather and the dot-product layer without a device: the exported symbols, the
refusals of the C entries on a host-only plan, the refusals of ops.incidence_softmax(incidence_score=...), ops.incidence_gather,
ops.incidence_dot and HypergraphAttnConv(score=...), all decided before a device is touched, and the layer's parameters."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402

ENTRY_SYMBOLS = ("hg_incidence_attention_entry_heads_f32", "hg_incidence_attention_entry_heads_bwd_f32",
                 "hg_incidence_attention_entry_dropout_heads_f32", "hg_incidence_attention_entry_dropout_heads_bwd_f32",
                 "hg_gather_rows_incidence_heads_f32")


def _calls(L, some):
    """name -> call(plan, group_or_hop, heads, entry_score): every pointer but entry_score is null, F = 12."""
    null = ctypes.c_void_p()
    return {
        "entry": lambda p, g, h, t: L.hg_incidence_attention_entry_heads_f32(p, g, h, null, null, null, null, t, 0.2, null, null),
        "entry_bwd": lambda p, g, h, t: L.hg_incidence_attention_entry_heads_bwd_f32(
            p, g, h, null, null, null, null, t, 0.2, null, null, null, null, null, null),
        "entry_drop": lambda p, g, h, t: L.hg_incidence_attention_entry_dropout_heads_f32(
            p, g, h, null, null, null, null, t, 0.2, 0.5, some, null, null, null),
        "entry_drop_bwd": lambda p, g, h, t: L.hg_incidence_attention_entry_dropout_heads_bwd_f32(
            p, g, h, null, null, null, null, t, 0.2, 0.5, some, null, null, null, null, null, null),
        "gather": lambda p, g, h, t: L.hg_gather_rows_incidence_heads_f32(p, g, 12, h, null, null, null, t, null, null, null,
                                                                         null, 0, null),
    }


def test_exports(hg):
    from hypergef_amd import _lib
    from hypergef_amd.plan import Plan
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hg_aggr.h")).read()
    for name in ENTRY_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert "HG_API int %s(" % name in header, name
    assert L.hg_version() == 410
    assert hg.incidence_gather is hg.ops.incidence_gather and hg.incidence_dot is hg.ops.incidence_dot
    assert hasattr(Plan, "gather_rows_incidence")
    import inspect
    assert "incidence_score" in inspect.signature(hg.ops.incidence_softmax).parameters
    for m in ("incidence_attention", "incidence_attention_backward", "incidence_attention_dropout",
              "incidence_attention_dropout_backward"):
        assert "entry" in inspect.signature(getattr(Plan, m)).parameters, m


def test_every_softmax_form_has_its_exported_entry(hg):
    """The Plan picks the C entry of a form from a table of names: all eight exist, with their argument types declared."""
    from hypergef_amd import _lib, plan
    L = _lib.lib()
    names = plan._SOFTMAX_ENTRIES
    assert sorted(names) == [(e, d, b) for e in (False, True) for d in (False, True) for b in (False, True)]
    assert len(set(names.values())) == 8
    for (entry, dropout, bwd), name in names.items():
        assert name in _lib.SYMBOLS and getattr(L, name).argtypes is not None, name
        assert ("_entry_" in name, "_dropout_" in name, "_bwd_" in name) == (entry, dropout, bwd), name
        # plan, group, heads, the CSR pair, sv, se [, entry], slope [, p_drop, rng], the arrays (1 / 2 forward, 5 backward), stream
        assert len(getattr(L, name).argtypes) == 7 + entry + 1 + 2 * dropout + (5 if bwd else 1 + dropout) + 1, name


def test_c_entries_refuse_on_a_host_only_plan(hg):
    from hypergef_amd import _lib
    from hypergef_amd.plan import Plan, make_opts
    L = _lib.lib()
    inc = ar.toy()
    plan = Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True))
    buf = np.zeros(4 * inc.nnz, np.float32)  # a non-null host address: never read, every call is refused before
    some = ctypes.c_void_p(buf.ctypes.data)
    null = ctypes.c_void_p()
    calls = _calls(L, some)
    for name, call in calls.items():
        for side in (0, 1):
            for heads in (1, 4):
                assert call(plan._h, side, heads, some) == _lib.HG_ERR_UNSUPPORTED, (name, side, heads)
                assert b"HOST_ONLY" in L.hg_last_error(), name
        for heads in (0, -3):
            assert call(plan._h, 0, heads, some) == _lib.HG_ERR_INVALID, (name, heads)
            assert b"heads" in L.hg_last_error(), name
        for bad in (-1, 2, 7):  # group of the softmax entries, hop of the gather
            assert call(plan._h, bad, 1, some) == _lib.HG_ERR_INVALID, (name, bad)
            assert (b"hop" if name == "gather" else b"group") in L.hg_last_error(), name
        assert call(null, 0, 2, some) == _lib.HG_ERR_INVALID, name
    for name in ("entry", "entry_bwd", "entry_drop", "entry_drop_bwd"):
        assert calls[name](plan._h, 0, 1, null) == _lib.HG_ERR_INVALID, name
        assert b"entry_score" in L.hg_last_error(), name
    for heads in (5, 8):  # F = 12 is no multiple of 5 or 8
        assert calls["gather"](plan._h, 0, heads, some) == _lib.HG_ERR_INVALID
        assert b"multiple of heads" in L.hg_last_error()
    # the gather's weights are optional: without them the host-only refusal is still the answer
    assert calls["gather"](plan._h, 1, 3, null) == _lib.HG_ERR_UNSUPPORTED


def test_python_refusals_need_no_device(hg, monkeypatch):
    from hypergef_amd import ops
    monkeypatch.setattr(ops, "cached_plan", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device touched")))
    inc = ar.toy()
    N, M, nnz, H = inc.N, inc.M, inc.nnz, 3
    ptr, ind = torch.from_numpy(inc.csrptr), torch.from_numpy(inc.colind)
    sv, se, t = torch.zeros(N, H), torch.zeros(M, H), torch.zeros(nnz, H)
    # --- incidence_softmax(incidence_score=)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_softmax(ptr, ind, sv, se, heads=H, incidence_score=t.to(torch.bfloat16))
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_softmax(ptr, ind, None, None, num_nodes=N, incidence_score=t[:, 0].to(torch.bfloat16))
    for bad in (torch.zeros(nnz), torch.zeros(nnz, H + 1), torch.zeros(nnz * H - 1)):
        with pytest.raises(ValueError, match="incidence_score must have %d elements" % (nnz * H)):
            ops.incidence_softmax(ptr, ind, sv, se, heads=H, incidence_score=bad)
    with pytest.raises(ValueError, match="elements"):
        ops.incidence_softmax(ptr, ind, None, None, num_nodes=N, incidence_score=torch.zeros(nnz + 1))
    with pytest.raises(ValueError, match="num_nodes"):
        ops.incidence_softmax(ptr, ind, None, None, incidence_score=torch.zeros(nnz))
    with pytest.raises(ValueError, match="variant"):
        ops.incidence_softmax(ptr, ind, sv, se, heads=H, incidence_score=t, options=ops.Options(variant="fused"))
    with pytest.raises(ValueError, match="group"):
        ops.incidence_softmax(ptr, ind, sv, se, heads=H, incidence_score=t, group="edge")
    with pytest.raises(ValueError, match="heads"):
        ops.incidence_softmax(ptr, ind, sv, se, heads=0, incidence_score=t)
    # _segment_args' order: a wrong dtype is refused before a wrong length, a wrong length before the device
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_softmax(ptr, ind, sv, se[:-1], heads=H, incidence_score=t.to(torch.bfloat16))
    with pytest.raises(TypeError, match="rng_state"):
        ops.incidence_softmax(ptr, ind, sv, se, heads=H, incidence_score=t, dropout=0.5, rng_state=torch.zeros(2))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_softmax(ptr, ind, sv, se, heads=H, incidence_score=t)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_softmax(ptr, ind, None, None, num_nodes=N, incidence_score=torch.zeros(nnz), dropout=0.5,
                              rng_state=torch.zeros(2, dtype=torch.int64))
    # --- incidence_gather
    x, xe, w = torch.zeros(N, 2 * H), torch.zeros(M, 2 * H), torch.zeros(nnz, H)
    for variant in ("fused", "push_atomic", "push_groups"):
        with pytest.raises(ValueError, match="variant"):
            ops.incidence_gather(ptr, ind, x, w, heads=H, options=ops.Options(variant=variant))
    for bad in ("edge", "hyperedges", 0, None):
        with pytest.raises(ValueError, match="to must be"):
            ops.incidence_gather(ptr, ind, x, w, to=bad, heads=H)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="heads"):
            ops.incidence_gather(ptr, ind, x, w, heads=bad)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_gather(ptr, ind, x.to(torch.bfloat16), w, heads=H)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_gather(ptr, ind, x, w.to(torch.bfloat16), heads=H)
    with pytest.raises(ValueError, match="multiple of heads"):
        ops.incidence_gather(ptr, ind, torch.zeros(N, 2 * H + 1), w, heads=H)
    for bad in (torch.zeros(nnz), torch.zeros(nnz * H - 1)):
        with pytest.raises(ValueError, match="per incidence and head"):
            ops.incidence_gather(ptr, ind, x, bad, heads=H)
    with pytest.raises(ValueError, match="one weight per incidence \\("):
        ops.incidence_gather(ptr, ind, x, torch.zeros(nnz, 2))
    with pytest.raises(ValueError, match="hyperedges"):
        ops.incidence_gather(ptr, ind, x, w, to="vertex", heads=H, num_nodes=N)  # src must be [M, F] there
    with pytest.raises(ValueError, match="one factor per row"):
        ops.incidence_gather(ptr, ind, x, w, heads=H, scale_a=torch.zeros(M + 1))
    with pytest.raises(ValueError, match="one factor per row"):
        ops.incidence_gather(ptr, ind, xe, w, to="vertex", heads=H, num_nodes=N, scale_b=torch.zeros(M) if M != N else torch.zeros(N + 1))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_gather(ptr, ind, x, w, heads=H)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_gather(ptr, ind, xe, None, to="vertex", num_nodes=N)
    # --- incidence_dot
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_dot(ptr, ind, x.to(torch.bfloat16), xe)
    with pytest.raises(ValueError, match="heads"):
        ops.incidence_dot(ptr, ind, x, xe, heads=0)
    with pytest.raises(ValueError, match="A must be"):
        ops.incidence_dot(ptr, ind, x, xe[:-1])
    with pytest.raises(ValueError, match="A must be"):
        ops.incidence_dot(ptr, ind, x, torch.zeros(M, 2 * H + 1))
    with pytest.raises(ValueError, match="multiple of heads"):
        ops.incidence_dot(ptr, ind, x, xe, heads=4)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_dot(ptr, ind, x, xe, heads=H)


def test_plan_methods_refuse_before_any_tensor(hg):
    from hypergef_amd.plan import Plan, make_opts
    inc = ar.toy()
    plan = Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True))
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match="heads"):
            plan.gather_rows_incidence(0, None, None, None, heads=bad)
    for bad in (2, -1, "edge"):
        with pytest.raises(ValueError):
            plan.gather_rows_incidence(bad, None, None, None)


def test_layer_score_argument_and_parameters(hg):
    class _H:  # refused before the hypergraph is looked at
        pass
    for bad in ("mul", "Dot", None, 1):
        with pytest.raises(ValueError, match="score"):
            hg.HypergraphAttnConv(_H(), 4, 4, score=bad)
    inc = ar.toy()
    hyperg = hg.HyperGraph.from_incidence(inc, "cpu", data_name="toy")
    # additive: the layer as it is -- the same keys, values and use of torch's generator
    torch.manual_seed(5)
    plain = hg.HypergraphAttnConv(hyperg, 5, 3, group="vertex", heads=2)
    after_plain = torch.rand(1)
    torch.manual_seed(5)
    add = hg.HypergraphAttnConv(hyperg, 5, 3, group="vertex", heads=2, score="additive")
    after_add = torch.rand(1)
    a, b = plain.state_dict(), add.state_dict()
    assert list(a) == list(b) == ["a_v", "a_e", "bias", "lin.weight"]
    assert all(torch.equal(a[k], b[k]) for k in a) and torch.equal(after_plain, after_add)
    assert add.score == "additive" and not hasattr(add, "lin_k")
    # dot: two bias-free linears and the bias, nothing else
    for heads, concat in ((1, True), (4, True), (4, False)):
        dot = hg.HypergraphAttnConv(hyperg, 5, 3, heads=heads, concat=concat, score="dot")
        shapes = {n: tuple(p.shape) for n, p in dot.named_parameters()}
        assert shapes == {"lin.weight": (3 * heads, 5), "lin_k.weight": (3 * heads, 5),
                          "bias": (3 * heads if concat else 3,)}
        assert sorted(dot.state_dict()) == ["bias", "lin.weight", "lin_k.weight"]
        assert not list(dot.buffers()) and not hasattr(dot, "a_v") and not hasattr(dot, "a_e")
        assert isinstance(dot.lin_k, hg.ops.Linear) and dot.lin_k.bias is None and dot.score == "dot"
