"""CPU-only checks of the multi-head incidence path: the float64 reference of tests/_heads_ref.py against gradcheck and against
the single-head references it is built on, the operators' argument errors (raised before a device is touched), the exported
symbols, the C entries' refusals on host-only plans, and the layer's parameters with heads."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402
import _grad_ref as gr  # noqa: E402
import _heads_ref as hr  # noqa: E402
import _incidence_ref as ir  # noqa: E402

HEADS_SYMBOLS = ("hg_incidence_attention_heads_f32", "hg_incidence_attention_heads_bwd_f32", "hg_incidence_sum_heads_f32",
                 "hg_aggr_incidence_heads_f32", "hg_incidence_dot_heads_f32")


def _graph(inc):
    degE = torch.from_numpy(np.diff(inc.csrptr).astype(np.float32)).pow(-1)
    degV = torch.rand(inc.N, generator=torch.Generator().manual_seed(1)) + 0.5
    return gr.Graph(inc, degE, degV, None)


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("group", ar.GROUPS)
def test_reference_passes_gradcheck(group, heads):
    inc = ar.toy()
    graph = _graph(inc)
    C = 2
    sv, se = _rand(inc.N, heads, seed=2).requires_grad_(True), _rand(inc.M, heads, seed=3).requires_grad_(True)
    for slope in (0.2, 1.0):
        assert torch.autograd.gradcheck(lambda a, b: hr.softmax(graph, a, b, group, slope, heads), (sv, se))
    val = _rand(inc.nnz, heads, seed=4).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: hr.segment_sum(graph, v, group), (val,))
    x = _rand(inc.N, heads * C, seed=5).requires_grad_(True)
    v2e, e2v = _rand(inc.nnz, heads, seed=6).requires_grad_(True), _rand(inc.nnz, heads, seed=7).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b, c: hr.incidence_aggr(graph, a, b, c, heads), (x, v2e, e2v))
    w = _rand(heads * C, 3, seed=8).requires_grad_(True)
    a_v, a_e = _rand(heads * C, seed=9).requires_grad_(True), _rand(heads * C, seed=10).requires_grad_(True)
    x3 = _rand(inc.N, 3, seed=11)
    for concat in (True, False):
        bias = _rand(heads * C if concat else C, seed=12).requires_grad_(True)
        assert torch.autograd.gradcheck(
            lambda ww, av, ae, b: hr.attn_conv(graph, x3, ww, av, ae, b, group, 0.2, heads, concat), (w, a_v, a_e, bias))


@pytest.mark.parametrize("group", ar.GROUPS)
def test_closed_form_backward_and_dot_equal_autograd(group):
    inc = ar.toy()
    graph = _graph(inc)
    H, C = 3, 2
    sv, se = _rand(inc.N, H, seed=2).requires_grad_(True), _rand(inc.M, H, seed=3).requires_grad_(True)
    dalpha = _rand(inc.nnz, H, seed=4)
    alpha = hr.softmax(graph, sv, se, group, 0.2, H)
    dsv, dse = torch.autograd.grad(alpha, (sv, se), dalpha)
    ds, csv, cse = hr.closed_form_backward(graph, sv.detach(), se.detach(), group, 0.2, alpha.detach(), dalpha)
    assert ds.shape == (inc.nnz, H)
    torch.testing.assert_close(csv, dsv, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(cse, dse, rtol=1e-10, atol=1e-12)
    # the weight gradients of the aggregation are per-head dot products: dv2e[p, h] = <X[u, head h], G[e, head h]>
    x = _rand(inc.N, H * C, seed=5)
    v2e, e2v = _rand(inc.nnz, H, seed=6).requires_grad_(True), _rand(inc.nnz, H, seed=7).requires_grad_(True)
    g = _rand(inc.N, H * C, seed=8)
    dv, de = torch.autograd.grad(hr.incidence_aggr(graph, x, v2e, e2v, H), (v2e, e2v), g)
    P = g * graph.degV.reshape(-1, 1)
    G = torch.cat([ir.hop1(graph, P[:, h * C:(h + 1) * C], e2v.detach()[:, h]) for h in range(H)], 1)
    Xe = torch.cat([ir.hop1(graph, x[:, h * C:(h + 1) * C], v2e.detach()[:, h]) for h in range(H)], 1)
    torch.testing.assert_close(hr.dot(graph, x, G, H), dv, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(hr.dot(graph, P, Xe, H), de, rtol=1e-10, atol=1e-12)


def test_one_head_is_the_single_head_reference():
    inc = ar.toy()
    graph = _graph(inc)
    sv, se, val = _rand(inc.N, seed=1), _rand(inc.M, seed=2), _rand(inc.nnz, seed=3)
    x, v2e, e2v = _rand(inc.N, 4, seed=4), _rand(inc.nnz, seed=5), _rand(inc.nnz, seed=6)
    w, a_v, a_e, bias = _rand(4, 3, seed=7), _rand(4, seed=8), _rand(4, seed=9), _rand(4, seed=10)
    for group in ar.GROUPS:
        alpha = ar.softmax(graph, sv, se, group, 0.2)
        assert torch.equal(hr.softmax(graph, sv[:, None], se[:, None], group, 0.2, 1)[:, 0], alpha)
        want = ar.closed_form_backward(graph, sv, se, group, 0.2, alpha, val)
        got = hr.closed_form_backward(graph, sv[:, None], se[:, None], group, 0.2, alpha[:, None], val[:, None])
        for a, b in zip(got, want):
            assert torch.equal(a[:, 0], b)
        assert torch.equal(hr.segment_sum(graph, val[:, None], group)[:, 0], ar.segment_sum(graph, val, group))
        # the layer forms its scores as a product and a sum where the single-head one calls a matrix product: float64 rounding
        torch.testing.assert_close(hr.attn_conv(graph, _rand(inc.N, 3, seed=11), w, a_v, a_e, bias, group, 0.2, 1, True),
                                   ar.attn_conv(graph, _rand(inc.N, 3, seed=11), w, a_v, a_e, bias, group, 0.2),
                                   rtol=1e-12, atol=1e-12)
    assert torch.equal(hr.incidence_aggr(graph, x, v2e[:, None], e2v[:, None], 1), ir.incidence_aggr(graph, x, v2e, e2v))
    b = _rand(inc.M, 4, seed=12)
    assert torch.equal(hr.dot(graph, x, b, 1)[:, 0], ir.dot(graph, x, b))
    # the mean over heads of identical heads is the head
    y2 = hr.attn_conv(graph, _rand(inc.N, 3, seed=11), torch.cat([w, w]), torch.cat([a_v, a_v]), torch.cat([a_e, a_e]),
                      bias, "hyperedge", 0.2, 2, False)
    torch.testing.assert_close(y2, ar.attn_conv(graph, _rand(inc.N, 3, seed=11), w, a_v, a_e, bias, "hyperedge", 0.2),
                               rtol=1e-12, atol=1e-12)


def test_argument_errors_need_no_device(hg, monkeypatch):
    from hypergef_amd import ops
    monkeypatch.setattr(ops, "cached_plan", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device touched")))
    inc = ar.toy()
    N, M, nnz, H = inc.N, inc.M, inc.nnz, 3
    ptr, ind = torch.from_numpy(inc.csrptr), torch.from_numpy(inc.colind)
    sv, se, val, x = torch.zeros(N, H), torch.zeros(M, H), torch.zeros(nnz, H), torch.zeros(N, 2 * H)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="heads"):
            ops.incidence_softmax(ptr, ind, sv, se, heads=bad)
        with pytest.raises(ValueError, match="heads"):
            ops.incidence_sum(ptr, ind, val, num_nodes=N, heads=bad)
        with pytest.raises(ValueError, match="heads"):
            ops.incidence_aggr(ptr, ind, x, val, val, heads=bad)
    # F % heads != 0
    with pytest.raises(ValueError, match="multiple of heads"):
        ops.incidence_aggr(ptr, ind, torch.zeros(N, 2 * H + 1), val, val, heads=H)
    # scores / weights / val of the wrong element count
    for bad_sv, bad_se in ((torch.zeros(N), se), (sv, torch.zeros(M)), (torch.zeros(N, H + 1), se), (sv, torch.zeros(M * H - 1))):
        with pytest.raises(ValueError, match="elements"):
            ops.incidence_softmax(ptr, ind, bad_sv, bad_se, num_nodes=N, heads=H)
    with pytest.raises(ValueError, match="elements"):
        ops.incidence_softmax(ptr, ind, None, torch.zeros(M), num_nodes=N, heads=H)
    for bad in (torch.zeros(nnz), torch.zeros(nnz, H + 1), torch.zeros(nnz * H - 1)):
        with pytest.raises(ValueError, match="elements"):
            ops.incidence_sum(ptr, ind, bad, num_nodes=N, heads=H)
        with pytest.raises(ValueError, match="per incidence and head"):
            ops.incidence_aggr(ptr, ind, x, bad, None, heads=H)
        with pytest.raises(ValueError, match="per incidence and head"):
            ops.incidence_aggr(ptr, ind, x, None, bad, heads=H)
    # the inherited refusals, with heads
    for variant in ("fused", "push_atomic", "push_groups"):
        with pytest.raises(ValueError, match="variant"):
            ops.incidence_softmax(ptr, ind, sv, se, options=ops.Options(variant=variant), heads=H)
        with pytest.raises(ValueError, match="variant"):
            ops.incidence_aggr(ptr, ind, x, val, val, options=ops.Options(variant=variant), heads=H)
    with pytest.raises(ValueError, match="group"):
        ops.incidence_softmax(ptr, ind, sv, se, group="edge", heads=H)
    with pytest.raises(ValueError, match="side"):
        ops.incidence_sum(ptr, ind, val, side="edge", num_nodes=N, heads=H)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_softmax(ptr, ind, sv.to(torch.bfloat16), se, heads=H)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_sum(ptr, ind, val.to(torch.bfloat16), num_nodes=N, heads=H)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_aggr(ptr, ind, x, val.to(torch.bfloat16), None, heads=H)
    with pytest.raises(ValueError, match="num_nodes"):
        ops.incidence_softmax(ptr, ind, None, se, heads=H)
    with pytest.raises(RuntimeError, match="GPU"):  # CPU tensors: refused as by every operator
        ops.incidence_softmax(ptr, ind, sv, se, heads=H)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_sum(ptr, ind, val, num_nodes=N, heads=H)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_aggr(ptr, ind, x, val, val, heads=H)
    # heads = 1 keeps today's rules: an [N, 1] score is flattened, a [nnz, 2] weight array is not one weight per incidence
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_softmax(ptr, ind, torch.zeros(N, 1), torch.zeros(M, 1), heads=1)
    with pytest.raises(ValueError, match="one weight per incidence \\(nnz"):
        ops.incidence_aggr(ptr, ind, x, torch.zeros(nnz, 2), None)


def test_plan_methods_refuse_bad_heads_before_any_tensor(hg):
    from hypergef_amd.plan import Plan, make_opts
    inc = ar.toy()
    plan = Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True))
    for bad in (0, -2, 1.5):
        for call in (lambda: plan.incidence_attention(None, None, heads=bad),
                     lambda: plan.incidence_attention_backward(None, None, None, None, heads=bad),
                     lambda: plan.incidence_sum(None, None, None, heads=bad),
                     lambda: plan.aggregate_incidence(None, None, None, heads=bad),
                     lambda: plan.incidence_dot(None, None, None, None, heads=bad)):
            with pytest.raises(ValueError, match="heads"):
                call()


def test_exports_and_host_only_refusals(hg):
    from hypergef_amd import _lib
    from hypergef_amd.plan import Plan, make_opts
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hg_aggr.h")).read()
    for name in HEADS_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert "HG_API int %s(" % name in header, name
    assert L.hg_version() == 410
    inc = ar.toy()
    plan = Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True))
    null = ctypes.c_void_p()
    calls = {
        "attention": lambda p, h: L.hg_incidence_attention_heads_f32(p, 0, h, null, null, null, null, 0.2, null, null),
        "attention_bwd": lambda p, h: L.hg_incidence_attention_heads_bwd_f32(p, 1, h, null, null, null, null, 0.2, null, null,
                                                                             null, null, null, null),
        "sum": lambda p, h: L.hg_incidence_sum_heads_f32(p, 1, h, null, null, null, null, null),
        "aggr": lambda p, h: L.hg_aggr_incidence_heads_f32(p, 12, h, null, null, null, null, null, null, null, null, null,
                                                           null, null, 0, null),
        "dot": lambda p, h: L.hg_incidence_dot_heads_f32(p, 12, h, null, null, null, null, null, null),
    }
    for name, call in calls.items():
        for heads in (1, 4):
            assert call(plan._h, heads) == _lib.HG_ERR_UNSUPPORTED, (name, heads)
            assert b"HOST_ONLY" in L.hg_last_error(), name
        for heads in (0, -3):
            assert call(plan._h, heads) == _lib.HG_ERR_INVALID, (name, heads)
            assert b"heads" in L.hg_last_error(), name
        assert call(null, 2) == _lib.HG_ERR_INVALID, name
    for name in ("aggr", "dot"):  # F = 12 is no multiple of 5 or 8
        for heads in (5, 8):
            assert calls[name](plan._h, heads) == _lib.HG_ERR_INVALID, (name, heads)
            assert b"multiple of heads" in L.hg_last_error(), name


def test_layer_with_one_head_is_the_layer_without_the_argument(hg):
    inc = ar.toy()
    hyperg = hg.HyperGraph.from_incidence(inc, "cpu", data_name="toy")
    torch.manual_seed(5)
    plain = hg.HypergraphAttnConv(hyperg, 5, 3, group="vertex", negative_slope=0.1)
    torch.manual_seed(5)
    one = hg.HypergraphAttnConv(hyperg, 5, 3, group="vertex", negative_slope=0.1, heads=1, concat=False)
    a, b = plain.state_dict(), one.state_dict()
    assert list(a) == list(b) == ["a_v", "a_e", "bias", "lin.weight"]
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    assert {n: tuple(p.shape) for n, p in one.named_parameters()} == {"lin.weight": (3, 5), "a_v": (3,), "a_e": (3,),
                                                                      "bias": (3,)}


@pytest.mark.parametrize("concat", [True, False])
def test_layer_shapes_with_four_heads(hg, concat):
    inc = ar.toy()
    hyperg = hg.HyperGraph.from_incidence(inc, "cpu", data_name="toy")
    layer = hg.HypergraphAttnConv(hyperg, 5, 3, heads=4, concat=concat)
    shapes = {n: tuple(p.shape) for n, p in layer.named_parameters()}
    assert shapes == {"lin.weight": (12, 5), "a_v": (12,), "a_e": (12,), "bias": (12,) if concat else (3,)}
    assert not list(layer.buffers()) and layer.heads == 4 and layer.concat is concat
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="heads"):
            hg.HypergraphAttnConv(hyperg, 5, 3, heads=bad)
