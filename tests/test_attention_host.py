"""CPU-only checks of the hypergraph attention coefficients: the float64 reference of tests/_attention_ref.py against
gradcheck and autograd, the closed-form backward the library implements, the plan's cut of each side into lane groups and
long rows (host-only plans), the operators' argument errors (raised before a device is touched), the exported symbols and
the layer's parameters."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402
import _grad_ref as gr  # noqa: E402

from hypergef_amd import synth  # noqa: E402

SLOPES = (0.2, 1.0)


def _scores(inc, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(inc.N, dtype=torch.float64, generator=g), torch.randn(inc.M, dtype=torch.float64, generator=g)


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("group", ar.GROUPS)
def test_reference_softmax_passes_gradcheck(group, slope):
    inc = ar.toy()
    graph = gr.Graph(inc)
    sv, se = (t.requires_grad_(True) for t in _scores(inc))
    assert torch.autograd.gradcheck(lambda a, b: ar.softmax(graph, a, b, group, slope), (sv, se))
    assert torch.autograd.gradcheck(lambda a: ar.softmax(graph, a, None, group, slope), (sv,))
    assert torch.autograd.gradcheck(lambda b: ar.softmax(graph, None, b, group, slope), (se,))


@pytest.mark.parametrize("side", ar.GROUPS)
def test_reference_segment_sum_passes_gradcheck(side):
    inc = ar.toy()
    graph = gr.Graph(inc)
    val = torch.randn(inc.nnz, dtype=torch.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: ar.segment_sum(graph, v, side), (val,))
    out = ar.segment_sum(graph, val.detach(), side)
    assert out.shape == ((inc.M,) if side == "hyperedge" else (inc.N,))
    assert float(out[2 if side == "hyperedge" else 4]) == 0.0  # the empty hyperedge / the isolated vertex


@pytest.mark.parametrize("group", ar.GROUPS)
def test_reference_softmax_facts(group):
    inc = ar.toy()
    graph = gr.Graph(inc)
    sv, se = _scores(inc, 1)
    alpha = ar.softmax(graph, sv, se, group, 0.2)
    sums = ar.segment_sum(graph, alpha, group)
    idx, n = ar.index_of(graph, group)
    sizes = torch.bincount(idx, minlength=n)
    torch.testing.assert_close(sums[sizes > 0], torch.ones(int((sizes > 0).sum()), dtype=torch.float64))
    assert bool((sums[sizes == 0] == 0).all()) and int((sizes == 0).sum()) == 1
    assert bool((alpha[sizes[idx] == 1] == 1.0).all()) and int((sizes == 1).sum()) >= 1
    # scores of magnitude 1e4 stay finite once the maximum is subtracted
    big = ar.softmax(graph, sv * 1e4, se * 1e4, group, 0.2)
    assert bool(torch.isfinite(big).all())


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("group", ar.GROUPS)
@pytest.mark.parametrize("shape", ["toy", "ragged"])
def test_closed_form_backward_equals_autograd(shape, group, slope):
    inc = ar.toy() if shape == "toy" else synth.random_incidence(300, 200, 5.0, seed=3, empty_frac=0.1)
    graph = gr.Graph(inc)
    sv, se = (t.requires_grad_(True) for t in _scores(inc, 2))
    dalpha = torch.randn(inc.nnz, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    alpha = ar.softmax(graph, sv, se, group, slope)
    dsv, dse = torch.autograd.grad(alpha, (sv, se), dalpha)
    ds, csv, cse = ar.closed_form_backward(graph, sv.detach(), se.detach(), group, slope, alpha.detach(), dalpha)
    torch.testing.assert_close(csv, dsv, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(cse, dse, rtol=1e-10, atol=1e-12)
    # ds itself is the gradient of the per-incidence score
    raw = ar.raw_score(graph, sv.detach(), se.detach()).requires_grad_(True)
    idx, n = ar.index_of(graph, group)
    e = torch.exp(torch.nn.functional.leaky_relu(raw, slope))
    a2 = e / torch.zeros(n, dtype=torch.float64).index_add_(0, idx, e)[idx]
    torch.testing.assert_close(ds, torch.autograd.grad(a2, raw, dalpha)[0], rtol=1e-10, atol=1e-12)


def _boundaries(width=4, keep=4, long=128):
    sizes = sorted(set(list(range(0, 71)) + [255, 256, 257, 1023, 1024, 1025, 5000]
                       + [t + d for t in (width * keep, long, 256 * keep) for d in (-1, 0, 1)]))
    return synth._from_sizes(np.random.default_rng(7), 6000, sizes, name="boundaries")


def test_segment_info_on_host_only_plans(hg):
    from hypergef_amd.plan import Plan, make_opts
    for inc in (ar.toy(), _boundaries(), ar.transpose(_boundaries()), synth.cora_shape()):
        plan = Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True))
        ptr_v, _ = plan.vertex_csr()
        for side, ptr in (("hyperedge", inc.csrptr), ("vertex", ptr_v)):
            info = plan.segment_info(side)
            lens = np.diff(ptr)
            assert info["keep"] == 4 and info["long"] == 128
            np.testing.assert_array_equal(info["long_rows"], np.nonzero(lens > info["long"])[0].astype(np.int32))
            short = lens[(lens > 0) & (lens <= info["long"])]
            mean = short.mean() if short.size else 0.0
            assert info["width"] == (4 if mean <= 4 else 8 if mean <= 8 else 16), (inc.name, side, mean, info)
            again = plan.segment_info(side)  # built once, asked twice
            assert again["width"] == info["width"]
            np.testing.assert_array_equal(again["long_rows"], info["long_rows"])


def test_width_steered_shapes_land_in_their_bands(hg):
    """The shapes of test_attention_widths.py, on host-only plans: the designed side of widths_W / its transpose runs at
    lane-group width W and holds every threshold +-1, 0, 1 and 5000; a change of seg_width or of the constants that moves
    a shape out of its band fails here, without a device."""
    from hypergef_amd.plan import Plan, make_opts

    def host_plan(inc):
        return Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True))
    for width, mean in ((4, 2.85), (8, 6.75), (16, 12.61)):
        inc = ar.width_shape(width)
        assert inc.M == 3081 and inc.nnz <= 48_000
        for shape, side in ((inc, "hyperedge"), (ar.transpose(inc), "vertex")):
            info = host_plan(shape).segment_info(side)
            lens = ar.side_lengths(shape, side)
            walked = lens[(lens > 0) & (lens <= info["long"])]
            assert abs(walked.mean() - mean) < 0.005, (shape.name, side, walked.mean())
            assert info["width"] == width, (shape.name, side, info)
            assert ar.reaches_every_path(info, lens) is None, (shape.name, side, ar.reaches_every_path(info, lens))
            assert lens.size % (256 // width) != 0  # the last workgroup has lane groups without a segment
            np.testing.assert_array_equal(info["long_rows"], np.nonzero(lens > info["long"])[0])
            other = ar.GROUPS[1 - ar.GROUPS.index(side)]
            info = host_plan(shape).segment_info(other)  # the other side: short rows, kept entries only
            assert info["width"] in (4, 8) and ar.longest(shape, other) < info["width"] * info["keep"]
    dup = ar.with_duplicates(ar.width_shape(4))
    assert host_plan(dup).segment_info("hyperedge")["width"] == 4 and dup.nnz > 1.02 * ar.width_shape(4).nnz
    # every non-empty row is long: the mean of the rows a lane group walks is 0, the width 4
    inc = synth._from_sizes(np.random.default_rng(5), 1100, [129, 0, 300, 1024], name="all_long")
    info = host_plan(inc).segment_info("hyperedge")
    assert info["width"] == 4
    np.testing.assert_array_equal(info["long_rows"], [0, 2, 3])
    empty = synth.Incidence(7, 5, np.zeros(6, np.int32), np.zeros(0, np.int32), name="no_entries")
    for side in ar.GROUPS:
        info = host_plan(empty).segment_info(side)
        assert info["width"] == 4 and info["long_rows"].size == 0


def test_host_only_plans_are_refused_by_the_device_entries(hg):
    from hypergef_amd import _lib
    from hypergef_amd.plan import Plan, make_opts
    inc = ar.toy()
    plan = Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True))
    L = _lib.lib()
    null = ctypes.c_void_p()
    assert L.hg_incidence_attention_f32(plan._h, 0, null, null, null, null, 0.2, null, null) == _lib.HG_ERR_UNSUPPORTED
    assert b"HOST_ONLY" in L.hg_last_error()
    assert L.hg_incidence_attention_bwd_f32(plan._h, 1, null, null, null, null, 0.2, null, null, null, null, null,
                                            null) == _lib.HG_ERR_UNSUPPORTED
    assert L.hg_incidence_sum_f32(plan._h, 1, null, null, null, null, null) == _lib.HG_ERR_UNSUPPORTED
    assert L.hg_incidence_sum_f32(null, 0, null, null, null, null, null) == _lib.HG_ERR_INVALID
    assert L.hg_plan_get_segment_info(plan._h, 2, (ctypes.c_int32 * 4)(), null) == _lib.HG_ERR_INVALID


def test_argument_errors_need_no_device(hg, monkeypatch):
    from hypergef_amd import ops
    monkeypatch.setattr(ops, "cached_plan", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device touched")))
    inc = ar.toy()
    ptr, ind = torch.from_numpy(inc.csrptr), torch.from_numpy(inc.colind)
    sv, se, val = torch.zeros(inc.N), torch.zeros(inc.M), torch.zeros(inc.nnz)
    for variant in ("fused", "push_atomic", "push_groups"):
        with pytest.raises(ValueError, match="variant"):
            ops.incidence_softmax(ptr, ind, sv, se, options=ops.Options(variant=variant))
    with pytest.raises(ValueError, match="group"):
        ops.incidence_softmax(ptr, ind, sv, se, group="edge")
    with pytest.raises(ValueError, match="side"):
        ops.incidence_sum(ptr, ind, val, side="edge", num_nodes=inc.N)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_softmax(ptr, ind, sv.to(torch.bfloat16), se)
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_softmax(ptr, ind, sv, se.to(torch.bfloat16))
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_sum(ptr, ind, val.to(torch.bfloat16), num_nodes=inc.N)
    with pytest.raises(ValueError, match="elements"):
        ops.incidence_softmax(ptr, ind, sv, torch.zeros(inc.M + 1))
    with pytest.raises(ValueError, match="elements"):
        ops.incidence_softmax(ptr, ind, None, torch.zeros(inc.M - 1), num_nodes=inc.N)
    with pytest.raises(ValueError, match="elements"):
        ops.incidence_sum(ptr, ind, torch.zeros(inc.nnz - 1), num_nodes=inc.N)
    with pytest.raises(ValueError, match="num_nodes"):
        ops.incidence_softmax(ptr, ind, None, se)
    for bad in (torch.zeros(inc.N + 1), torch.zeros(inc.N - 1)):  # N is known: node_score must match it
        with pytest.raises(ValueError, match="elements"):
            ops.incidence_softmax(ptr, ind, bad, se, num_nodes=inc.N)
    for group in ar.GROUPS:
        with pytest.raises(RuntimeError, match="GPU"):  # CPU tensors: refused as by every operator
            ops.incidence_softmax(ptr, ind, sv, se, group=group)
        with pytest.raises(RuntimeError, match="GPU"):
            ops.incidence_sum(ptr, ind, val, side=group, num_nodes=inc.N)


def test_exports(hg):
    assert hg.incidence_softmax is hg.ops.incidence_softmax
    assert hg.incidence_sum is hg.ops.incidence_sum
    from hypergef_amd import _lib, models
    assert hg.HypergraphAttnConv is models.HypergraphAttnConv
    for name in ("hg_incidence_attention_f32", "hg_incidence_attention_bwd_f32", "hg_incidence_sum_f32"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert _lib.lib().hg_version() == 410


@pytest.mark.parametrize("group", ar.GROUPS)
def test_layer_has_exactly_its_parameters(hg, group):
    inc = ar.toy()
    hyperg = hg.HyperGraph.from_incidence(inc, "cpu", data_name="toy")
    layer = hg.HypergraphAttnConv(hyperg, 5, 3, group=group, negative_slope=0.1)
    shapes = {n: tuple(p.shape) for n, p in layer.named_parameters()}
    assert shapes == {"lin.weight": (3, 5), "a_v": (3,), "a_e": (3,), "bias": (3,)}
    assert not list(layer.buffers())
    assert isinstance(layer.lin, hg.ops.Linear) and layer.group == group and layer.negative_slope == 0.1
    with pytest.raises(ValueError, match="group"):
        hg.HypergraphAttnConv(hyperg, 5, 3, group="edge")


def test_reference_layer_matches_a_dense_formula():
    """attn_conv against the same layer written with a dense [N, M] coefficient matrix."""
    inc = synth.random_incidence(40, 25, 3.0, seed=5, empty_frac=0.1)
    degE = torch.from_numpy(np.diff(inc.csrptr).astype(np.float32)).pow(-1)
    degV = torch.rand(inc.N) + 0.5
    graph = gr.Graph(inc, degE, degV, None)
    g = torch.Generator().manual_seed(6)
    x, w = torch.randn(inc.N, 4, dtype=torch.float64, generator=g), torch.randn(3, 4, dtype=torch.float64, generator=g)
    a_v, a_e, bias = (torch.randn(3, dtype=torch.float64, generator=g) for _ in range(3))
    for group in ar.GROUPS:
        got = ar.attn_conv(graph, x, w, a_v, a_e, bias, group, 0.2)
        z = x @ w.t()
        Hm = torch.zeros(inc.N, inc.M, dtype=torch.float64)
        Hm[graph.V, graph.E] = 1.0
        sizes = Hm.sum(0)
        se = (Hm.t() @ (z @ a_e)) / sizes.clamp(min=1)
        s = torch.nn.functional.leaky_relu((z @ a_v)[:, None] + se[None, :], 0.2).masked_fill(Hm == 0, -float("inf"))
        A = torch.nan_to_num(torch.softmax(s, dim=0 if group == "hyperedge" else 1), nan=0.0) * Hm
        xe = (A.t() @ z) * torch.nan_to_num(graph.degE, posinf=0.0)[:, None]
        want = (A @ xe) * graph.degV[:, None] + bias
        torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-12)
