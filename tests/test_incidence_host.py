"""CPU-only checks of the incidence-weighted aggregation: the plan's H-to-H_T permutation (host-only plans), the float64
reference of tests/_incidence_ref.py against autograd, gradcheck and the unweighted reference, and the operator's
argument errors, all raised before a device is touched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _grad_ref as gr  # noqa: E402
import _incidence_ref as ir  # noqa: E402

from hypergef_amd import synth  # noqa: E402


def _dup_vertex():
    """A hand-made H_T: vertex 2 listed twice in hyperedge 1, an empty hyperedge 2, vertex 4 in no hyperedge."""
    ptr = np.array([0, 3, 7, 7, 9], np.int32)
    ind = np.array([0, 2, 3, 1, 2, 2, 5, 0, 5], np.int32)
    return synth.Incidence(6, 4, ptr, ind, name="dup")


SHAPES = {
    "cora": synth.cora_shape,
    "citeseer": synth.citeseer_shape,
    "pubmed": synth.pubmed_shape,
    "ragged": lambda: synth.random_incidence(700, 450, 7.0, seed=3, empty_frac=0.1),
    "dup": _dup_vertex,
}


def _host_plan(hg, inc):
    from hypergef_amd.plan import Plan, make_opts
    return Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_perm_is_the_stable_transpose(hg, shape):
    inc = SHAPES[shape]()
    plan = _host_plan(hg, inc)
    perm = plan.incidence_perm()
    assert perm.dtype == np.int32 and perm.shape == (inc.nnz,)
    np.testing.assert_array_equal(perm, np.argsort(inc.colind, kind="stable"))
    # H entry q is the hyperedge that holds H_T position perm[q], and the vertex there is q's row
    ptr_v, ind_v = plan.vertex_csr()
    E = np.repeat(np.arange(inc.M), np.diff(inc.csrptr))
    np.testing.assert_array_equal(ind_v, E[perm])
    rows = np.repeat(np.arange(inc.N), np.diff(ptr_v))
    np.testing.assert_array_equal(inc.colind[perm], rows)
    np.testing.assert_array_equal(plan.incidence_perm(), perm)  # built once, asked twice


def _case(shape, seed=0, F=3, scales=True):
    inc = SHAPES[shape]()
    rng = np.random.default_rng(seed)
    degE = torch.from_numpy(np.diff(inc.csrptr).astype(np.float32)).pow(-1) if scales else None  # inf on empty edges
    degV = torch.from_numpy(rng.random(inc.N).astype(np.float32) + 0.5) if scales else None
    W = torch.from_numpy(rng.random(inc.M).astype(np.float32) + 0.5) if scales else None
    graph = gr.Graph(inc, degE, degV, W)
    x = torch.from_numpy(rng.standard_normal((inc.N, F))).to(torch.float64)
    v2e = torch.from_numpy(rng.standard_normal(inc.nnz))
    e2v = torch.from_numpy(rng.standard_normal(inc.nnz))
    return inc, graph, x, v2e, e2v


@pytest.mark.parametrize("shape", ["ragged", "dup"])
def test_reference_passes_gradcheck(shape):
    inc, graph, x, v2e, e2v = _case(shape, F=2)
    if shape == "ragged":  # keep the numerical Jacobian small: a sub-block of the graph is enough
        inc = synth.random_incidence(40, 25, 3.0, seed=5, empty_frac=0.1)
        graph = gr.Graph(inc, torch.from_numpy(np.diff(inc.csrptr).astype(np.float32)).pow(-1),
                         torch.rand(inc.N) + 0.5, torch.rand(inc.M) + 0.5)
        x = torch.randn(inc.N, 2, dtype=torch.float64)
        v2e, e2v = torch.randn(inc.nnz, dtype=torch.float64), torch.randn(inc.nnz, dtype=torch.float64)
    ins = tuple(t.clone().requires_grad_(True) for t in (x, v2e, e2v))
    assert torch.autograd.gradcheck(lambda a, b, c: ir.incidence_aggr(graph, a, b, c), ins)


@pytest.mark.parametrize("scales", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_reference_with_unit_weights_is_the_sum_aggregation(shape, scales):
    inc, graph, x, _, _ = _case(shape, scales=scales)
    ones = torch.ones(inc.nnz, dtype=torch.float64)
    want = graph.A(x)
    torch.testing.assert_close(ir.incidence_aggr(graph, x, ones, ones), want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ir.incidence_aggr(graph, x), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_closed_form_gradients_equal_autograd(shape):
    inc, graph, x, v2e, e2v = _case(shape, seed=1, F=4)
    g = torch.randn(inc.N, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    xs, vs, es = (t.clone().requires_grad_(True) for t in (x, v2e, e2v))
    dx, dv, de = torch.autograd.grad(ir.incidence_aggr(graph, xs, vs, es), (xs, vs, es), g)
    cx, cv, ce = ir.closed_form_grads(graph, x, v2e, e2v, g)
    for got, want in ((cx, dx), (cv, dv), (ce, de)):
        torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10)
    # the weight gradients are incidence dots: dv2e = dot(X, G), de2v = dot(P, Xe)
    P = g * graph.degV.reshape(-1, 1)
    torch.testing.assert_close(ir.dot(graph, x, ir.hop1(graph, P, e2v)), dv, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(ir.dot(graph, P, ir.hop1(graph, x, v2e)), de, rtol=1e-10, atol=1e-10)


def _cpu_args(inc, F=4, dtype=torch.float32):
    ptr = torch.from_numpy(inc.csrptr)
    ind = torch.from_numpy(inc.colind)
    x = torch.zeros(inc.N, F, dtype=dtype)
    return ptr, ind, x


def test_argument_errors_need_no_device(hg, monkeypatch):
    from hypergef_amd import ops
    # any device access would go through the plan cache: make that an error of its own kind
    monkeypatch.setattr(ops, "cached_plan", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device touched")))
    inc = SHAPES["dup"]()
    ptr, ind, x = _cpu_args(inc)
    w = torch.ones(inc.nnz)
    for variant in ("fused", "push_atomic", "push_groups"):
        with pytest.raises(ValueError, match="variant"):
            ops.incidence_aggr(ptr, ind, x, w, w, options=ops.Options(variant=variant))
    with pytest.raises(TypeError, match="bfloat16"):
        ops.incidence_aggr(ptr, ind, x.to(torch.bfloat16), w, w)
    with pytest.raises(TypeError, match="float32"):
        ops.incidence_aggr(ptr, ind, x, w.to(torch.bfloat16), None)
    for bad in (torch.ones(inc.nnz - 1), torch.ones(inc.nnz + 1)):
        with pytest.raises(ValueError, match="nnz"):
            ops.incidence_aggr(ptr, ind, x, bad, None)
        with pytest.raises(ValueError, match="nnz"):
            ops.incidence_aggr(ptr, ind, x, None, bad)
    with pytest.raises(RuntimeError, match="GPU"):  # CPU tensors: refused as by every operator
        ops.incidence_aggr(ptr, ind, x, w, w)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_aggr(ptr, ind, x)
    with pytest.raises(ValueError, match="variant"):
        ops.HGNNAggrIncidence(_Bag(ptr, ind), x, w, w, None, None, None, options=ops.Options(variant="fused"))


class _Bag:
    def __init__(self, ptr, ind):
        self.H_T_csrptr, self.H_T_colind = ptr, ind


def test_exports(hg):
    assert hg.incidence_aggr is hg.ops.incidence_aggr
    assert hg.HGNNAggrIncidence is hg.ops.HGNNAggrIncidence
    from hypergef_amd import _lib
    for name in ("hg_aggr_incidence_workspace_bytes", "hg_aggr_incidence_f32", "hg_incidence_dot_f32",
                 "hg_plan_get_incidence_perm"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
