"""CPU self-checks of the float64 gradient reference (tests/_grad_ref.py): it has the transpose it claims, the reference
rule returns forward(grad), its layer formulas agree with the plain-torch models (models.Torch*Conv) in float64, and its
forward agrees with the C oracle.  A GPU gradient test that fails then points at the library, not at the reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _grad_ref as gr  # noqa: E402

from conftest import vertex_csr  # noqa: E402
from hypergef_amd import synth  # noqa: E402

F64 = torch.float64


def _small(seed=0):
    """Ragged: an empty hyperedge (degE = inf) first and last, two isolated vertices, besides ordinary ones."""
    base = synth.random_incidence(40, 25, 3.0, seed=seed)
    ptr = np.concatenate([[0], base.csrptr, [base.nnz]])
    inc = synth.Incidence(base.N + 2, base.M + 2, ptr, base.colind, "small")
    sizes = inc.sizes()
    deg = np.bincount(inc.colind, minlength=inc.N)
    assert (sizes == 0).sum() >= 2 and (deg == 0).sum() >= 2
    with np.errstate(divide="ignore"):
        degE = torch.from_numpy((1.0 / sizes).astype(np.float32))
        degV = torch.from_numpy(np.where(deg > 0, deg.astype(np.float64) ** -0.5, 1.0).astype(np.float32))
    W = torch.from_numpy((np.random.default_rng(seed).random(inc.M) + 0.5).astype(np.float32))
    return inc, degE, degV, W


def _dense(graph):
    """A as a dense [N, N] float64 matrix, column by column."""
    return graph.A(torch.eye(graph.N, dtype=F64))


@pytest.mark.parametrize("scales", ["all", "deg", "none"])
def test_adjoint_rule_passes_gradcheck(scales):
    inc, degE, degV, W = _small(1)
    graph = gr.Graph(inc, degE if scales != "none" else None, degV if scales != "none" else None,
                     W if scales == "all" else None)
    x = torch.randn(inc.N, 3, dtype=F64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: graph.aggr(t, "adjoint"), (x,))
    A = _dense(graph)
    g = torch.randn(inc.N, 3, dtype=F64)
    assert torch.allclose(graph.AT(g), A.t() @ g, rtol=1e-12, atol=1e-12)
    assert torch.isfinite(A).all()  # empty hyperedges contribute nothing, not inf * 0


def test_layer_formulas_pass_gradcheck_under_the_adjoint_rule():
    inc, degE, degV, W = _small(2)
    graph = gr.Graph(inc, degE, degV, W)
    r = lambda *s: torch.randn(*s, dtype=F64, requires_grad=True)
    x, w, m, res, cb = r(inc.N, 4), r(3, 4), r(5, 4), r(inc.N, 4), r(())
    mask = torch.rand(inc.N, 5) > 0.3
    assert torch.autograd.gradcheck(lambda a, b: gr.hgnnaggr_linear(graph, a, b, "adjoint"), (x, w))
    for ca in (1.0, 0.9, 0.0, -0.5):
        assert torch.autograd.gradcheck(
            lambda a, b, c, d: gr.aggr_res_linear(graph, a, b, "adjoint", residual=c, ca=ca, cb=d, mask=mask),
            (x, m, res, cb))
    bias = r(3)
    assert torch.autograd.gradcheck(gr.linear, (x, w, bias))


def test_reference_rule_returns_forward_of_grad():
    inc, degE, degV, W = _small(3)
    for graph in (gr.Graph(inc, degE, degV, W), gr.Graph(inc, degE, degV), gr.Graph(inc)):
        x = torch.randn(inc.N, 5, dtype=F64, requires_grad=True)
        g = torch.randn(inc.N, 5, dtype=F64)
        gx, = torch.autograd.grad(graph.aggr(x, "reference"), x, g)
        assert torch.equal(gx, graph.A(g))
        ga, = torch.autograd.grad(graph.aggr(x, "adjoint"), x, g)
        if graph.degV is None:  # without degV the two rules coincide (A is symmetric) ...
            assert torch.allclose(gx, ga, rtol=1e-12, atol=1e-12)
        else:  # ... with it they do not: the reference rule is not the transpose
            assert not torch.allclose(gx, ga, rtol=1e-6, atol=1e-6)


def _torch_graph(inc):
    import hypergef_amd as hg
    from hypergef_amd import models
    hyperg = hg.HyperGraph.from_incidence(inc, "cpu")
    return hyperg, models._TorchGraph(hyperg, "cpu")


def test_layer_formulas_match_the_torch_models_in_float64():
    from hypergef_amd import models
    inc, _, _, _ = _small(4)
    hyperg, tg = _torch_graph(inc)
    graph = gr.Graph(inc, hyperg.degE, hyperg.degV)
    torch.manual_seed(4)
    X = torch.randn(inc.N, 6, dtype=F64, requires_grad=True)
    X0 = torch.randn(inc.N, 6, dtype=F64, requires_grad=True)
    G = torch.randn(inc.N, 6, dtype=F64)

    def check(want, got, params):
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
        gw = torch.autograd.grad(want, params, G, retain_graph=True)
        gg = torch.autograd.grad(got, params, G)
        for a, b in zip(gw, gg):
            assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)

    conv = models.TorchHGNNConv(tg, 6, 6, "sum").double()
    check(conv(X), gr.hgnnaggr_linear(graph, X, conv.linear.weight, "adjoint"), (X, conv.linear.weight))

    conv = models.TorchGINConv(tg, 6, 6, "sum").double()
    conv.eps.data.fill_(0.25)
    plain = gr.Graph(inc)
    check(conv(X), gr.unigin(plain, X, conv.W.weight, conv.eps, "adjoint"), (X, conv.W.weight, conv.eps))
    # the fused form of the same layer: ((1 + eps) X + Aggr(X)) . W^T
    check(conv(X), gr.aggr_res_linear(plain, X, conv.W.weight, "adjoint", residual=X, ca=1.0, cb=1 + conv.eps),
          (X, conv.W.weight, conv.eps))

    conv = models.TorchGCNIIConv(tg, 6, 6).double()
    for alpha, beta in ((0.1, 0.4), (1.0, 0.3), (0.0, 0.5)):
        want = conv(X, X0, alpha, beta)
        check(want, gr.unigcnii(graph, X, X0, conv.W.weight, "adjoint", 1 - alpha, alpha, 1 - beta, beta),
              (X, X0, conv.W.weight))
        Mm = (1 - beta) * torch.eye(6, dtype=F64) + beta * conv.W.weight  # the fused layer's M
        check(want, gr.aggr_res_linear(graph, X, Mm, "adjoint", residual=X0, ca=1 - alpha, cb=alpha), (X, X0))


def test_forward_agrees_with_the_oracle(oracle):
    inc = synth.cora_shape()
    degE, degV = oracle.degrees(inc.N, inc.M, inc.csrptr, inc.colind)
    W = (np.random.default_rng(5).random(inc.M) + 0.5).astype(np.float32)
    X = np.random.default_rng(6).standard_normal((inc.N, 7)).astype(np.float32)
    H_ptr, H_ind = vertex_csr(inc, oracle)
    want = oracle.hgnn_check(inc.N, inc.M, 7, H_ptr, H_ind, inc.csrptr, inc.colind, X, degE, degV, W)
    graph = gr.Graph(inc, degE, degV, W)
    y = graph.A(gr.f64(X))
    mass = graph.abs().A(gr.f64(X).abs())
    gr.assert_within(torch.from_numpy(want), y, mass, gr.FP32_C, "oracle vs float64")


def test_bounds_reject_what_they_should():
    """The checks themselves: an element off by more than c * mass fails, a NaN fails, a flushed subnormal fails."""
    ref = torch.tensor([1.0, -2.0, 3e-40], dtype=F64)
    mass = torch.tensor([1.0, 4.0, 3e-40], dtype=F64)
    gr.assert_within(ref.float(), ref, mass, gr.FP32_C)
    for got in ([1.0 + 2e-5, -2.0, 3e-40], [float("nan"), -2.0, 3e-40], [1.0, -2.0, 0.0]):
        with pytest.raises(AssertionError):
            gr.assert_within(torch.tensor(got, dtype=torch.float32), ref, mass, gr.FP32_C)
    pre = torch.tensor([1.0, -1.0, 1e-9], dtype=F64)
    gr.assert_mask_agrees(torch.tensor([1.0, 0.0, 0.0]), pre, torch.ones(3, dtype=F64), gr.FP32_C)
    with pytest.raises(AssertionError):
        gr.assert_mask_agrees(torch.tensor([0.0, 0.0, 0.0]), pre, torch.ones(3, dtype=F64), gr.FP32_C)
