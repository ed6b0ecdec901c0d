"""The incidence-weighted aggregation on the GPU (hg_aggr_incidence_f32, hg_incidence_dot_f32, ops.incidence_aggr).

1. Bit for bit: unit weights and NULL weights give exactly the unweighted pull variant on a plan without the streaming
   row kernel (the same panels + wave-task kernels), power-of-two weights exactly scale it, two calls agree, and a
   captured hipGraph replay equals the eager call.
2. Accuracy: signed random weights with exact zeros, against float64, within FP32_C * max(mass, TINY) per element;
   v2e and e2v distinct and each checked alone, so a missing or wrong hop-2 permutation fails.
3. Gradients: dX at FP32_C, dv2e / de2v at FP32_C + (F + 1) 2^-24 (the dot product's recursive-summation bound on top
   of the error of G or Xe); incidence_dot alone at max(FP32_C, (F + 2) 2^-24) and deterministic; a small attention
   layer's parameter gradients against the same layer in float64 torch.
4. The refused inputs.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _grad_ref as gr  # noqa: E402
import _incidence_ref as ir  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
WIDTHS = (1, 3, 4, 8, 16, 32, 33, 64, 128)
SHAPES = {
    "cora": synth.cora_shape,
    "citeseer": synth.citeseer_shape,
    "pubmed": synth.pubmed_shape,
    "cora_x64": lambda: synth.replicate_block_diagonal(synth.cora_shape(), 64),
    "citeseer_x64": lambda: synth.replicate_block_diagonal(synth.citeseer_shape(), 64),
    "pubmed_x64": lambda: synth.replicate_block_diagonal(synth.pubmed_shape(), 64),
    "ragged": lambda: synth.random_incidence(3000, 2000, 6.0, seed=4, empty_frac=0.1),
    "powerlaw": lambda: synth.powerlaw(50_000, 200_000),
}


class _Case:
    def __init__(self, hg, name):
        from hypergef_amd.plan import Plan, make_opts
        self.inc = inc = SHAPES[name]()
        self.h = hg.HyperGraph.from_incidence(inc, DEV, data_name=name)
        self.ptr, self.ind = self.h.H_T_csrptr, self.h.H_T_colind
        self.plan = Plan.from_tensors(inc.N, self.ptr, self.ind, make_opts(row_stream=False))
        rng = np.random.default_rng(11)
        self.W = torch.from_numpy(rng.random(inc.M).astype(np.float32) + 0.5).to(DEV)
        self.degE, self.degV = self.h.degE.reshape(-1), self.h.degV.reshape(-1)  # degE = inf on empty hyperedges
        w = rng.standard_normal((2, inc.nnz)).astype(np.float32)
        w[rng.random((2, inc.nnz)) < 0.1] = 0.0  # exact zeros
        self.v2e, self.e2v = (torch.from_numpy(r.copy()).to(DEV) for r in w)
        self._graphs = {}

    def scales(self, on):
        return (self.degE, self.degV, self.W) if on else (None, None, None)

    def graph(self, on):
        if on not in self._graphs:
            self._graphs[on] = gr.Graph(self.inc, *self.scales(on))
        return self._graphs[on]


_CASES = {}


@pytest.fixture
def case(hg):
    def get(name):
        if name not in _CASES:
            _CASES.clear()  # one shape at a time on the device (the x64 / power-law ones are large)
            torch.cuda.empty_cache()
            _CASES[name] = _Case(hg, name)
        return _CASES[name]
    return get


def _x(case, F, seed=0, unaligned=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = case.inc.N * F
    if unaligned:  # a contiguous view 4 bytes past an allocation: 4-byte lanes only
        buf = torch.randn(n + 1, device=DEV, generator=g)
        x = buf[1:].view(case.inc.N, F)
        assert x.data_ptr() % 16 == 4
        return x
    return torch.randn(case.inc.N, F, device=DEV, generator=g)


def _bits(t):
    return t.contiguous().view(torch.int32)


CELLS = [(s, F) for s in SHAPES for F in WIDTHS]


def test_powerlaw_reaches_wave_tasks_and_fixups_on_both_hops(case):
    c = case("powerlaw")
    info = c.plan.info
    assert min(info["tasks"]) > 0 and min(info["fixups"]) > 0, info
    assert (np.diff(c.inc.csrptr) > 512).sum() > 0 and (np.bincount(c.inc.colind, minlength=c.inc.N) > 512).sum() > 0


@pytest.mark.parametrize("shape,F", CELLS + [("cora", "u4"), ("powerlaw", "u32"), ("ragged", "u3")])
def test_bit_exact_against_unweighted_pull(case, shape, F):
    c = case(shape)
    unaligned = isinstance(F, str)
    F = int(F[1:]) if unaligned else F
    X = _x(c, F, unaligned=unaligned)
    ones = torch.ones(c.inc.nnz, device=DEV)
    p2a = torch.full((c.inc.nnz,), 2.0 ** -3, device=DEV)
    p2b = torch.full((c.inc.nnz,), 2.0 ** 5, device=DEV)
    for on in (True, False):
        degE, degV, W = c.scales(on)
        ref = c.plan.aggregate(c.ptr, c.ind, X, degE, degV, W, variant="pull", bind_scales=False)
        got_null = c.plan.aggregate_incidence(c.ptr, c.ind, X, None, None, degE, degV, W)
        got_ones = c.plan.aggregate_incidence(c.ptr, c.ind, X, ones, ones, degE, degV, W)
        got_ones2 = c.plan.aggregate_incidence(c.ptr, c.ind, X, ones, ones, degE, degV, W)
        got_p2 = c.plan.aggregate_incidence(c.ptr, c.ind, X, p2a, p2b, degE, degV, W)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got_null), _bits(ref)), "NULL weights differ from the unweighted pull (scales %s)" % on
        assert torch.equal(_bits(got_ones), _bits(ref)), "unit weights differ from the unweighted pull (scales %s)" % on
        assert torch.equal(_bits(got_ones2), _bits(got_ones)), "two calls differ"
        assert torch.equal(_bits(got_p2), _bits(ref * 4)), "2^-3 / 2^5 weights are not exactly 4x (scales %s)" % on


@pytest.mark.parametrize("shape", ["cora", "powerlaw"])
def test_graph_replay_equals_eager(case, shape):
    c = case(shape)
    F = 32
    X = _x(c, F, seed=3)
    degE, degV, W = c.scales(True)
    Y = torch.empty(c.inc.N, F, device=DEV)
    Xe = torch.empty(c.inc.M, F, device=DEV)
    ws = torch.empty(max(c.plan.incidence_workspace_bytes(F), 256), dtype=torch.uint8, device=DEV)
    run = lambda: c.plan.aggregate_incidence(c.ptr, c.ind, X, c.v2e, c.e2v, degE, degV, W, xe_out=Xe, out=Y,  # noqa: E731
                                             workspace=ws)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # warm-up: builds and uploads the permutation
    torch.cuda.current_stream().wait_stream(s)
    eager, eager_xe = Y.clone(), Xe.clone()
    Y.zero_()
    Xe.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(Y), _bits(eager)) and torch.equal(_bits(Xe), _bits(eager_xe))


@pytest.mark.parametrize("shape,F", CELLS)
def test_accuracy_against_float64(case, shape, F):
    c = case(shape)
    X = _x(c, F, seed=1)
    for on in (True, False):
        graph = c.graph(on)
        degE, degV, W = c.scales(on)
        for v2e, e2v, what in ((c.v2e, c.e2v, "both"), (c.v2e, None, "v2e"), (None, c.e2v, "e2v")):
            got = c.plan.aggregate_incidence(c.ptr, c.ind, X, v2e, e2v, degE, degV, W)
            ins = {"x": X, "v2e": v2e, "e2v": e2v}
            out, _, mass, _ = gr.evaluate(ir.fn, graph, ins, torch.zeros(c.inc.N, F), ())
            print("%s F=%d scales=%s %s: max |err| / mass %.3g" % (
                shape, F, on, what, float(((gr.f64(got) - out).abs() / mass.clamp(min=gr.TINY)).max())))
            gr.assert_within(got, out, mass, gr.FP32_C, "%s F=%d scales=%s weights=%s" % (shape, F, on, what))


@pytest.mark.parametrize("shape,F", CELLS)
def test_gradients_against_float64(hg, case, shape, F):
    c = case(shape)
    X = _x(c, F, seed=2).requires_grad_(True)
    v2e, e2v = c.v2e.clone().requires_grad_(True), c.e2v.clone().requires_grad_(True)
    g = _x(c, F, seed=5)
    degE, degV, W = c.scales(True)
    Y = hg.ops.incidence_aggr(c.ptr, c.ind, X, v2e, e2v, degE, degV, W)
    dX, dv, de = torch.autograd.grad(Y, (X, v2e, e2v), g)
    out, grads, out_mass, grad_mass = gr.evaluate(ir.fn, c.graph(True), {"x": X, "v2e": v2e, "e2v": e2v}, g,
                                                  ("x", "v2e", "e2v"))
    c_w = gr.FP32_C + (F + 1) * U
    for name, got, cc in (("x", dX, gr.FP32_C), ("v2e", dv, c_w), ("e2v", de, c_w)):
        print("%s F=%d d%s: max |err| / mass %.3g (bound %.3g)" % (shape, F, name, float(
            ((gr.f64(got) - grads[name]).abs() / grad_mass[name].clamp(min=gr.TINY)).max()), cc))
    gr.assert_within(Y, out, out_mass, gr.FP32_C, "%s F=%d out" % (shape, F))
    gr.assert_within(dX, grads["x"], grad_mass["x"], gr.FP32_C, "%s F=%d dX" % (shape, F))
    gr.assert_within(dv, grads["v2e"], grad_mass["v2e"], c_w, "%s F=%d dv2e" % (shape, F))
    gr.assert_within(de, grads["e2v"], grad_mass["e2v"], c_w, "%s F=%d de2v" % (shape, F))


@pytest.mark.parametrize("shape,F", CELLS + [("pubmed", "u33")])
def test_incidence_dot_against_float64(case, shape, F):
    c = case(shape)
    unaligned = isinstance(F, str)
    F = int(F[1:]) if unaligned else F
    A = _x(c, F, seed=6, unaligned=unaligned)
    g = torch.Generator(device=DEV).manual_seed(7)
    B = torch.randn(c.inc.M, F, device=DEV, generator=g)
    graph = c.graph(False)
    got = c.plan.incidence_dot(c.ptr, c.ind, A, B)
    again = c.plan.incidence_dot(c.ptr, c.ind, A, B)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(again)), "incidence_dot is not deterministic"
    cc = max(gr.FP32_C, (F + 2) * U)
    gr.assert_within(got, ir.dot(graph, A, B), ir.dot_mass(graph, A, B), cc, "%s F=%d incidence_dot" % (shape, F))


class _Attention(torch.nn.Module):
    """Scores from torch ops, then the weighted aggregation with the coefficients in both hops:
    a(v, e) = sigmoid(<X[v] Wlin^T, att> + bias[e]),  Y = incidence_aggr(X Wlin^T, a, a, degE, degV)."""

    def __init__(self, F_in, F_out, M, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.lin = torch.nn.Parameter(torch.rand(F_out, F_in, generator=g) / F_in)
        self.att = torch.nn.Parameter(torch.rand(F_out, generator=g))
        self.bias = torch.nn.Parameter(torch.rand(M, generator=g))

    def forward(self, aggr, V, E, X):
        Z = X @ self.lin.t()
        a = torch.sigmoid((Z @ self.att)[V] + self.bias[E])
        return aggr(Z, a)


@pytest.mark.parametrize("shape", ["cora", "ragged"])
def test_attention_layer_gradients(hg, case, shape):
    """Every input, parameter and output gradient here is non-negative (X, Wlin, att, bias, dY >= 0; sigmoid' > 0), so
    no cancellation occurs and each quantity's mass is its own magnitude: |got - ref| <= c |ref| per element.  The fp32
    path's relative errors add to first order: the aggregation and its backward (FP32_C each), the weight gradients'
    dot products ((F + 1) 2^-24), torch's fp32 sums over at most nnz terms and products over F_in terms in any order
    ((nnz + F_in) 2^-24), and 16 units for the elementwise sigmoid / products."""
    c = case(shape)
    F_in, F_out = 16, 8
    g = torch.Generator().manual_seed(9)
    X32 = torch.rand(c.inc.N, F_in, generator=g)
    dY = torch.rand(c.inc.N, F_out, generator=g)
    V = torch.from_numpy(c.inc.colind.astype(np.int64))
    E = torch.from_numpy(np.repeat(np.arange(c.inc.M), np.diff(c.inc.csrptr)))
    degE, degV, _ = c.scales(True)
    m32 = _Attention(F_in, F_out, c.inc.M).to(DEV)
    m64 = _Attention(F_in, F_out, c.inc.M).to(torch.float64)
    Y = m32(lambda Z, a: hg.ops.incidence_aggr(c.ptr, c.ind, Z, a, a, degE, degV), V.to(DEV), E.to(DEV), X32.to(DEV))
    Y.backward(dY.to(DEV))
    graph64 = gr.Graph(c.inc, degE, degV, None)
    Y64 = m64(lambda Z, a: ir.incidence_aggr(graph64, Z, a, a), V, E, X32.double())
    Y64.backward(dY.double())
    cc = 3 * gr.FP32_C + (F_out + 1 + c.inc.nnz + F_in + 16) * U
    gr.assert_within(Y, Y64.detach(), Y64.detach().abs(), cc, "%s attention out" % shape)
    for (name, p32), p64 in zip(m32.named_parameters(), m64.parameters()):
        ref = p64.grad
        err = float(((gr.f64(p32.grad) - ref).abs() / ref.abs().clamp(min=gr.TINY)).max())
        print("%s attention d%s: max relative error %.3g (bound %.3g)" % (shape, name, err, cc))
        gr.assert_within(p32.grad, ref, ref.abs(), cc, "%s attention d%s" % (shape, name))


def test_refused_inputs(hg, case):
    c = case("cora")
    ops = hg.ops
    X = _x(c, 8)
    w = torch.ones(c.inc.nnz, device=DEV)
    for variant in ("fused", "push_atomic", "push_groups"):
        with pytest.raises(ValueError):
            ops.incidence_aggr(c.ptr, c.ind, X, w, w, options=ops.Options(variant=variant))
    for variant in ("auto", "pull"):
        ops.incidence_aggr(c.ptr, c.ind, X, w, w, options=ops.Options(variant=variant))
    with pytest.raises(TypeError):
        ops.incidence_aggr(c.ptr, c.ind, X.to(torch.bfloat16), w, w)
    with pytest.raises(ValueError):
        ops.incidence_aggr(c.ptr, c.ind, X, w[:-1], w)
    with pytest.raises(ValueError):
        ops.incidence_aggr(c.ptr, c.ind, X, w, torch.ones(c.inc.nnz + 1, device=DEV))
    with pytest.raises(RuntimeError):
        ops.incidence_aggr(c.ptr, c.ind, X.cpu(), w, w)
    with pytest.raises(RuntimeError):
        ops.incidence_aggr(c.ptr, c.ind, X, w.cpu(), None)
    Y = ops.HGNNAggrIncidence(c.h, X, w, w, c.degE, c.degV, c.W)
    assert torch.equal(_bits(Y), _bits(c.plan.aggregate_incidence(c.ptr, c.ind, X, None, None, c.degE, c.degV, c.W)))
