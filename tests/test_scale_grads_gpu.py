"""The gradients of the scales degE, degV and W on the GPU (hg_hyperedge_dot_heads_f32, hg_rows_dot_f32, ops).

1. Plan.hyperedge_dot against float64 with A != B and wa != wb (signed weights with exact zeros), per element within
   c max(mass, TINY), c = 2 FP32_C + (F + 2) 2^-24: each of the two hyperedge sums carries the library's any-order bound
   FP32_C, the dot over F columns its recursive-summation bound (F - 1 additions, F products, the weights' fma).  The
   mass is the same expression on absolute values.  Empty hyperedges give exactly +0.0.
2. Exact properties: two calls agree, exchanging (A, wa) with (B, wb) changes no bit, A * 2^k scales the result exactly,
   B = 0 gives zeros, a captured replay equals the eager call.
3. Autograd: dW / ddegE within c + 2^-24 (the partner's product), ddegV within FP32_C + (F + 1) 2^-24 (Z at the any-order
   bound, then a dot over F columns), dX bit-identical to the call where no scale requires a gradient; every subset of
   the three scales; an empty hyperedge with degE = inf gives exactly 0.
4. The two layers with learn_hyperedge_weight=True against the same layer in float64 torch; an SGD step; a captured step.

The float64 references are evaluated on the device (tests/_scale_grad_ref.py is device-agnostic): the power-law shape at
F = 260 would take seconds on the host.
"""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402
import _grad_ref as gr  # noqa: E402
import _scale_grad_ref as sr  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
F64 = torch.float64
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
WIDTHS = (1, 3, 4, 8, 16, 32, 33, 64, 128, 260)


def crafted():
    """N = 1200, one hyperedge of every length in LENGTHS: every lane-group width is crossed and 128 / 129 straddle the
    lane-group / workgroup boundary."""
    rng = np.random.default_rng(5)
    rows = [np.sort(rng.choice(1200, n, replace=False)).astype(np.int32) for n in LENGTHS]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return synth.Incidence(1200, len(rows), ptr, np.concatenate(rows).astype(np.int32), name="crafted")


SHAPES = {
    "crafted": crafted,
    "ragged": lambda: synth.random_incidence(3000, 2000, 6.0, seed=4, empty_frac=0.1),
    "powerlaw": lambda: synth.powerlaw(50_000, 200_000),
    "cora": synth.cora_shape,
}


class _Case:
    def __init__(self, hg, name):
        self.inc = inc = SHAPES[name]()
        self.h = hg.HyperGraph.from_incidence(inc, DEV, data_name=name)
        self.ptr, self.ind = self.h.H_T_csrptr, self.h.H_T_colind
        from hypergef_amd.plan import cached_plan
        self.plan = cached_plan(inc.N, self.ptr, self.ind)
        self.idx = sr.Index(inc, DEV)
        rng = np.random.default_rng(11)
        self.W = torch.from_numpy(rng.random(inc.M).astype(np.float32) + 0.5).to(DEV)
        self.degE, self.degV = self.h.degE.reshape(-1), self.h.degV.reshape(-1)  # degE = inf on empty hyperedges
        self.sizes = np.diff(inc.csrptr)
        self._w = {}

    def weights(self, heads):
        """Two distinct signed weight arrays [nnz, heads] with exact zeros."""
        if heads not in self._w:
            rng = np.random.default_rng(100 + heads)
            w = rng.standard_normal((2, self.inc.nnz, heads)).astype(np.float32)
            w[rng.random(w.shape) < 0.1] = 0.0
            self._w[heads] = tuple(torch.from_numpy(r.copy()).to(DEV) for r in w)
        return self._w[heads]


_CASES = {}


@pytest.fixture
def case(hg):
    def get(name):
        if name not in _CASES:
            _CASES.clear()  # one shape at a time on the device
            torch.cuda.empty_cache()
            _CASES[name] = _Case(hg, name)
        return _CASES[name]
    return get


def _rand(rows, F, seed, unaligned=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if unaligned:  # a contiguous view 4 bytes past an allocation: 4-byte lanes only
        x = torch.randn(rows * F + 1, device=DEV, generator=g)[1:].view(rows, F)
        assert x.data_ptr() % 16 == 4
        return x
    return torch.randn(rows, F, device=DEV, generator=g)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _d(t):
    return None if t is None else t.detach().to(F64)


def _report(what, got, ref, mass, c):
    err = float(((_d(got).to(ref.device).reshape(ref.shape) - ref).abs() / mass.clamp(min=gr.TINY)).max()) if ref.numel() else 0.0
    print("%s: max |err| / mass %.3g (bound %.3g)" % (what, err, c))
    gr.assert_within(got, ref, mass, c, what)


def test_shapes_reach_every_path(case):
    c = case("crafted")
    assert tuple(c.sizes) == LENGTHS
    info = c.plan.segment_info("hyperedge")
    assert info["long"] == 128 and sorted(c.sizes[info["long_rows"]]) == [129, 255, 256, 257, 1000]
    p = case("powerlaw")
    assert (p.sizes > 512).sum() > 0 and len(p.plan.segment_info("hyperedge")["long_rows"]) == (p.sizes > 128).sum()
    r = case("ragged")
    assert (r.sizes == 0).sum() > 0 and bool(torch.isinf(r.degE[torch.from_numpy(r.sizes == 0).to(DEV)]).all())
    assert (np.bincount(r.inc.colind, minlength=r.inc.N) == 0).sum() > 0  # isolated vertices


# ---- 1. the kernel against float64 ------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", WIDTHS + ("u32", "u33"))
@pytest.mark.parametrize("shape", ["crafted", "ragged", "powerlaw"])
def test_hyperedge_dot_against_float64(case, shape, F):
    c = case(shape)
    unaligned = isinstance(F, str)
    F = int(F[1:]) if unaligned else F
    A = _rand(c.inc.N, F, 1, unaligned)
    B = _rand(c.inc.N, F, 2, unaligned)
    empty = torch.from_numpy(c.sizes == 0).to(DEV)
    bound = 2 * gr.FP32_C + (F + 2) * U
    for heads in (1, 4):
        if F % heads:
            continue
        wa, wb = c.weights(heads)
        for a_w, b_w, what in ((wa, wb, "both"), (None, None, "unit"), (wa, None, "wa"), (None, wb, "wb")):
            got = c.plan.hyperedge_dot(c.ptr, c.ind, A, B, a_w, b_w, heads=heads)
            assert got.shape == (c.inc.M,) and got.dtype == torch.float32
            ref = sr.edge_dot(c.idx, _d(A), _d(a_w), _d(B), _d(b_w), heads)
            mass = sr.edge_dot(c.idx, _d(A).abs(), None if a_w is None else _d(a_w).abs(), _d(B).abs(),
                               None if b_w is None else _d(b_w).abs(), heads)
            _report("%s F=%d%s heads=%d %s" % (shape, F, " unaligned" if unaligned else "", heads, what), got, ref, mass, bound)
            z = _bits(got[empty])
            assert bool((z == 0).all()), "an empty hyperedge must give +0.0f"


@pytest.mark.parametrize("F", (1, 3, 32, 33, 260))
def test_rows_dot_against_float64(case, F):
    c = case("ragged")
    for unaligned in (False, True):
        A, B = _rand(c.inc.N, F, 3, unaligned), _rand(c.inc.N, F, 4, unaligned)
        got = c.plan.rows_dot(A, B)
        ref = (_d(A) * _d(B)).sum(1)
        _report("rows_dot F=%d unaligned=%s" % (F, unaligned), got, ref, (_d(A) * _d(B)).abs().sum(1), (F + 1) * U)
        assert torch.equal(_bits(got), _bits(c.plan.rows_dot(A, B)))


# ---- 2. exact properties ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F,heads", [(3, 1), (32, 1), (32, 4), (8, 4), (260, 1), (260, 4)])
@pytest.mark.parametrize("shape", ["crafted", "powerlaw"])
def test_exact_properties(case, shape, F, heads):
    c = case(shape)
    A, B = _rand(c.inc.N, F, 5), _rand(c.inc.N, F, 6)
    wa, wb = c.weights(heads)
    run = lambda *a: c.plan.hyperedge_dot(c.ptr, c.ind, *a, heads=heads)  # noqa: E731
    first = run(A, B, wa, wb)
    assert torch.equal(_bits(first), _bits(run(A, B, wa, wb))), "two calls differ"
    assert torch.equal(_bits(first), _bits(run(B, A, wb, wa))), "exchanging (A, wa) with (B, wb) changes bits"
    assert torch.equal(_bits(run(A, B, wa, None)), _bits(run(B, A, None, wa)))
    for k in (3, -5):
        assert torch.equal(_bits(run(A * 2.0 ** k, B, wa, wb)), _bits(first * 2.0 ** k)), "A * 2^%d" % k
    assert bool((run(A, torch.zeros_like(B), wa, wb) == 0).all())
    assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0


@pytest.mark.parametrize("shape", ["crafted", "powerlaw"])
def test_graph_replay_equals_eager(case, shape):
    c = case(shape)
    F, heads = 32, 4
    A, B = _rand(c.inc.N, F, 7), _rand(c.inc.N, F, 8)
    wa, wb = c.weights(heads)
    run = lambda: (c.plan.hyperedge_dot(c.ptr, c.ind, A, B, wa, wb, heads=heads), c.plan.rows_dot(A, B))  # noqa: E731
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = run()  # the warm call: uploads the long-row list
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for t in out:
        t.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[0]), _bits(eager[0])) and torch.equal(_bits(out[1]), _bits(eager[1]))


# ---- 3. autograd -------------------------------------------------------------------------------------------------------

SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(("degE", "degV", "W"), n)]


def _check_scale_grads(c, what, run, x64, F, v2e=None, e2v=None, heads=1, x64_mass=None):
    """run(scales: dict of tensors) -> Y.  Every subset of the scales requires a gradient in turn; dX must keep the bits of
    the call where none does.  x64: the rows the aggregation sees, in float64; x64_mass: their mass (default |x64|)."""
    base = {"degE": c.degE, "degV": c.degV, "W": c.W}
    X = run.X
    Y0 = run(base)
    dY = _rand(c.inc.N, Y0.shape[1], 9).to(Y0.dtype)
    (dX0,) = torch.autograd.grad(Y0, (X,), dY)
    dy64 = _d(dY)
    ref = sr.scale_grads(c.idx, x64, dy64, _d(c.degE), _d(c.degV), _d(c.W), _d(v2e), _d(e2v), heads)
    mass = sr.scale_grad_masses(c.idx, x64 if x64_mass is None else x64_mass, dy64, _d(c.degE), _d(c.degV), _d(c.W),
                                _d(v2e), _d(e2v), heads)
    c_e = 2 * gr.FP32_C + (F + 2) * U + U
    c_v = gr.FP32_C + (F + 1) * U
    empty = torch.from_numpy(c.sizes == 0).to(DEV)
    isolated = torch.from_numpy(np.bincount(c.inc.colind, minlength=c.inc.N) == 0).to(DEV)
    for subset in SUBSETS:
        leaves = {k: (v.clone().requires_grad_(True) if k in subset else v) for k, v in base.items()}
        Y = run(leaves)
        assert torch.equal(_bits(Y), _bits(Y0)), "%s %s: the forward changed" % (what, subset)
        grads = torch.autograd.grad(Y, (X,) + tuple(leaves[k] for k in subset), dY)
        assert torch.equal(_bits(grads[0]), _bits(dX0)), "%s %s: dX changed its bits" % (what, subset)
        for k, got in zip(subset, grads[1:]):
            assert got.dtype == torch.float32 and got.shape == base[k].shape
            _report("%s %s d%s" % (what, "+".join(subset), k), got, ref[k], mass[k], c_v if k == "degV" else c_e)
            if k == "degV":
                assert bool((got[isolated] == 0).all()), "a vertex in no hyperedge gets ddegV = 0"
            else:
                assert bool(torch.isfinite(got).all()) and bool((got[empty] == 0).all()), \
                    "%s d%s: an empty hyperedge (degE = inf) must give exactly 0" % (what, k)


@pytest.mark.parametrize("backward", ["reference", "adjoint"])
@pytest.mark.parametrize("shape", ["ragged", "powerlaw"])
def test_hgnnaggr_scale_gradients(hg, case, shape, backward):
    c = case(shape)
    F = 32
    opt = hg.ops.Options(backward=backward)
    X = _rand(c.inc.N, F, 10).requires_grad_(True)
    run = lambda s: hg.HGNNAggr(c.h, X, s["degE"], s["degV"], s["W"], options=opt)  # noqa: E731
    run.X = X
    _check_scale_grads(c, "%s hgnnaggr %s" % (shape, backward), run, _d(X), F)


@pytest.mark.parametrize("shape", ["ragged", "powerlaw"])
def test_absent_partners(hg, case, shape):
    """W = None: ddegE = q; degE = None: dW = q; no degV: P = dY."""
    c = case(shape)
    F = 16
    X = _rand(c.inc.N, F, 11).requires_grad_(True)
    dY = _rand(c.inc.N, F, 12)
    c_e = 2 * gr.FP32_C + (F + 2) * U + U
    for present in (("degE",), ("W",), ("degE", "degV"), ("degV", "W"), ("degV",)):
        s = {k: (getattr(c, k).clone().requires_grad_(True) if k in present else None) for k in ("degE", "degV", "W")}
        Y = hg.ops.hgnnaggr(c.h.group_key, c.h.group_row, c.h.group_start, c.h.group_end, c.ptr, c.ind, X, s["degE"],
                            s["degV"], s["W"])
        grads = torch.autograd.grad(Y, [s[k] for k in present], dY)
        ref = sr.scale_grads(c.idx, _d(X), _d(dY), _d(s["degE"]), _d(s["degV"]), _d(s["W"]))
        mass = sr.scale_grad_masses(c.idx, _d(X), _d(dY), _d(s["degE"]), _d(s["degV"]), _d(s["W"]))
        for k, got in zip(present, grads):
            _report("%s %s d%s" % (shape, "+".join(present), k), got, ref[k], mass[k],
                    gr.FP32_C + (F + 1) * U if k == "degV" else c_e)


@pytest.mark.parametrize("shape", ["ragged", "powerlaw"])
def test_hgnnaggr_linear_scale_gradients(hg, case, shape):
    """32 -> 32.  The kernels see (X, dT = dY . Wlin) at F_in; the float64 gradient is that of Aggr(X Wlin^T), its mass
    evaluated on |X| |Wlin|^T."""
    c = case(shape)
    F = 32
    g = torch.Generator(device=DEV).manual_seed(13)
    Wlin = (torch.randn(F, F, device=DEV, generator=g) / F ** 0.5).requires_grad_(True)
    X = _rand(c.inc.N, F, 14).requires_grad_(True)
    run = lambda s: hg.ops.hgnnaggr_linear(c.ptr, c.ind, X, Wlin, s["degE"], s["degV"], s["W"])  # noqa: E731
    run.X = X
    _check_scale_grads(c, "%s hgnnaggr_linear" % shape, run, _d(X) @ _d(Wlin).t(), F,
                       x64_mass=_d(X).abs() @ _d(Wlin).abs().t())


@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("shape", ["ragged", "powerlaw"])
def test_incidence_aggr_scale_gradients(hg, case, shape, heads):
    c = case(shape)
    F = 32
    v2e, e2v = c.weights(heads)
    if heads == 1:
        v2e, e2v = v2e.reshape(-1), e2v.reshape(-1)
    X = _rand(c.inc.N, F, 16).requires_grad_(True)
    run = lambda s: hg.ops.incidence_aggr(c.ptr, c.ind, X, v2e, e2v, s["degE"], s["degV"], s["W"], heads=heads)  # noqa: E731
    run.X = X
    _check_scale_grads(c, "%s incidence_aggr heads=%d" % (shape, heads), run, _d(X), F, v2e, e2v, heads)


def test_weight_and_scale_gradients_together(hg, case):
    """v2e, e2v and all three scales in one backward: the weight gradients keep the bits they have alone."""
    c = case("ragged")
    F = 16
    v2e, e2v = (t.reshape(-1).clone().requires_grad_(True) for t in c.weights(1))
    X = _rand(c.inc.N, F, 17).requires_grad_(True)
    dY = _rand(c.inc.N, F, 18)
    Y = hg.ops.incidence_aggr(c.ptr, c.ind, X, v2e, e2v, c.degE, c.degV, c.W)
    alone = torch.autograd.grad(Y, (X, v2e, e2v), dY)
    s = [t.clone().requires_grad_(True) for t in (c.degE, c.degV, c.W)]
    Y = hg.ops.incidence_aggr(c.ptr, c.ind, X, v2e, e2v, *s)
    both = torch.autograd.grad(Y, (X, v2e, e2v) + tuple(s), dY)
    for a, b in zip(alone, both):
        assert torch.equal(_bits(a), _bits(b))
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in both[3:])


def test_bf16_hgnnaggr_scale_gradients(hg, case):
    """bf16 rows: the operands of hyperedge_dot are the widened bf16 values, so dW / ddegE meet the fp32 bound against the
    float64 gradient on those values; Z is a bf16 aggregation (one bf16 rounding of each row): bf16_c(1) + (F + 1) 2^-24."""
    c = case("ragged")
    F = 32
    X = _rand(c.inc.N, F, 19).to(torch.bfloat16).requires_grad_(True)
    dY = _rand(c.inc.N, F, 20).to(torch.bfloat16)
    s = {k: getattr(c, k).clone().requires_grad_(True) for k in ("degE", "degV", "W")}
    Y = hg.HGNNAggr(c.h, X, s["degE"], s["degV"], s["W"])
    assert Y.dtype == torch.bfloat16
    grads = dict(zip(s, torch.autograd.grad(Y, list(s.values()), dY)))
    ref = sr.scale_grads(c.idx, _d(X), _d(dY), _d(c.degE), _d(c.degV), _d(c.W))
    mass = sr.scale_grad_masses(c.idx, _d(X), _d(dY), _d(c.degE), _d(c.degV), _d(c.W))
    c_e = 2 * gr.FP32_C + (F + 2) * U + U
    for k in ("degE", "W"):
        assert grads[k].dtype == torch.float32
        _report("bf16 d%s" % k, grads[k], ref[k], mass[k], c_e)
    assert grads["degV"].dtype == torch.float32
    _report("bf16 ddegV", grads["degV"], ref["degV"], mass["degV"], gr.bf16_c(1) + (F + 1) * U)


def test_trainable_scales_are_never_bound(hg, case):
    """A scale set with a tensor that requires a gradient is not pre-gathered: no binding is made for it, and a binding
    of the constant set stays."""
    c = case("cora")
    F = 32
    X = _rand(c.inc.N, F, 21)
    c.plan.unbind()
    c.plan.aggregate(c.ptr, c.ind, X, c.degE, c.degV, c.W)
    bound = dict(getattr(c.plan, "_bound", {}))
    W = c.W.clone().requires_grad_(True)
    Y = c.plan.aggregate(c.ptr, c.ind, X, c.degE, c.degV, W)
    after = getattr(c.plan, "_bound", {})
    assert set(after) == set(bound) and all(after[k][0] == bound[k][0] for k in bound)
    assert torch.equal(_bits(Y), _bits(c.plan.aggregate(c.ptr, c.ind, X, c.degE, c.degV, c.W, bind_scales=False)))
    # through the operator, with W shaped [M, 1]: inside the autograd Function the flattened view no longer says that it
    # requires a gradient, and the set is still neither bound nor tested for all ones (a device read-back)
    c.plan.aggregate(c.ptr, c.ind, X, c.degE, c.degV, c.W)  # bound again (bind_scales=False above dropped the binding)
    bound = dict(getattr(c.plan, "_bound", {}))
    Wp = torch.nn.Parameter(torch.ones(c.inc.M, 1, device=DEV))
    Xg = X.clone().requires_grad_(True)
    hg.HGNNAggr(c.h, Xg, c.h.degE, c.h.degV, Wp).sum().backward()
    assert Wp.grad is not None and Wp.grad.shape == Wp.shape and Xg.grad is not None
    assert all(k[0] != Wp.data_ptr() for k in getattr(c.plan, "_unit_w", {})), "a trainable W was tested for all ones"
    after = getattr(c.plan, "_bound", {})
    assert set(after) == set(bound) and all(after[k][0] == bound[k][0] for k in bound)


# ---- 4. the layers -----------------------------------------------------------------------------------------------------

def _train_step(layer, opt, X, dY):
    opt.zero_grad(set_to_none=True)
    (layer(X) * dY).sum().backward()
    opt.step()


def _step_and_capture(build, X, dY):
    """One SGD step with lr = 2^-3 moves Wdiag by exactly -lr * grad; a captured step replays with the eager step's bits.
    The layer is a fresh one whose every backward runs on the side stream: autograd runs a parameter's gradient
    accumulation on the stream that was current when the accumulator was made, and one made on the default stream (by a
    backward outside, whose graph is still alive) would draw that stream into the capture."""
    from hypergef_amd import plan as planmod
    lr = 2.0 ** -3
    layer = build()
    opt = torch.optim.SGD(layer.parameters(), lr=lr)
    state0 = {k: v.clone() for k, v in layer.state_dict().items()}

    def restore():
        with torch.no_grad():
            for k, v in layer.state_dict().items():
                v.copy_(state0[k])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _train_step(layer, opt, X, dY)  # warm: everything a first call allocates
        restore()
        _train_step(layer, opt, X, dY)  # the eager step
        grad = layer.Wdiag.grad.clone()
        eager = {k: v.clone() for k, v in layer.state_dict().items()}
        restore()
        opt.zero_grad(set_to_none=True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert float(grad.abs().max()) > 0
    assert torch.equal(_bits(eager["Wdiag"]), _bits(state0["Wdiag"] - lr * grad)), "Wdiag did not move by -lr * grad"
    planmod.clear_pack_cache()  # cached packings are keyed on version counters a replay does not advance
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _train_step(layer, opt, X, dY)
    planmod.clear_pack_cache()
    restore()
    graph.replay()
    torch.cuda.synchronize()
    for k, v in layer.state_dict().items():
        assert torch.equal(_bits(v), _bits(eager[k])), "captured step: %s differs from the eager step" % k
    planmod.clear_pack_cache()


def test_hgnn_layer_with_learned_hyperedge_weight(hg, case):
    """HyperGsysHGNN 32 -> 32 under the adjoint rule (so that every parameter gradient is the true one).  X, the
    parameters and dY are non-negative: nothing cancels, a gradient's mass is its own float64 value.  cc: the aggregation
    and its backward (2 FP32_C), the two hyperedge sums of dWdiag (2 FP32_C, the larger pair), the fp32 products around
    them -- the projection or dT over F columns, the dot over F columns, the weight gradient's contraction over N rows."""
    from hypergef_amd.models import HyperGsysHGNN
    c = case("cora")
    F = 32
    g = torch.Generator().manual_seed(22)
    X = torch.rand(c.inc.N, F, generator=g)
    dY = torch.rand(c.inc.N, F, generator=g)
    params = {"W.weight": torch.rand(F, F, generator=g) / F, "Wdiag": torch.rand(c.inc.M, generator=g) + 0.5}

    def build():
        m = HyperGsysHGNN(c.h, F, F, "sum", options=hg.ops.Options(backward="adjoint"), learn_hyperedge_weight=True).to(DEV)
        with torch.no_grad():
            for name, p in m.named_parameters():
                p.copy_(params[name])
        return m
    layer = build()
    assert sorted(n for n, _ in layer.named_parameters()) == ["W.weight", "Wdiag"]
    Y = layer(X.to(DEV))
    Y.backward(dY.to(DEV))
    idx = sr.Index(c.inc)
    leaves = {k: v.double().requires_grad_(True) for k, v in params.items()}
    out = sr.fn_linear(idx, X.double(), leaves["W.weight"], gr.f64(c.degE), gr.f64(c.degV), leaves["Wdiag"])
    ref = dict(zip(leaves, torch.autograd.grad(out, list(leaves.values()), dY.double())))
    cc = 4 * gr.FP32_C + (3 * F + c.inc.N + 16) * U
    _report("hgnn layer out", Y, out.detach(), out.detach().abs(), cc)
    for name, p in layer.named_parameters():
        _report("hgnn layer d%s" % name, p.grad, ref[name], ref[name].abs(), cc)
    del Y, layer
    _step_and_capture(build, X.to(DEV), dY.to(DEV))


@pytest.mark.parametrize("variant", ["auto", "push_atomic"])
def test_hgnn_layer_learns_hyperedge_weight_under_every_first_aggr(hg, case, variant):
    """HyperGsysHGNN runs the sum operator whatever first_aggr says (HGNNAggr ignores it, as the reference does), on both
    branches of its forward: a learned Wdiag gets the 'sum' layer's gradient, bit for bit, under 'mean' and 'max' too --
    it never lands on the mean / max first aggregations, which give W no gradient."""
    from hypergef_amd.models import HyperGsysHGNN
    c = case("cora")
    F = 32
    X, dY = _rand(c.inc.N, F, 31), _rand(c.inc.N, F, 32)
    grads = {}
    for first_aggr in ("sum", "mean", "max"):
        torch.manual_seed(33)
        m = HyperGsysHGNN(c.h, F, F, first_aggr, options=hg.ops.Options(variant=variant), learn_hyperedge_weight=True).to(DEV)
        m(X).backward(dY)
        assert m.Wdiag.grad is not None and float(m.Wdiag.grad.abs().max()) > 0
        grads[first_aggr] = m.Wdiag.grad
    assert torch.equal(_bits(grads["mean"]), _bits(grads["sum"])) and torch.equal(_bits(grads["max"]), _bits(grads["sum"]))


def test_nonempty_mask_made_in_a_capture_is_not_kept(hg, case):
    """Plan.nonempty_edges keeps its mask with the plan, except one made during a stream capture: that tensor lives in the
    graph's private pool and must not outlive the graph."""
    c = case("ragged")
    from hypergef_amd.plan import Plan
    plan = Plan.from_tensors(c.inc.N, c.ptr, c.ind)
    ref = torch.from_numpy(c.sizes > 0).to(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        inside = plan.nonempty_edges(c.ptr)
    assert plan._nonempty is None
    del inside, graph
    kept = plan.nonempty_edges(c.ptr)
    assert plan._nonempty is kept and plan.nonempty_edges(c.ptr) is kept and torch.equal(kept, ref)


def test_attention_layer_with_learned_hyperedge_weight(hg, case):
    """HypergraphAttnConv 16 -> 8 with Wdiag a parameter, by test_attention_gpu.py's mass rule (non-negative X, parameters
    and dY; the softmax backward returns its masses) and its cc, plus dWdiag's own terms 2 FP32_C + (F_out + 3) 2^-24."""
    c = case("cora")
    F_in, F_out, slope, group = 16, 8, 0.2, "hyperedge"
    g = torch.Generator().manual_seed(23)
    X = torch.rand(c.inc.N, F_in, generator=g)
    dY = torch.rand(c.inc.N, F_out, generator=g)
    params = {"lin.weight": torch.rand(F_out, F_in, generator=g) / F_in, "a_v": torch.rand(F_out, generator=g),
              "a_e": torch.rand(F_out, generator=g), "bias": torch.rand(F_out, generator=g),
              "Wdiag": torch.rand(c.inc.M, generator=g) + 0.5}

    def build():
        m = hg.HypergraphAttnConv(c.h, F_in, F_out, group=group, negative_slope=slope, learn_hyperedge_weight=True).to(DEV)
        with torch.no_grad():
            for name, p in m.named_parameters():
                p.copy_(params[name])
        return m
    layer = build()
    assert sorted(n for n, _ in layer.named_parameters()) == sorted(params)
    Y = layer(X.to(DEV))
    Y.backward(dY.to(DEV))
    idx = sr.Index(c.inc)
    degE, degV = gr.f64(c.degE), gr.f64(c.degV)

    def run64(mass):
        lv = {k: v.double().requires_grad_(True) for k, v in params.items()}
        z = X.double() @ lv["lin.weight"].t()
        sv = z @ lv["a_v"]
        sizes = ar.segment_sum(idx, torch.ones(c.inc.nnz, dtype=F64), "hyperedge")
        inv = torch.where(sizes > 0, 1.0 / sizes.clamp(min=1.0), torch.zeros_like(sizes))
        se = ar.segment_sum(idx, (z @ lv["a_e"])[idx.V], "hyperedge") * inv
        alpha = ar._MassSoftmax.apply(sv, se, idx, group, slope) if mass else ar.softmax(idx, sv, se, group, slope)
        out = sr.fn(idx, z, degE, degV, lv["Wdiag"], alpha, alpha) + lv["bias"]
        return out.detach(), dict(zip(lv, torch.autograd.grad(out, list(lv.values()), dY.double())))
    Y64, ref = run64(False)
    _, mass = run64(True)
    z = X.double() @ params["lin.weight"].double().t()
    smax = float((z @ params["a_v"].double()).max() + (z @ params["a_e"].double()).max())
    Lh, Lv = ar.longest(c.inc, "hyperedge"), ar.longest(c.inc, "vertex")
    c_alpha = (Lh + 16 + 16 * smax) * U
    cc = (3 * gr.FP32_C + (F_out + 1 + c.inc.nnz + F_in + 16) * U + 2 * smax * (F_in + F_out + Lh + 4) * U + 2 * c_alpha
          + 2 * c_alpha + (Lh + Lv + Lh + 8) * U) + 2 * gr.FP32_C + (F_out + 3) * U
    _report("attention layer out", Y, Y64, Y64.abs(), cc)
    for name, p in layer.named_parameters():
        assert bool((mass[name] >= ref[name].abs() * (1 - 1e-12)).all())
        _report("attention layer d%s" % name, p.grad, ref[name], mass[name], cc)
    del Y, layer
    _step_and_capture(build, X.to(DEV), dY.to(DEV))
