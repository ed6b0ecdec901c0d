"""Per-incidence logits in the attention softmax, the one-hop weighted gather, the differentiable dot product and the
dot-product layer on the GPU (hg_incidence_attention_entry_*_f32, hg_gather_rows_incidence_heads_f32,
ops.incidence_softmax(incidence_score=...), ops.incidence_gather, ops.incidence_dot, HypergraphAttnConv(score="dot")).
U = 2^-24 throughout; float64 references in tests/_entry_ref.py.

Shapes: the toy graph (duplicate member, empty hyperedge, isolated vertex, one-entry groups); `ragged` (3000 / 2000, 10 %
empty); `boundaries` and its transpose (every kernel threshold +-1, the length 5000 and the long-row workgroups on both
sides); the three width shapes for one exactness check at each lane-group width.  Heads: 1; 3 with C = 5 (4-byte lanes, a
head boundary inside a lane tile); 2 with C = 8 (16-byte lanes).

1. Exact facts, bit for bit, the reference being the existing entry: incidence_score = 0 changes nothing; sv = se = None with
   incidence_score = fl(sv[u] + se[e]) gives the call on (sv, se); both with dropout 0.3 and a fixed state; column h of a
   heads call is the single-head call on column h; two calls agree; one-entry groups are 1.0f; guard words keep their
   sentinel; a graph replay equals eager; d incidence_score is the backward entry's ds_out.
2. alpha against float64 with all three terms: |got - ref| <= c ref, c = (L + 16 + 20 Smax) U (_entry_ref.bound_c), t drawn
   so that no |raw| < 1e-3 (the sign of raw is then the same in fp32 and float64: an fp32 sum of magnitude >= 1e-3 carries
   an error below 2^-22).
3. dsv, dse, dt through torch.autograd.grad against the closed form, at check 4 of test_attention_gpu.py with this c:
   |got - ref| <= (2 c + (L + D + 8) U) max(mass, TINY).
4. incidence_gather: both hops compose to incidence_aggr bit for bit, unweighted equals Plan.gather_rows, gradients against
   float64 at test_incidence_aggr.py's bounds (FP32_C for d src, FP32_C + (C + 1) U for d weight, C the head's width: the
   dot product runs over it).
5. incidence_dot: forward bits of Plan.incidence_dot, dA / dB against float64 at FP32_C of sum |g| |B| / sum |g| |A|.
6. HypergraphAttnConv(score="dot") against the same formulas in float64 (tolerance: see test_dot_layer_against_float64) and
   its dropout: reproducible under torch.manual_seed, the kept pattern that of hg_dropout_keep_host.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402
import _dropout_ref as dr  # noqa: E402
import _entry_ref as er  # noqa: E402
import _grad_ref as gr  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = ar.DEV
U = ar.U
SLOPES = ar.SLOPES
HEADS = (1, 3, 2)
PAIRS = ((1, 8), (3, 5), (2, 8))  # (H, C)

SHAPES = {
    "toy": ar.toy,
    "ragged": lambda: synth.random_incidence(3000, 2000, 6.0, seed=4, empty_frac=0.1),
    "boundaries": ar.boundaries,
    "boundaries_T": lambda: ar.transpose(ar.boundaries()),
    "widths_4": lambda: ar.width_shape(4),
    "widths_8": lambda: ar.width_shape(8),
    "widths_16": lambda: ar.width_shape(16),
}
MAIN = ("toy", "ragged", "boundaries", "boundaries_T")
CELLS = [(s, g) for s in MAIN for g in ar.GROUPS]

_CASES = {}
_bits = ar.bits


class Case(ar.Case):
    """ar.Case with, per head count, fp32 scores scaled to max 4, an entry logit that keeps |raw| >= 1e-3, a signed
    dalpha, and the float64 alpha of the three-term logit: computed once, shared, never modified."""

    def __init__(self, hg, inc, name):
        super().__init__(hg, inc, name)
        self._h3 = {}
        self._ref3 = {}

    def inputs(self, H):
        if H not in self._h3:
            g = torch.Generator().manual_seed(40 + H)
            sv, se = torch.randn(self.inc.N, H, generator=g), torch.randn(self.inc.M, H, generator=g)
            sv, se = sv * (4.0 / float(sv.abs().max())), se * (4.0 / float(se.abs().max()))
            t = er.draw_entry(self.graph, sv, se, H, seed=50 + H)
            assert not bool(((sv == 0) & torch.signbit(sv)).any() | ((se == 0) & torch.signbit(se)).any())  # no -0.0
            dalpha = torch.randn(self.inc.nnz, H, generator=g)
            self._h3[H] = {"sv": sv, "se": se, "t": t, "dalpha": dalpha,
                           "dev": tuple(x.to(DEV) for x in (sv, se, t, dalpha))}
        return self._h3[H]

    def ref3(self, H, group, slope):
        """(alpha float64 [nnz, H], raw float64, Smax)."""
        key = (H, group, slope)
        if key not in self._ref3:
            i = self.inputs(H)
            raw = er.raw64(self.graph, i["sv"], i["se"], i["t"], H)
            assert not bool((raw.abs() < 1e-3).any())
            self._ref3[key] = (er.softmax_raw(self.graph, raw, group, slope), raw, float(raw.abs().max()) if raw.numel() else 0.0)
        return self._ref3[key]


@pytest.fixture
def case(hg):
    def get(name):
        if name not in _CASES:
            _CASES.clear()  # one shape at a time on the device
            torch.cuda.empty_cache()
            _CASES[name] = Case(hg, SHAPES[name](), name)
        return _CASES[name]
    return get


def _rng(seed=0x1234):
    return torch.tensor([0x0123456789ABCDEF, seed], dtype=torch.int64, device=DEV)


def test_shapes_reach_every_path(case):
    for name, side in (("boundaries", "hyperedge"), ("boundaries_T", "vertex")):
        c = case(name)
        assert ar.reaches_every_path(c.plan.segment_info(side), ar.side_lengths(c.inc, side)) is None, name
        assert len(c.plan.segment_info(side)["long_rows"]) > 0
    for w in (4, 8, 16):
        assert case("widths_%d" % w).plan.segment_info("hyperedge")["width"] == w


# ---- 1. exact facts ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,group", CELLS + [("widths_%d" % w, "hyperedge") for w in (4, 8, 16)])
def test_exact_facts(hg, case, shape, group):
    c = case(shape)
    ops = hg.ops
    N, nnz, guard = c.inc.N, c.inc.nnz, 64
    idx, sizes = c.sizes(group)
    V, E = c.graph.V.to(DEV), c.graph.E.to(DEV)
    for H in HEADS:
        sv, se, t, dalpha = c.inputs(H)["dev"]
        kw = dict(group=group, num_nodes=N, heads=H)
        for slope in SLOPES:
            what = "%s %s H=%d slope %g" % (shape, group, H, slope)
            kw["negative_slope"] = slope
            plain = ops.incidence_softmax(c.ptr, c.ind, sv, se, **kw)
            zero = ops.incidence_softmax(c.ptr, c.ind, sv, se, incidence_score=torch.zeros_like(t), **kw)
            assert torch.equal(_bits(zero), _bits(plain)), "incidence_score = 0 changed alpha: " + what
            summed = sv[V] + se[E]  # the fp32 sum, formed in torch
            alone = ops.incidence_softmax(c.ptr, c.ind, None, None, incidence_score=summed, **kw)
            assert torch.equal(_bits(alone), _bits(plain)), "the logit alone differs from sv + se: " + what
            dplain = ops.incidence_softmax(c.ptr, c.ind, sv, se, dropout=0.3, rng_state=_rng(), **kw)
            dzero = ops.incidence_softmax(c.ptr, c.ind, sv, se, incidence_score=torch.zeros_like(t), dropout=0.3,
                                          rng_state=_rng(), **kw)
            dalone = ops.incidence_softmax(c.ptr, c.ind, None, None, incidence_score=summed, dropout=0.3, rng_state=_rng(), **kw)
            assert torch.equal(_bits(dzero), _bits(dplain)) and torch.equal(_bits(dalone), _bits(dplain)), "dropout: " + what
            assert bool((dplain == 0).any()) or nnz < 8
            # the general call: guard words, determinism, one-entry groups, columns
            buf = torch.full(((nnz + 2 * guard) * H,), ar.SENTINEL, device=DEV)
            out = buf[guard * H:(guard + nnz) * H]
            c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope, out=out, heads=H, entry=t)
            again = ops.incidence_softmax(c.ptr, c.ind, sv, se, incidence_score=t, **kw)
            torch.cuda.synchronize()
            assert torch.equal(_bits(out), _bits(again.reshape(-1))), "two calls differ: " + what
            assert bool((buf[:guard * H] == ar.SENTINEL).all()) and bool((buf[(guard + nnz) * H:] == ar.SENTINEL).all()), what
            assert not bool((out == ar.SENTINEL).any()), "a real position was not written: " + what
            got = again.reshape(nnz, H)
            assert bool((got.cpu()[sizes[idx] == 1] == 1.0).all()), "one-entry groups are not exactly 1.0f: " + what
            for h in range(H):
                col = ops.incidence_softmax(c.ptr, c.ind, sv[:, h].contiguous(), se[:, h].contiguous(), group=group,
                                            negative_slope=slope, num_nodes=N, incidence_score=t[:, h].contiguous())
                assert torch.equal(_bits(col), _bits(got[:, h])), "column %d is not the single-head call: %s" % (h, what)
            # d incidence_score is the backward entry's ds_out for the equivalent (sv, se) call
            for pd in (0.0, 0.3):
                leaf = torch.zeros_like(t).requires_grad_(True)
                a = ops.incidence_softmax(c.ptr, c.ind, sv, se, incidence_score=leaf, dropout=pd, rng_state=_rng(), **kw)
                (dt,) = torch.autograd.grad(a, leaf, dalpha.reshape(a.shape))
                if pd:
                    ds = c.plan.incidence_attention_dropout_backward(c.ptr, c.ind, plain, dalpha.reshape(plain.shape), sv, se,
                                                                     group, slope, pd, _rng(), heads=H)[0]
                else:
                    ds = c.plan.incidence_attention_backward(c.ptr, c.ind, plain, dalpha.reshape(plain.shape), sv, se, group,
                                                             slope, heads=H)[0]
                assert torch.equal(_bits(dt.reshape(-1)), _bits(ds.reshape(-1))), "dt is not ds_out (dropout %g): %s" % (pd, what)


@pytest.mark.parametrize("group", ar.GROUPS)
def test_graph_replay_equals_eager(case, group):
    c = case("ragged")
    H = 3
    sv, se, t, dalpha = c.inputs(H)["dev"]
    alpha = torch.empty(c.inc.nnz, H, device=DEV)
    rng = _rng()  # made before the capture: a copy from the host cannot be captured
    outs = {}

    def run():
        c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, 0.2, out=alpha, heads=H, entry=t)
        outs["bwd"] = c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, dalpha, sv, se, group, 0.2, heads=H, entry=t)
        outs["drop"] = c.plan.incidence_attention_dropout(c.ptr, c.ind, sv, se, group, 0.2, 0.3, rng, heads=H, entry=t)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # the warm call: builds and uploads the permutation and the long-row lists
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = [alpha.clone()] + [x.clone() for x in outs["bwd"]] + [x.clone() for x in outs["drop"]]
    alpha.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip([alpha] + list(outs["bwd"]) + list(outs["drop"]), eager):
        assert torch.equal(_bits(got), _bits(want)), group


# ---- 2. and 3. against float64 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,group", CELLS)
def test_alpha_against_float64(hg, case, shape, group):
    c = case(shape)
    for H in HEADS:
        sv, se, t, _ = c.inputs(H)["dev"]
        for slope in SLOPES:
            ref, _, smax = c.ref3(H, group, slope)
            cc = er.bound_c(c.L[group], smax)
            got = gr.f64(hg.ops.incidence_softmax(c.ptr, c.ind, sv, se, group=group, negative_slope=slope, num_nodes=c.inc.N,
                                                  heads=H, incidence_score=t)).reshape(ref.shape)
            rel = float(((got - ref).abs() / ref).max()) if ref.numel() else 0.0
            print("%s %s H=%d slope %g: max |err| / alpha %.3g (bound %.3g, L %d, Smax %.2f)" % (
                shape, group, H, slope, rel, cc, c.L[group], smax))
            assert smax <= 12.0
            assert bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= cc * ref).all()), (shape, group, H, slope)


@pytest.mark.parametrize("shape,group", CELLS)
def test_gradients_against_float64(hg, case, shape, group):
    c = case(shape)
    D = {"ds": 0, "dsv": c.L["vertex"], "dse": c.L["hyperedge"], "dt": 0}
    for H in HEADS:
        sv, se, t, dalpha = c.inputs(H)["dev"]
        da = gr.f64(dalpha)
        for slope in SLOPES:
            ref_alpha, raw, smax = c.ref3(H, group, slope)
            cc = er.bound_c(c.L[group], smax)
            want = dict(zip(("ds", "dsv", "dse", "dt"), er.closed_form_backward(c.graph, raw, group, slope, ref_alpha, da)))
            m = er.backward_masses(c.graph, group, slope, ref_alpha, da)
            mass = {"ds": m[0], "dsv": m[1], "dse": m[2], "dt": m[0]}
            leaves = [x.clone().requires_grad_(True) for x in (sv, se, t)]
            out = hg.ops.incidence_softmax(c.ptr, c.ind, leaves[0], leaves[1], group=group, negative_slope=slope,
                                           num_nodes=c.inc.N, heads=H, incidence_score=leaves[2])
            got = dict(zip(("dsv", "dse", "dt"), torch.autograd.grad(out, leaves, dalpha.reshape(out.shape))))
            what = "%s %s H=%d slope %g" % (shape, group, H, slope)
            for name in ("dsv", "dse", "dt"):
                bound = 2 * cc + (c.L[group] + D[name] + 8) * U
                g = got[name].reshape(want[name].shape)
                err = float(((gr.f64(g) - want[name]).abs() / mass[name].clamp(min=gr.TINY)).max()) if g.numel() else 0.0
                print("%s %s: max |err| / mass %.3g (bound %.3g)" % (what, name, err, bound))
                gr.assert_within(g, want[name], mass[name], bound, what + " " + name)


# ---- 4. incidence_gather ----------------------------------------------------------------------------------------------------

def _gather_inputs(c, H, C, seed):
    g = torch.Generator().manual_seed(seed)
    inc = c.inc
    sizes = np.diff(inc.csrptr).astype(np.float32)
    with np.errstate(divide="ignore"):
        degE = torch.from_numpy(1.0 / sizes)  # inf on an empty hyperedge: never applied
    return {"X": torch.randn(inc.N, H * C, generator=g).to(DEV), "Xe": torch.randn(inc.M, H * C, generator=g).to(DEV),
            "w": torch.randn(inc.nnz, H, generator=g).to(DEV), "w2": torch.randn(inc.nnz, H, generator=g).to(DEV),
            "degE": degE.to(DEV), "W": (torch.rand(inc.M, generator=g) + 0.5).to(DEV),
            "degV": (torch.rand(inc.N, generator=g) + 0.5).to(DEV),
            "gE": torch.randn(inc.M, H * C, generator=g).to(DEV), "gV": torch.randn(inc.N, H * C, generator=g).to(DEV),
            "sE": torch.randn(inc.M, generator=g).to(DEV), "sV": torch.randn(inc.N, generator=g).to(DEV)}


@pytest.mark.parametrize("shape", MAIN)
def test_gather_composes_to_incidence_aggr(hg, case, shape):
    c = case(shape)
    ops = hg.ops
    for H, C in PAIRS:
        i = _gather_inputs(c, H, C, seed=60 + H)
        what = "%s H=%d C=%d" % (shape, H, C)
        xe_ref = torch.empty(c.inc.M, H * C, device=DEV)
        y_ref = c.plan.aggregate_incidence(c.ptr, c.ind, i["X"], i["w"], i["w2"], i["degE"], i["degV"], i["W"], xe_out=xe_ref,
                                           heads=H)
        y_op = ops.incidence_aggr(c.ptr, c.ind, i["X"], i["w"], i["w2"], i["degE"], i["degV"], i["W"], heads=H)
        xe = ops.incidence_gather(c.ptr, c.ind, i["X"], i["w"], to="hyperedge", scale_a=i["degE"], scale_b=i["W"], heads=H)
        y = ops.incidence_gather(c.ptr, c.ind, xe, i["w2"], to="vertex", scale_a=i["degV"], heads=H, num_nodes=c.inc.N)
        again = ops.incidence_gather(c.ptr, c.ind, xe, i["w2"], to="vertex", scale_a=i["degV"], heads=H)  # N from the scale
        torch.cuda.synchronize()
        assert xe.shape == xe_ref.shape and torch.equal(_bits(xe), _bits(xe_ref)), "hop 0 is not xe_out: " + what
        assert torch.equal(_bits(y), _bits(y_ref)) and torch.equal(_bits(y), _bits(y_op)), "hop 0 + hop 1 is not Y: " + what
        assert torch.equal(_bits(y), _bits(again)), "two calls differ: " + what
        for hop, to, src in ((0, "hyperedge", i["X"]), (1, "vertex", i["Xe"])):
            plain = ops.incidence_gather(c.ptr, c.ind, src, None, to=to, num_nodes=c.inc.N)
            assert torch.equal(_bits(plain), _bits(c.plan.gather_rows(hop, c.ptr, c.ind, src))), "unweighted %s: %s" % (to, what)


@pytest.mark.parametrize("shape", MAIN)
def test_gather_gradients_against_float64(hg, case, shape):
    c = case(shape)
    for H, C in PAIRS:
        i = _gather_inputs(c, H, C, seed=70 + H)
        c_w = gr.FP32_C + (C + 1) * U
        for to, src, sa, sb, g in (("hyperedge", i["X"], i["sE"], i["W"], i["gE"]), ("vertex", i["Xe"], i["sV"], None, i["gV"])):
            for w in (i["w"], None):
                s = src.clone().requires_grad_(True)
                wl = None if w is None else w.clone().requires_grad_(True)
                out = hg.ops.incidence_gather(c.ptr, c.ind, s, wl, to=to, scale_a=sa, scale_b=sb, heads=H, num_nodes=c.inc.N)
                wrt = ("src",) if w is None else ("src", "w")
                grads = dict(zip(wrt, torch.autograd.grad(out, [s] if w is None else [s, wl], g)))
                ref, rg, mass, mg = gr.evaluate(er.gather, c.graph, {"src": src, "w": w, "sa": sa, "sb": sb, "to": to, "heads": H},
                                                g, wrt)
                what = "%s H=%d C=%d to=%s%s" % (shape, H, C, to, "" if w is not None else " unweighted")
                gr.assert_within(out, ref, mass, gr.FP32_C, what + " out")
                for name, cc in (("src", gr.FP32_C), ("w", c_w)):
                    if name in grads:
                        err = float(((gr.f64(grads[name]) - rg[name]).abs() / mg[name].clamp(min=gr.TINY)).max())
                        print("%s d%s: max |err| / mass %.3g (bound %.3g)" % (what, name, err, cc))
                        gr.assert_within(grads[name], rg[name], mg[name], cc, what + " d" + name)


# ---- 5. incidence_dot -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", MAIN)
def test_dot_forward_bits_and_gradients(hg, case, shape):
    c = case(shape)
    for H, C in PAIRS:
        i = _gather_inputs(c, H, C, seed=80 + H)
        A, B = i["X"].clone().requires_grad_(True), i["Xe"].clone().requires_grad_(True)
        what = "%s H=%d C=%d" % (shape, H, C)
        out = hg.ops.incidence_dot(c.ptr, c.ind, A, B, heads=H)
        assert out.grad_fn is not None and hg.ops.incidence_dot(c.ptr, c.ind, i["X"], i["Xe"], heads=H).grad_fn is None
        want = c.plan.incidence_dot(c.ptr, c.ind, i["X"], i["Xe"], heads=H)
        assert out.shape == want.shape and torch.equal(_bits(out.detach()), _bits(want)), "forward bits: " + what
        g = i["w"] if H > 1 else i["w"].reshape(-1)
        dA, dB = torch.autograd.grad(out, (A, B), g)
        only_a = torch.autograd.grad(hg.ops.incidence_dot(c.ptr, c.ind, A, i["Xe"], heads=H), A, g)[0]
        assert torch.equal(_bits(only_a), _bits(dA)), what
        _, rg, _, mg = gr.evaluate(lambda graph, a, b: er.dot(graph, a, b, H), c.graph, {"a": i["X"], "b": i["Xe"]},
                                   i["w"], ("a", "b"))  # the masses: sum |g| |B| for dA, sum |g| |A| for dB
        for name, got in (("a", dA), ("b", dB)):
            err = float(((gr.f64(got) - rg[name]).abs() / mg[name].clamp(min=gr.TINY)).max())
            print("%s d%s: max |err| / mass %.3g (bound %.3g)" % (what, name.upper(), err, gr.FP32_C))
            gr.assert_within(got, rg[name], mg[name], gr.FP32_C, what + " d" + name.upper())


# ---- 6. the layer -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("group", ar.GROUPS)
@pytest.mark.parametrize("shape", ["toy", "ragged"])
def test_dot_layer_against_float64(hg, case, shape, group, heads):
    """X, every parameter and dY are non-negative, so the logits are non-negative (the leaky relu is the identity on them)
    and outside the softmax backward nothing cancels: Y's mass is |Y|, and a parameter gradient's mass is what autograd
    accumulates when the softmax backward returns mass_ds (check 3) instead of ds (_entry_ref._MassSoftmax).
    |got - ref| <= cc max(mass, TINY), cc composed as test_attention_gpu.py's test_layer_against_float64 composes its own,
    the first-order sum of
      * that test's terms for the aggregation, its backward and torch's fp32 ops around it:
        3 FP32_C + (F_out + 1 + nnz + F_in + 16) U, F_out = H C;
      * the logits: an fp32 dot product over C terms of a row of Z (dot products over F_in terms) with a row of Ke (a mean
        over at most Lh members of rows of Kv, dot products over F_in terms), scaled once: absolute error at most
        Smax (2 F_in + C + Lh + 4) U, in an exponent of the numerator and of the denominator:
        2 Smax (2 F_in + C + Lh + 4) U;
      * alpha itself, check 2's c = (L + 16 + 20 Smax) U (an upper bound here: sv = se = None adds +0 exactly), once in each
        hop: 2 c;
      * the softmax backward, check 3 for dt (no further reduction: D = 0): 2 c + (L + 8) U;
      * what dt then runs through: the scaling by C^-1/2, the dot's backward (two weighted hops) and the member mean's
        backward (one unweighted hop), each an aggregation kernel at FP32_C: 3 FP32_C + 2 U."""
    c = case(shape)
    F_in, C, slope = 12, 4, 0.2
    F_out = heads * C
    g = torch.Generator().manual_seed(9)
    X32 = torch.rand(c.inc.N, F_in, generator=g)
    dY = torch.rand(c.inc.N, F_out, generator=g)
    params = {"lin.weight": torch.rand(F_out, F_in, generator=g) / F_in, "lin_k.weight": torch.rand(F_out, F_in, generator=g) / F_in,
              "bias": torch.rand(F_out, generator=g)}
    layer = hg.HypergraphAttnConv(c.h, F_in, C, group=group, negative_slope=slope, heads=heads, score="dot", dropout=0.5).to(DEV)
    assert sorted(n for n, _ in layer.named_parameters()) == sorted(params)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            p.copy_(params[name])
    layer.eval()
    Y = layer(X32.to(DEV))
    Y.backward(dY.to(DEV))
    graph64 = gr.Graph(c.inc, c.h.degE.reshape(-1), c.h.degV.reshape(-1), None)

    def run64(mass):
        leaves = {k: v.double().requires_grad_(True) for k, v in params.items()}
        out, logits = er.dot_conv(graph64, X32.double(), leaves["lin.weight"], leaves["lin_k.weight"], leaves["bias"], group,
                                  slope, heads, True, mass=mass)
        grads = torch.autograd.grad(out, list(leaves.values()), dY.double())
        return out.detach(), dict(zip(leaves, grads)), logits
    Y64, ref, logits = run64(False)
    _, mass, _ = run64(True)
    smax = float(logits.max()) if logits.numel() else 0.0
    assert bool((logits >= 0).all())
    Lh = c.L["hyperedge"]
    c_alpha = er.bound_c(c.L[group], smax)
    cc = (3 * gr.FP32_C + (F_out + 1 + c.inc.nnz + F_in + 16) * U + 2 * smax * (2 * F_in + C + Lh + 4) * U + 2 * c_alpha
          + 2 * c_alpha + (c.L[group] + 8) * U + 3 * gr.FP32_C + 2 * U)
    what = "%s %s H=%d dot layer" % (shape, group, heads)
    gr.assert_within(Y, Y64, Y64.abs(), cc, what + " out")
    for name, p in layer.named_parameters():
        err = float(((gr.f64(p.grad) - ref[name]).abs() / mass[name].clamp(min=gr.TINY)).max())
        print("%s d%s: max |err| / mass %.3g (bound %.3g)" % (what, name, err, cc))
        assert bool((mass[name] >= ref[name].abs() * (1 - 1e-12)).all())
        gr.assert_within(p.grad, ref[name], mass[name], cc, what + " d" + name)
    # the hyperedge embeddings are a public output: the member mean of lin_k(X), 0 for an empty hyperedge
    ke = layer.hyperedge_keys(X32.to(DEV)).detach()
    empty = torch.from_numpy(np.diff(c.inc.csrptr) == 0)
    assert ke.shape == (c.inc.M, F_out) and bool((ke.cpu()[empty] == 0).all())


@pytest.mark.parametrize("heads", [1, 2])
def test_dot_layer_dropout(hg, case, heads):
    c = case("ragged")
    F_in, C, pd = 12, 4, 0.5
    torch.manual_seed(5)
    X = torch.rand(c.inc.N, F_in, device=DEV)
    layer = hg.HypergraphAttnConv(c.h, F_in, C, group="vertex", heads=heads, score="dot", dropout=pd).to(DEV)
    layer.train()
    torch.manual_seed(11)
    y1 = layer(X)
    y2 = layer(X)
    torch.manual_seed(11)
    y3 = layer(X)
    assert torch.equal(_bits(y1.detach()), _bits(y3.detach())), "not reproducible under torch.manual_seed"
    assert not torch.equal(_bits(y1.detach()), _bits(y2.detach())), "two consecutive calls drew the same mask"
    y1.square().sum().backward()
    for name, p in layer.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), name
    # the kept pattern: the state the layer drew after the seed is the first thing it took from torch's generator
    with torch.no_grad():
        Z = layer.lin(X)
        torch.manual_seed(11)
        dropped = layer.coefficients(Z, X).reshape(c.inc.nnz, heads)
        torch.manual_seed(11)
        info = torch.iinfo(torch.int64)
        state = torch.randint(info.min, info.max, (2,), dtype=torch.int64, device=DEV)
        layer.eval()
        alpha = layer.coefficients(Z, X).reshape(c.inc.nnz, heads)
    keep = torch.from_numpy(dr.keep_of_state(state, pd, c.inc.nnz, heads))
    assert bool((alpha > 0).all())
    assert torch.equal(dropped.cpu() != 0, keep), "the kept pattern is not hg_dropout_keep_host's for the drawn state"
    scaled = alpha.cpu() * torch.tensor(float(dr.scale(pd)))
    assert torch.equal(_bits(dropped.cpu()[keep]), _bits(scaled[keep]))
    # the same through the operator, which returns its state
    out, st = hg.ops.incidence_softmax(c.ptr, c.ind, None, None, group="vertex", num_nodes=c.inc.N, heads=heads, dropout=pd,
                                       incidence_score=torch.zeros(c.inc.nnz, heads, device=DEV), return_rng_state=True)
    assert torch.equal(out.reshape(c.inc.nnz, heads).cpu() != 0, torch.from_numpy(dr.keep_of_state(st, pd, c.inc.nnz, heads)))
