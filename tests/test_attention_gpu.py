"""The hypergraph attention coefficients on the GPU (hg_incidence_attention_f32 / _bwd_f32, hg_incidence_sum_f32,
ops.incidence_softmax, ops.incidence_sum, models.HypergraphAttnConv), for both groups, with sv only, se only and both, at
slopes 0.2 and 1.0, against the float64 reference of tests/_attention_ref.py.  U = 2^-24 throughout.

Shapes: the toy graph of the host tests; `ragged` (10 % empty hyperedges); `cora`; `boundaries` -- one hyperedge of every
size 0 .. 70, 255 .. 257, 1023 .. 1025, 5000 and every threshold of the kernels +-1 (lane-group width x entries kept in
registers; the longest row a lane group takes; 256 lanes x entries kept) -- and its transpose, so that the vertex side
crosses the same sizes; `powerlaw(50_000, 200_000)` with long rows on both sides.

1. Exact facts: two calls agree bit for bit; one-entry groups are 1.0f; only the nnz real positions are written (guard
   words around the output keep their sentinel, every position inside loses it); a hipGraph replay equals the eager call.
2. alpha against float64, per element and relative to alpha itself (all terms are positive, so an element's mass is its
   value): |got - ref| <= c ref, c = (L + 16 + 16 Smax) U, L the longest group of the side, Smax = max |raw|.
   Derivation: the fp32 sum sv + se, the leaky product, the subtraction of the maximum and the exponent's argument scaling
   each put at most about 2 Smax U into an exponent -- in the numerator and in every term of the denominator: 16 Smax U;
   the two exponentials contribute 2 ulp each; an L-term positive sum in any order (L - 1) U; one division.  The sign of
   raw in fp32 equals its sign in float64 (a sum of two floats rounds to zero only if it is zero), so both take the same
   leaky branch.  The reference reads the same fp32 sv / se.
3. Range: scores of magnitude 1e4 give finite output; every non-empty group sums to 1 within (2 L + 16) U; the entry
   holding a group's maximum has alpha >= 1 / L (checked against the group's own length, the sharper statement).
4. Gradients: ds, dsv, dse of Plan.incidence_attention_backward and dsv, dse through torch.autograd.grad of
   ops.incidence_softmax, dalpha signed: |got - ref| <= (2 c + (L + D + 8) U) max(mass, TINY) with
   mass_ds[p] = alpha[p] (|dalpha[p]| + sum_g alpha |dalpha|) max(1, slope), mass_dsv / mass_dse its segment sums, c from
   check 2 and D the longest segment of the reducing side (0 for ds itself).
5. incidence_sum alone: both sides, signed values, within (D + 2) U of sum |val|; two calls bit-equal.
6. HypergraphAttnConv against the same layer in float64 (see test_layer_against_float64 for the composed tolerance).
7. The refused inputs.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402
import _grad_ref as gr  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = ar.DEV
U = ar.U
SENTINEL = ar.SENTINEL
SLOPES = ar.SLOPES
MODES = ar.MODES

SHAPES = {
    "toy": ar.toy,
    "ragged": lambda: synth.random_incidence(3000, 2000, 6.0, seed=4, empty_frac=0.1),
    "cora": synth.cora_shape,
    "boundaries": ar.boundaries,
    "boundaries_T": lambda: ar.transpose(ar.boundaries()),
    "powerlaw": lambda: synth.powerlaw(50_000, 200_000),
}

_CASES = {}


@pytest.fixture
def case(hg):
    def get(name):
        if name not in _CASES:
            _CASES.clear()  # one shape at a time on the device
            torch.cuda.empty_cache()
            _CASES[name] = ar.Case(hg, SHAPES[name](), name)
        return _CASES[name]
    return get


_bits = ar.bits


def _sizes(c, group):
    return c.sizes(group)


CELLS = [(s, g) for s in SHAPES for g in ar.GROUPS]


def test_shapes_reach_every_path(case):
    c = case("powerlaw")
    assert (np.diff(c.inc.csrptr) > 512).sum() > 0 and (np.bincount(c.inc.colind, minlength=c.inc.N) > 512).sum() > 0
    for side in ar.GROUPS:
        assert len(c.plan.segment_info(side)["long_rows"]) > 0, side
    for name in ("boundaries", "boundaries_T"):
        c = case(name)
        info = c.plan.segment_info("hyperedge" if name == "boundaries" else "vertex")
        lens = np.diff(c.inc.csrptr) if name == "boundaries" else np.bincount(c.inc.colind, minlength=c.inc.N)
        have = set(int(x) for x in lens)
        for t in (info["width"] * info["keep"], info["long"], 256 * info["keep"]):
            assert {t - 1, t, t + 1} <= have, (name, t)
        assert {0, 1, 5000} <= have


@pytest.mark.parametrize("shape,group", CELLS)
def test_determinism_and_exact_facts(case, shape, group):
    c = case(shape)
    nnz, guard = c.inc.nnz, 64
    idx, sizes = _sizes(c, group)
    for mode in MODES:
        sv, se = c.scores(mode)
        for slope in SLOPES:
            buf = torch.full((nnz + 2 * guard,), SENTINEL, device=DEV)
            out = buf[guard:guard + nnz]
            c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope, out=out)
            again = c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope)
            torch.cuda.synchronize()
            what = "%s %s %s slope %g" % (shape, group, mode, slope)
            assert torch.equal(_bits(out), _bits(again)), "two calls differ: " + what
            assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + nnz:] == SENTINEL).all()), what
            assert not bool((out == SENTINEL).any()), "a real position was not written: " + what
            ones = out.cpu()[sizes[idx] == 1]
            assert bool((ones == 1.0).all()), "one-entry groups are not exactly 1.0f: " + what


def test_graph_replay_equals_eager(case):
    c = case("cora")
    for group in ar.GROUPS:
        alpha = torch.empty(c.inc.nnz, device=DEV)
        dse_sum = torch.empty(c.inc.M if group == "hyperedge" else c.inc.N, device=DEV)
        outs = {}

        def run():
            c.plan.incidence_attention(c.ptr, c.ind, c.sv, c.se, group, 0.2, out=alpha)
            outs["bwd"] = c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, c.dalpha, c.sv, c.se, group, 0.2)
            c.plan.incidence_sum(c.ptr, c.ind, alpha, group, out=dse_sum)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            run()  # warm-up: builds and uploads the permutation and the long-row lists
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        eager = [alpha.clone(), dse_sum.clone()] + [t.clone() for t in outs["bwd"]]
        alpha.zero_()
        dse_sum.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip([alpha, dse_sum] + list(outs["bwd"]), eager):
            assert torch.equal(_bits(got), _bits(want)), group


@pytest.mark.parametrize("shape,group", CELLS)
def test_alpha_against_float64(case, shape, group):
    c = case(shape)
    for mode in MODES:
        sv, se = c.scores(mode)
        for slope in SLOPES:
            ref, smax = c.ref(mode, group, slope)
            cc = c.c(mode, group, slope)
            assert smax <= 8.0
            got = gr.f64(c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope))
            rel = ((got - ref).abs() / ref).max() if ref.numel() else 0.0
            print("%s %s %s slope %g: max |err| / alpha %.3g (bound %.3g, L %d, Smax %.2f)" % (
                shape, group, mode, slope, float(rel), cc, c.L[group], smax))
            assert bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= cc * ref).all()), (shape, group, mode, slope)


@pytest.mark.parametrize("shape,group", CELLS)
def test_range(case, shape, group):
    c = case(shape)
    idx, sizes = _sizes(c, group)
    L = c.L[group]
    for slope in SLOPES:
        sv, se = c.sv * 2500.0, c.se * 2500.0  # max |sv| = max |se| = 1e4
        got = gr.f64(c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope))
        assert bool(torch.isfinite(got).all())
        sums = ar.segment_sum(c.graph, got, group)
        dev = (sums[sizes > 0] - 1.0).abs()
        print("%s %s slope %g: max |sum - 1| %.3g (bound %.3g)" % (shape, group, slope, float(dev.max()), (2 * L + 16) * U))
        assert bool((dev <= (2 * L + 16) * U).all())
        assert bool((sums[sizes == 0] == 0).all())
        s = torch.nn.functional.leaky_relu(ar.raw_score(c.graph, gr.f64(sv), gr.f64(se)), slope)
        m = torch.full((sizes.numel(),), -float("inf"), dtype=torch.float64).scatter_reduce(0, idx, s, "amax")
        at_max = s == m[idx]
        assert bool((got[at_max] >= 1.0 / L).all())
        own = (torch.ones((), dtype=torch.float32) / sizes[idx][at_max].to(torch.float32)).double()  # fl32(1 / len)
        assert bool((got[at_max] >= own).all())


@pytest.mark.parametrize("shape,group", CELLS)
def test_gradients_against_float64(hg, case, shape, group):
    c = case(shape)
    D = {"ds": 0, "dsv": c.L["vertex"], "dse": c.L["hyperedge"]}
    da = gr.f64(c.dalpha)
    for mode in MODES:
        sv, se = c.scores(mode)
        for slope in SLOPES:
            ref_alpha, _ = c.ref(mode, group, slope)
            cc = c.c(mode, group, slope)
            want = dict(zip(("ds", "dsv", "dse"), ar.closed_form_backward(c.graph, gr.f64(sv), gr.f64(se), group, slope,
                                                                          ref_alpha, da)))
            mass = dict(zip(("ds", "dsv", "dse"), ar.backward_masses(c.graph, group, slope, ref_alpha, da)))
            alpha = c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope)
            got = dict(zip(("ds", "dsv", "dse"), c.plan.incidence_attention_backward(
                c.ptr, c.ind, alpha, c.dalpha, sv, se, group, slope)))
            again = c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, c.dalpha, sv, se, group, slope)
            leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (sv, se)]
            out = hg.ops.incidence_softmax(c.ptr, c.ind, leaves[0], leaves[1], group=group, negative_slope=slope,
                                           num_nodes=c.inc.N)
            auto = torch.autograd.grad(out, [t for t in leaves if t is not None], c.dalpha)
            auto = dict(zip([n for n, t in zip(("dsv", "dse"), leaves) if t is not None], auto))
            torch.cuda.synchronize()
            what = "%s %s %s slope %g" % (shape, group, mode, slope)
            for (name, g), a in zip(got.items(), again):
                assert torch.equal(_bits(g), _bits(a)), "two backward calls differ in %s: %s" % (name, what)
            for name in ("ds", "dsv", "dse"):
                bound = 2 * cc + (c.L[group] + D[name] + 8) * U
                err = ((gr.f64(got[name]) - want[name]).abs() / mass[name].clamp(min=gr.TINY)).max() if want[name].numel() else 0.0
                print("%s %s: max |err| / mass %.3g (bound %.3g)" % (what, name, float(err), bound))
                gr.assert_within(got[name], want[name], mass[name], bound, what + " " + name)
                if name in auto:
                    gr.assert_within(auto[name], want[name], mass[name], bound, what + " autograd " + name)
            assert set(auto) == {n for n, t in (("dsv", sv), ("dse", se)) if t is not None}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_incidence_sum_against_float64(hg, case, shape):
    c = case(shape)
    for side in ar.GROUPS:
        got = c.plan.incidence_sum(c.ptr, c.ind, c.val, side)
        again = c.plan.incidence_sum(c.ptr, c.ind, c.val, side)
        leaf = c.val.clone().requires_grad_(True)
        out = hg.ops.incidence_sum(c.ptr, c.ind, leaf, side=side, num_nodes=c.inc.N)
        w = torch.randn(out.numel(), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
        (dval,) = torch.autograd.grad(out, leaf, w)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(again)) and torch.equal(_bits(out.detach()), _bits(got)), (shape, side)
        want = ar.segment_sum(c.graph, gr.f64(c.val), side)
        mass = ar.segment_sum(c.graph, gr.f64(c.val).abs(), side)
        bound = (c.L[side] + 2) * U
        err = ((gr.f64(got) - want).abs() / mass.clamp(min=gr.TINY)).max()
        print("%s incidence_sum %s: max |err| / sum|val| %.3g (bound %.3g)" % (shape, side, float(err), bound))
        gr.assert_within(got, want, mass, bound, "%s incidence_sum %s" % (shape, side))
        idx, _ = ar.index_of(c.graph, side)
        assert torch.equal(dval.cpu(), w.cpu()[idx]), "incidence_sum backward is not the gather"


@pytest.mark.parametrize("group", ar.GROUPS)
@pytest.mark.parametrize("shape", ["cora", "ragged"])
def test_layer_against_float64(hg, case, shape, group):
    """X, every parameter and dY are non-negative, so outside the softmax backward nothing cancels: Y's mass is |Y|, and a
    parameter gradient's mass is what autograd accumulates when the softmax backward returns its masses (check 4's
    mass_dsv / mass_dse) instead of its signed sums (_attention_ref._MassSoftmax).  |got - ref| <= cc max(mass, TINY) with
    cc the first-order sum of
      * test_attention_layer_gradients' terms for the aggregation, its backward and torch's fp32 ops around it:
        3 FP32_C + (F_out + 1 + nnz + F_in + 16) U;
      * the scores: sv and se are fp32 dot products over F_out terms of rows that are dot products over F_in terms, se a
        mean over at most Lh members; their absolute error, at most Smax (F_in + F_out + Lh + 4) U, sits in an exponent of
        the numerator and of the denominator: 2 Smax (F_in + F_out + Lh + 4) U;
      * alpha itself, check 2's c = (L + 16 + 16 Smax) U, once in each hop: 2 c;
      * the softmax backward and its two reductions, check 4: 2 c + (L + Lv + Lh + 8) U."""
    c = case(shape)
    F_in, F_out, slope = 16, 8, 0.2
    g = torch.Generator().manual_seed(9)
    X32 = torch.rand(c.inc.N, F_in, generator=g)
    dY = torch.rand(c.inc.N, F_out, generator=g)
    params = {"lin.weight": torch.rand(F_out, F_in, generator=g) / F_in, "a_v": torch.rand(F_out, generator=g),
              "a_e": torch.rand(F_out, generator=g), "bias": torch.rand(F_out, generator=g)}
    layer = hg.HypergraphAttnConv(c.h, F_in, F_out, group=group, negative_slope=slope).to(DEV)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            p.copy_(params[name])
    Y = layer(X32.to(DEV))
    Y.backward(dY.to(DEV))
    graph64 = gr.Graph(c.inc, c.h.degE.reshape(-1), c.h.degV.reshape(-1), None)

    def run64(mass):
        leaves = {k: v.double().requires_grad_(True) for k, v in params.items()}
        out = ar.attn_conv(graph64, X32.double(), leaves["lin.weight"], leaves["a_v"], leaves["a_e"], leaves["bias"], group,
                           slope, mass=mass)
        grads = torch.autograd.grad(out, list(leaves.values()), dY.double())
        return out.detach(), dict(zip(leaves, grads))
    Y64, ref = run64(False)
    _, mass = run64(True)
    z = X32.double() @ params["lin.weight"].double().t()
    smax = float((z @ params["a_v"].double()).max() + (z @ params["a_e"].double()).max())
    Lh, Lv = c.L["hyperedge"], c.L["vertex"]
    c_alpha = (c.L[group] + 16 + 16 * smax) * U
    cc = (3 * gr.FP32_C + (F_out + 1 + c.inc.nnz + F_in + 16) * U + 2 * smax * (F_in + F_out + Lh + 4) * U + 2 * c_alpha
          + 2 * c_alpha + (c.L[group] + Lv + Lh + 8) * U)
    gr.assert_within(Y, Y64, Y64.abs(), cc, "%s %s layer out" % (shape, group))
    for name, p in layer.named_parameters():
        err = float(((gr.f64(p.grad) - ref[name]).abs() / mass[name].clamp(min=gr.TINY)).max())
        print("%s %s layer d%s: max |err| / mass %.3g (bound %.3g)" % (shape, group, name, err, cc))
        assert bool((mass[name] >= ref[name].abs() * (1 - 1e-12)).all())
        gr.assert_within(p.grad, ref[name], mass[name], cc, "%s %s layer d%s" % (shape, group, name))


def test_refused_inputs(hg, case):
    c = case("cora")
    ops = hg.ops
    N, M, nnz = c.inc.N, c.inc.M, c.inc.nnz
    for variant in ("fused", "push_atomic", "push_groups"):
        with pytest.raises(ValueError):
            ops.incidence_softmax(c.ptr, c.ind, c.sv, c.se, options=ops.Options(variant=variant))
    for variant in ("auto", "pull"):
        ops.incidence_softmax(c.ptr, c.ind, c.sv, c.se, options=ops.Options(variant=variant))
    with pytest.raises(TypeError):
        ops.incidence_softmax(c.ptr, c.ind, c.sv.to(torch.bfloat16), c.se)
    with pytest.raises(TypeError):
        ops.incidence_sum(c.ptr, c.ind, c.val.to(torch.bfloat16), num_nodes=N)
    with pytest.raises(ValueError):
        ops.incidence_softmax(c.ptr, c.ind, c.sv, c.se[:-1])
    with pytest.raises(ValueError):
        ops.incidence_softmax(c.ptr, c.ind, torch.zeros(N + 1, device=DEV), c.se, num_nodes=N)
    with pytest.raises(ValueError):
        ops.incidence_softmax(c.ptr, c.ind, c.sv[:-1], c.se, num_nodes=N)
    with pytest.raises(ValueError):
        ops.incidence_sum(c.ptr, c.ind, c.val[:-1], num_nodes=N)
    with pytest.raises(ValueError):
        c.plan.incidence_attention_backward(c.ptr, c.ind, c.val[:-1], c.dalpha, c.sv, c.se)
    with pytest.raises(RuntimeError):
        ops.incidence_softmax(c.ptr, c.ind, c.sv.cpu(), c.se)
    with pytest.raises(RuntimeError):
        ops.incidence_softmax(c.ptr, c.ind, c.sv, c.se.cpu())
    with pytest.raises(RuntimeError):
        ops.incidence_sum(c.ptr, c.ind, c.val.cpu(), num_nodes=N)
    with pytest.raises(RuntimeError):
        ops.incidence_softmax(c.ptr.cpu(), c.ind, c.sv, c.se)
    # neither score: the uniform coefficients 1 / |group|
    uni = ops.incidence_softmax(c.ptr, c.ind, None, None, num_nodes=N)
    sizes = torch.from_numpy(np.repeat(np.diff(c.inc.csrptr), np.diff(c.inc.csrptr)).astype(np.float32))
    assert torch.equal(uni.cpu(), 1.0 / sizes) and uni.numel() == nnz and M == c.se.numel()
