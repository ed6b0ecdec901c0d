"""The fused attention aggregation on the GPU: hg_incidence_attention_stats_heads_f32, hg_aggr_incidence_attention_heads_f32,
hg_gather_rows_attention_heads_f32, ops.incidence_attention_aggr and HypergraphAttnConv(fuse_attention=True).

Graphs: `dup` (a vertex listed twice, an empty hyperedge, an isolated vertex); `ragged` (700 x 450, 10 % empty hyperedges);
`dense` (300 x 40, 150 members on average, 13 hyperedges above 128 entries -- wave tasks in hop 1, workgroup segments on
the hyperedge side); `cora` with the latency schedule pinned for one or both hops; `ragged` on a plan with 16-row, 32-entry
panels and split_len = 8, so that rows are cut and fixups run.
(F, H): (4, 1), (32, 1), (33, 1), (128, 1), (260, 1), (32, 8), (6, 2), (64, 2): 4-byte lanes (33, and C = 3 with F % 4 != 0),
16-byte lanes, two column tiles (260), C = 4 (a 16-byte lane per head).

Bit checks compare int32 patterns.  Float64 bounds, U = 2^-24, mass = the expression on absolute values:
  alpha from the statistics: the project's bound of alpha itself, c_alpha = (L + 16 + 16 Smax) U relative (test_attention_gpu),
    plus 4 U for the exponential, the product and the two roundings of the torch expression that rebuilds it;
  Y, dX, ddegE, ddegV, dW: multilinear in (X, alpha, alpha, scales, dY): FP32_C of the mass for the sums (the bound of
    test_incidence_aggr) plus 2 c_alpha for the two coefficient factors, plus (C + 1) U where a C-term dot ends the chain;
  dsv, dse: the softmax backward's own bound 2 c_alpha + (L + D + 8) U (test_attention_gpu; D the other side's longest
    group) on a dalpha that is itself a C-term dot of two tables each within FP32_C + 2 c_alpha: in all
    FP32_C + 4 c_alpha + (L + D + C + 9) U of the mass (backward_masses on dalpha's mass)."""
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
import _scale_grad_ref as sg  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV, U, SENTINEL = ar.DEV, ar.U, ar.SENTINEL
GUARD = 64
_bits = ar.bits
SLOPE = 0.2
PAIRS = [(4, 1), (32, 1), (33, 1), (128, 1), (260, 1), (32, 8), (6, 2), (64, 2)]
GROUPS = ar.GROUPS


def _dup():
    ptr = np.array([0, 3, 7, 7, 9], np.int32)
    ind = np.array([0, 2, 3, 1, 2, 2, 5, 0, 5], np.int32)
    return synth.Incidence(6, 4, ptr, ind, name="dup")


SHAPES = {
    "dup": _dup,
    "ragged": lambda: synth.random_incidence(700, 450, 7.0, seed=3, empty_frac=0.1),
    "dense": lambda: synth.random_incidence(300, 40, 150.0, seed=6),
    "cora": synth.cora_shape,
}
# name -> (shape, make_opts keywords, pinned pull_hop_kernels or None)
PLANS = {
    "dup": ("dup", {}, None),
    "ragged": ("ragged", {}, None),
    "dense": ("dense", {}, None),
    "cora_lat_hop0": ("cora", {}, 2 + 3 * 1),
    "cora_lat_hop1": ("cora", {}, 1 + 3 * 2),
    "cora_lat_both": ("cora", {}, 2 + 3 * 2),
    "ragged_small": ("ragged", ir.option_sets()["small"], None),
}


class _G:
    """One incidence on the device with a plan of its own, scales (degE = 1 / |e|: inf on an empty hyperedge), scores."""

    def __init__(self, name):
        from hypergef_amd.plan import Plan, make_opts
        shape, opts, self.pin = PLANS[name]
        self.name, self.inc = name, SHAPES[shape]()
        inc = self.inc
        self.ptr, self.ind = torch.from_numpy(inc.csrptr).to(DEV), torch.from_numpy(inc.colind).to(DEV)
        self.plan = Plan.from_tensors(inc.N, self.ptr, self.ind, opts=make_opts(**opts) if opts else None)
        if self.pin is not None:
            assert self.plan.has_latency_schedule(), name
        rng = np.random.default_rng(5)
        self.degE = torch.from_numpy(np.diff(inc.csrptr).astype(np.float32)).pow(-1).to(DEV)
        self.degV = torch.from_numpy(rng.random(inc.N).astype(np.float32) + 0.5).to(DEV)
        self.W = torch.from_numpy(rng.random(inc.M).astype(np.float32) + 0.5).to(DEV)
        self.index = sg.Index(inc)
        self.L = {g: ar.longest(inc, g) for g in GROUPS}

    def scores(self, H, seed=31):
        g = torch.Generator().manual_seed(seed + H)
        sv, se = torch.randn(self.inc.N, H, generator=g), torch.randn(self.inc.M, H, generator=g)
        sv, se = sv * (4.0 / float(sv.abs().max())), se * (4.0 / float(se.abs().max()))
        if H == 1:
            sv, se = sv.reshape(-1), se.reshape(-1)
        return sv.to(DEV), se.to(DEV)

    def feats(self, F, seed=1, rows=None):
        g = torch.Generator().manual_seed(seed * 1000 + F)
        return torch.randn(self.inc.N if rows is None else rows, F, generator=g).to(DEV)

    def use(self, F):
        if self.pin is not None:
            self.plan.pin(F, "pull", self.pin)

    def c_alpha(self, group, smax=8.0):
        return (self.L[group] + 16 + 16 * smax) * U


_GRAPHS = {}


@pytest.fixture
def graph(hg):
    def get(name):
        if name not in _GRAPHS:
            _GRAPHS[name] = _G(name)
        return _GRAPHS[name]
    return get


def _guarded(*shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _eq(a, b):
    return torch.equal(_bits(a), _bits(b))


def _modes(sv, se):
    return (("both", sv, se), ("sv", sv, None), ("se", None, se))


# ---- 1. the statistics ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dup", "ragged", "dense"])
@pytest.mark.parametrize("H", [1, 8])
def test_statistics_rebuild_alpha(graph, name, H):
    g = graph(name)
    inc = g.inc
    sv, se = g.scores(H)
    E = torch.from_numpy(np.repeat(np.arange(inc.M), np.diff(inc.csrptr))).to(DEV)
    V = g.ind.long()
    for group in GROUPS:
        idx, nseg = (E, inc.M) if group == "hyperedge" else (V, inc.N)
        empty = torch.bincount(idx, minlength=nseg) == 0
        for mode, a, b in _modes(sv, se):
            what = "%s H %d %s %s" % (name, H, group, mode)
            mx, inv = g.plan.incidence_attention_stats(g.ptr, g.ind, a, b, group, SLOPE, heads=H)
            mx2, inv2 = g.plan.incidence_attention_stats(g.ptr, g.ind, a, b, group, SLOPE, heads=H)
            assert _eq(mx, mx2) and _eq(inv, inv2), "two calls differ: " + what
            assert mx.shape == ((nseg,) if H == 1 else (nseg, H))
            assert bool((mx[empty] == 0).all()) and bool((inv[empty] == 0).all()), "empty segments: " + what
            assert bool(torch.isfinite(mx).all()) and bool((inv[~empty] > 0).all()) and bool((inv <= 1).all()), what
            alpha = g.plan.incidence_attention(g.ptr, g.ind, a, b, group, SLOPE, heads=H)
            raw = torch.zeros_like(alpha, dtype=torch.float64)
            if a is not None:
                raw = raw + a.double()[V]
            if b is not None:
                raw = raw + b.double()[E]
            raw = raw.float().double()  # the kernel's raw: one fp32 addition of two fp32 scores
            rebuilt = torch.exp(torch.nn.functional.leaky_relu(raw, SLOPE) - mx.double()[idx]) * inv.double()[idx]
            ref = hr.softmax(g.index, gr.f64(a).reshape(inc.N, H) if a is not None else None,
                             gr.f64(b).reshape(inc.M, H) if b is not None else None, group, SLOPE, H).reshape(alpha.shape)
            print("%s: max |rebuilt - alpha| / alpha = %.3g" % (what, float(((rebuilt - alpha.double()).abs() / alpha.double()).max())))
            c = g.c_alpha(group) + 4 * U
            for got, label in ((rebuilt, "rebuilt from the statistics"), (alpha, "alpha")):
                gr.assert_within(got, ref, ref, c, "%s, %s" % (label, what))
            # slope * raw is a rounded fp32 product in the kernel: against the kernel's own alpha the rebuilt value is
            # within the exponential's and the roundings' few units
            gr.assert_within(rebuilt, alpha, alpha, 8 * U + 16 * 8.0 * U, "rebuilt against the kernel's alpha, " + what)


# ---- 2. bit equality with the composition, 5. guard bands ---------------------------------------------------------------

def _composed(g, X, a, b, group, H, scales):
    degE, degV, W = scales
    alpha = g.plan.incidence_attention(g.ptr, g.ind, a, b, group, SLOPE, heads=H)
    xe = torch.empty(g.inc.M, X.shape[1], device=DEV)
    return g.plan.aggregate_incidence(g.ptr, g.ind, X, alpha, alpha, degE, degV, W, xe_out=xe, heads=H), xe


@pytest.mark.parametrize("name", list(PLANS))
@pytest.mark.parametrize("F,H", PAIRS)
def test_bits_of_the_composition_inside_guard_bands(graph, name, F, H):
    g = graph(name)
    g.use(F)
    inc = g.inc
    X = g.feats(F)
    sv, se = g.scores(H)
    nbytes = g.plan.incidence_workspace_bytes(F)
    for group in GROUPS:
        nseg = inc.M if group == "hyperedge" else inc.N
        for mode, a, b in _modes(sv, se):
            for scales in ((g.degE, g.degV, g.W), (None, None, None)):
                if mode != "both" and scales[0] is None:
                    continue
                what = "%s F %d H %d %s %s scales %s" % (name, F, H, group, mode, scales[0] is not None)
                want, want_xe = _composed(g, X, a, b, group, H, scales)
                bm, mx = _guarded(nseg, H)
                bi, inv = _guarded(nseg, H)
                g.plan.incidence_attention_stats(g.ptr, g.ind, a, b, group, SLOPE, heads=H, out=(mx, inv))
                by, Y = _guarded(inc.N, F)
                bx, xe = _guarded(inc.M, F)
                bw = torch.full((nbytes // 4 + 2 * GUARD,), SENTINEL, device=DEV)
                ws = bw[GUARD:GUARD + nbytes // 4].view(torch.uint8)
                g.plan.aggregate_incidence_attention(g.ptr, g.ind, X, a, b, group, SLOPE, mx, inv, *scales, xe_out=xe,
                                                     out=Y, workspace=ws, heads=H)
                assert _eq(Y, want), "Y: " + what
                assert _eq(xe, want_xe), "Xe_out: " + what
                for buf in (bm, bi, by, bx, bw):
                    assert _guards_intact(buf), "guard words: " + what
                assert not bool((mx == SENTINEL).any()) and not bool((inv == SENTINEL).any()), what
                assert not bool((Y == SENTINEL).any()) and not bool((xe == SENTINEL).any()), what
                # hop 0 into hop 1 as calls of their own
                t = g.plan.gather_rows_attention(0, g.ptr, g.ind, X, mx, inv, a, b, group, SLOPE, scales[0], scales[2], heads=H)
                y2 = g.plan.gather_rows_attention(1, g.ptr, g.ind, t, mx, inv, a, b, group, SLOPE, scales[1], None, heads=H)
                assert _eq(t, want_xe) and _eq(y2, want), "one hop at a time: " + what
    if name == "dup":  # the empty hyperedge's row is exactly 0 under degE = inf; the isolated vertex's too
        assert bool((want_xe[2] == 0).all()) and bool((want[4] == 0).all())


def test_the_graphs_reach_the_paths_they_are_here_for(graph):
    g = graph("dense")
    assert int(np.diff(g.inc.csrptr).max()) > 128
    assert len(g.plan.segment_info("hyperedge")["long_rows"]) > 0, "dense: no workgroup segment"
    assert len(g.plan.schedule(0)["tasks"]) > 0, "dense: hop 1 runs no wave tasks"
    s = graph("ragged_small")
    for hop in (0, 1):
        assert len(s.plan.schedule(hop)["tasks"]) > 0 and len(s.plan.schedule(hop)["fixups"]) > 0, "small panels: no split rows"


# ---- 3. float64, 4. gradients equal the composed graph's --------------------------------------------------------------------

def _run(fn, g, X, sv, se, group, H, with_scales, dY):
    from hypergef_amd import ops  # noqa: F401
    leaves = [t.clone().requires_grad_(True) for t in (X, sv, se)]
    scales = [t.clone().requires_grad_(True) for t in (g.degE, g.degV, g.W)] if with_scales else [None, None, None]
    Y = fn(g, leaves[0], leaves[1], leaves[2], group, H, scales)
    Y.backward(dY)
    return Y.detach(), [t.grad for t in leaves] + [None if t is None else t.grad for t in scales]


def _fused_op(g, X, sv, se, group, H, scales):
    from hypergef_amd import ops
    return ops.incidence_attention_aggr(g.ptr, g.ind, X, sv, se, group=group, negative_slope=SLOPE, degE=scales[0],
                                        degV=scales[1], W=scales[2], heads=H)


def _composed_op(g, X, sv, se, group, H, scales):
    from hypergef_amd import ops
    alpha = ops.incidence_softmax(g.ptr, g.ind, sv, se, group=group, negative_slope=SLOPE, heads=H, num_nodes=g.inc.N)
    return ops.incidence_aggr(g.ptr, g.ind, X, alpha, alpha, scales[0], scales[1], scales[2], heads=H)


NAMES = ("X", "node_score", "edge_score", "degE", "degV", "W")


@pytest.mark.parametrize("name", ["dup", "ragged", "dense", "cora_lat_both", "ragged_small"])
@pytest.mark.parametrize("F,H", [(33, 1), (32, 8), (6, 2), (128, 1)])
@pytest.mark.parametrize("group", GROUPS)
def test_gradients_equal_the_composed_graphs(hg, graph, name, F, H, group):
    from hypergef_amd import plan as planmod
    g = graph(name)
    inc = g.inc
    opts = PLANS[name][1]
    # the operators run on the cached plan of these tensors: built here with this case's options and pin
    planmod.set_default_opts(planmod.make_opts(**opts) if opts else None)
    try:
        cached = planmod.cached_plan(inc.N, g.ptr, g.ind)
        if g.pin is not None:
            cached.pin(F, "pull", g.pin)
        X, dY = g.feats(F), g.feats(F, seed=2)
        sv, se = g.scores(H)
        for with_scales in (True, False):
            Yf, gf = _run(_fused_op, g, X, sv, se, group, H, with_scales, dY)
            Yc, gc = _run(_composed_op, g, X, sv, se, group, H, with_scales, dY)
            assert _eq(Yf, Yc), "Y"
            for n, a, b in zip(NAMES, gf, gc):
                assert (a is None) == (b is None), n
                if a is not None:
                    assert a.shape == b.shape and _eq(a, b), "d%s differs from the composed graph's (%s F %d H %d %s)" % (
                        n, name, F, H, group)
    finally:
        planmod.set_default_opts(None)


@pytest.mark.parametrize("name", ["dup", "ragged", "dense"])
@pytest.mark.parametrize("F,H", [(33, 1), (32, 8), (6, 2)])
@pytest.mark.parametrize("group", GROUPS)
def test_against_float64(hg, graph, name, F, H, group):
    g = graph(name)
    inc, ix = g.inc, g.index
    C = F // H
    X, dY = g.feats(F), g.feats(F, seed=2)
    sv, se = g.scores(H)
    Y, grads = _run(_fused_op, g, X, sv, se, group, H, True, dY)

    def ref(mass):
        x, a, b, dE, dV, w = (gr.f64(t) for t in (X, sv.reshape(inc.N, H), se.reshape(inc.M, H), g.degE, g.degV, g.W))
        go = gr.f64(dY)
        if mass:
            x, dE, dV, w, go = x.abs(), dE.abs(), dV.abs(), w.abs(), go.abs()
        ins = [t.requires_grad_(True) for t in (x, a, b, dE, dV, w)]
        alpha = hr._MassSoftmax.apply(a, b, ix, group, SLOPE) if mass else hr.softmax(ix, a, b, group, SLOPE, H)
        y = sg.fn(ix, ins[0], ins[3], ins[4], ins[5], alpha, alpha, H)
        return y.detach(), torch.autograd.grad(y, ins, go)

    y64, g64 = ref(False)
    ym, gm = ref(True)
    other = "vertex" if group == "hyperedge" else "hyperedge"
    ca = g.c_alpha(group)
    c_lin = gr.FP32_C + 2 * ca + (C + 1) * U
    c_score = gr.FP32_C + 4 * ca + (g.L[group] + g.L[other] + C + 9) * U
    what = "%s F %d H %d %s" % (name, F, H, group)
    gr.assert_within(Y, y64, ym, c_lin, "Y, " + what)
    for n, got, want, mass in zip(NAMES, grads, g64, gm):
        c = c_score if n in ("node_score", "edge_score") else c_lin
        err = ((gr.f64(got).reshape(want.shape) - want).abs() / mass.clamp(min=gr.TINY)).max()
        print("%s d%s: max error %.3g of the mass (bound %.3g)" % (what, n, float(err), c))
        gr.assert_within(got.reshape(want.shape), want, mass, c, "d%s, %s" % (n, what))


def test_without_grad_no_node_is_made(hg, graph):
    from hypergef_amd import ops
    g = graph("ragged")
    X = g.feats(32)
    sv, se = g.scores(8)
    Y = ops.incidence_attention_aggr(g.ptr, g.ind, X, sv, se, heads=8)
    assert Y.grad_fn is None and not Y.requires_grad
    with torch.no_grad():
        Y2 = ops.incidence_attention_aggr(g.ptr, g.ind, X.clone().requires_grad_(True), sv, se, heads=8)
    assert Y2.grad_fn is None and _eq(Y, Y2)
    want, _ = _composed(g, X, sv, se, "hyperedge", 8, (None, None, None))
    assert _eq(Y, want)


# ---- 6. nothing of size nnz is kept -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dense", "cora"])
@pytest.mark.parametrize("group", GROUPS)
def test_nothing_of_size_nnz_is_kept(hg, graph, name, group):
    from hypergef_amd import plan as planmod
    H, F = 8, 8  # F small enough that the feature rows themselves stay below nnz * H elements on both shapes
    inc = SHAPES[name]()
    assert inc.N * F < inc.nnz * H
    ptr, ind = torch.from_numpy(inc.csrptr).to(DEV), torch.from_numpy(inc.colind).to(DEV)
    g = type("G", (), dict(ptr=ptr, ind=ind, inc=inc))
    gen = torch.Generator().manual_seed(3)
    X, sv, se = (torch.randn(*s, generator=gen).to(DEV) for s in ((inc.N, F), (inc.N, H), (inc.M, H)))
    R = inc.M if group == "hyperedge" else inc.N
    held = {}
    for label, fn in (("fused", _fused_op), ("composed", _composed_op)):  # both warm first: plans, lists, permutation
        leaves = [t.clone().requires_grad_(True) for t in (X, sv, se)]
        fn(g, *leaves, group, H, [None, None, None]).sum().backward()
        del leaves
        torch.cuda.synchronize()
        leaves = [t.clone().requires_grad_(True) for t in (X, sv, se)]
        base = torch.cuda.memory_allocated()
        Y = fn(g, *leaves, group, H, [None, None, None])
        torch.cuda.synchronize()
        held[label] = torch.cuda.memory_allocated() - base
        if label == "fused":
            saved = [t for t in Y.grad_fn.saved_tensors if t is not None]
            assert len(saved) >= 5
            for t in saved:
                assert t.numel() < inc.nnz * H, "a saved tensor of %d elements (nnz * H = %d)" % (t.numel(), inc.nnz * H)
        Y.sum().backward()
        assert all(t.grad is not None for t in leaves)
        del Y, leaves
    print("%s %s: held between forward and backward: fused %d B, composed %d B" % (name, group, held["fused"], held["composed"]))
    assert held["composed"] - held["fused"] >= inc.nnz * H * 4 - 2 * R * H * 4, held
    planmod.clear_plan_cache()


# ---- 7. no permutation: capturable after one warm call of itself -----------------------------------------------------------

@pytest.mark.parametrize("group", GROUPS)
def test_captured_on_a_fresh_plan(hg, group):
    from hypergef_amd import ops, plan as planmod
    planmod.clear_plan_cache()
    inc = synth.random_incidence(900, 500, 6.0, seed=12, empty_frac=0.05)  # tensors no other test has made a plan for
    ptr, ind = torch.from_numpy(inc.csrptr).to(DEV), torch.from_numpy(inc.colind).to(DEV)
    H, F = 4, 32
    gen = torch.Generator().manual_seed(9)
    X, sv, se = (torch.randn(*s, generator=gen).to(DEV) for s in ((inc.N, F), (inc.N, H), (inc.M, H)))
    degE = torch.from_numpy(np.diff(inc.csrptr).astype(np.float32)).pow(-1).to(DEV)

    def call():
        return ops.incidence_attention_aggr(ptr, ind, X, sv, se, group=group, degE=degE, heads=H)

    eager = call()  # the one warm call: builds the plan, uploads the long-row list; no incidence_aggr has run
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            out = call()
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(3):
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert _eq(out, eager)
    # and it is the composition's answer (this call uploads the permutation the fused one never asked for)
    alpha = ops.incidence_softmax(ptr, ind, sv, se, group=group, heads=H, num_nodes=inc.N)
    assert _eq(eager, ops.incidence_aggr(ptr, ind, X, alpha, alpha, degE, heads=H))
    planmod.clear_plan_cache()


# ---- 8. the layer -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("group", GROUPS)
def test_layer_with_and_without_the_switch(hg, heads, group):
    import hypergef_amd as hgm
    inc = synth.random_incidence(700, 450, 7.0, seed=3, empty_frac=0.1)
    hyperg = hgm.HyperGraph.from_incidence(inc, DEV, data_name="ragged-layer", ngs=1 << 30)
    torch.manual_seed(4)
    kw = dict(group=group, heads=heads, learn_hyperedge_weight=True)
    plain = hgm.HypergraphAttnConv(hyperg, 12, 8, **kw).to(DEV)
    fused = hgm.HypergraphAttnConv(hyperg, 12, 8, fuse_attention=True, **kw).to(DEV)
    fused.load_state_dict(plain.state_dict())
    X = torch.randn(inc.N, 12, device=DEV)
    dY = torch.randn(inc.N, heads * 8, device=DEV)
    outs = []
    for layer in (plain, fused):
        x = X.clone().requires_grad_(True)
        y = layer(x)
        y.backward(dY)
        outs.append((y.detach(), x.grad, {n: p.grad for n, p in layer.named_parameters()}))
    assert "IncidenceAttentionAggr" in type(fused(X).grad_fn.next_functions[0][0]).__name__
    assert _eq(outs[0][0], outs[1][0]) and _eq(outs[0][1], outs[1][1])
    assert list(outs[0][2]) == list(outs[1][2])
    for n in outs[0][2]:
        assert outs[1][2][n] is not None and _eq(outs[0][2][n], outs[1][2][n]), "gradient of %s" % n
    # dropout in training mode: the switch steps aside, the same seed gives the same mask
    a = hgm.HypergraphAttnConv(hyperg, 12, 8, dropout=0.5, **kw).to(DEV)
    b = hgm.HypergraphAttnConv(hyperg, 12, 8, dropout=0.5, fuse_attention=True, **kw).to(DEV)
    b.load_state_dict(a.state_dict())
    ys = []
    for layer in (a, b):
        torch.manual_seed(77)
        ys.append(layer(X).detach())
    assert _eq(ys[0], ys[1])
    assert not _eq(ys[0], a.eval()(X).detach())  # the mask did something
    assert _eq(a.eval()(X).detach(), b.eval()(X).detach())  # eval(): no dropout active, the fused path again
