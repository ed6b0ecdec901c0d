"""The pull variant's three kernels per hop, each named with Plan.pin (hg_plan_set_choice) instead of left to the tuner's
stopwatch: k = 0 the streaming row gather, 1 row panels + wave tasks on the plan's schedule, 2 the same kernel on the latency
schedule; a mask is k0 + 3 * k1.  test_hop_kernels_host.py vets the pin entry itself and the integer inputs of check 2.

Graphs toy, ragged, boundaries, boundaries_T, ragged+dups and powerlaw of _incidence_ref.GRAPHS (all below 2^18 incidences)
under the option sets default and wide (latency schedule: nine masks) and dfs, small and odd (short_max <= 6, none: the four
masks of kinds 0 and 1; odd also turns the XCD remap off, which the streaming kernel reads).  Widths 1 and 3 -- not 16-byte
lanes, so kind 0 falls through to the general kernel there and must equal kind 1 bit for bit -- and 4, 8, 12, 20, 33, 64, 128,
260.  Weighted (degE, degV, W) and unweighted, fp32 and bf16.  Per cell and reachable mask:

1. The pin took effect.  a: a default plan pinned to mask 1 + 3 * 1 gives the bits of a plan built with row_stream=False and
   never pinned, for the forced pull and for Plan.gather_rows on each hop.  b: mask 0, and the plan after unpin, give the bits
   of a plan that was never pinned.  c: at F = 64 on the side of boundaries / boundaries_T that has the rows of 255 .. 257,
   1023 .. 1025 and 5000 entries, kinds 0 and 1, and kinds 1 and 2, differ in at least one bit: three kernels ran.
2. X in {-1, 0, 1}, scales powers of two: fp32 Xe and Y equal the float64 answer exactly under every mask.
3. randn inputs: |got - ref| <= FP32_C * max(mass, TINY) per element (_grad_ref).
4. aggregate(variant="pull") under (k0, k1) is gather_rows(1, gather_rows(0, X)) under the same mask bit for bit; hop 0's Xe
   has the same bits for every k1; for a fixed Xe, hop 1's Y has the same bits for every k0.
5. bf16, F % 4 == 0: aggregate(Xb) == aggregate(Xb.float()).to(bf16) bit for bit for variant "pull" and for "auto" pinned to
   pull, under every mask, and once more on a row_stream=False plan without a pin.
6. Under mask 2 + 3 * 2 (1 + 3 * 1 without a latency schedule) Plan.aggregate_incidence with NULL and with unit weights is the
   unweighted pull under the same pin bit for bit, and multi-head columns equal the single-head calls.
7. A fresh plan pinned to what Plan.tune returned reproduces the Y the tuner left; after unpin it gives a never-tuned plan's.
8. Two calls under one pin agree; outputs and workspace sit between NaN guard bands that stay intact, and every element of
   the output is written.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _grad_ref as gr  # noqa: E402
import _incidence_ref as ir  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FMAX = max(ir.HOP_WIDTHS)
GUARD = 128  # elements on either side: 512 bytes of fp32, 256 of bf16, so the guarded view keeps its alignment
NAN = float("nan")
CELLS = [(g, s) for g in ir.GRAPHS for s in ir.HOP_OPTION_SETS]
BF16_WIDTHS = tuple(F for F in ir.HOP_WIDTHS if F % 4 == 0)
NOT_LANES16 = tuple(F for F in ir.HOP_WIDTHS if not (F % 4 == 0 or F > 8))  # run_hop's lanes16: 1 and 3
NONE = (None, None, None)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _guarded(dtype, *shape):
    """(buffer, view): a NaN-filled buffer and the output inside it, GUARD elements on either side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), NAN, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


class _Case:
    """One graph on the device: inputs drawn once at the widest width (a narrower call takes the first columns), scales,
    plans per option set and the float64 answers, computed once on the device (ir.graph_on) and never modified."""

    def __init__(self, name):
        self.name = name
        self.inc = inc = ir.schedule_graph(name)
        self.N, self.M, self.nnz = inc.N, inc.M, inc.nnz
        self.ptr, self.ind = torch.from_numpy(inc.csrptr).to(DEV), torch.from_numpy(inc.colind).to(DEV)
        rng = np.random.default_rng(29)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)  # noqa: E731
        self._X = {"randn": dev(rng.standard_normal((inc.N, FMAX))), "int": dev(ir.integer_inputs(inc, FMAX)[0])}
        self._scales = {"randn": tuple(dev(rng.random(n) + 0.5) for n in (inc.M, inc.N, inc.M)),
                        "int": tuple(dev(a) for a in ir.power_of_two_scales(inc))}  # (degE, degV, W)
        self._plans, self._refs = {}, {}

    def X(self, kind, F):
        return self._X[kind][:, :F].contiguous()

    def scales(self, kind, weighted):
        return self._scales[kind] if weighted else NONE

    def plan(self, opts, row_stream=True, tag=""):
        from hypergef_amd.plan import Plan, make_opts
        key = (opts, row_stream, tag)
        if key not in self._plans:
            self._plans[key] = Plan.from_tensors(self.N, self.ptr, self.ind,
                                                 make_opts(row_stream=row_stream, **ir.option_sets()[opts]))
        return self._plans[key]

    def ref(self, kind, weighted):
        """(Xe, mass of Xe, Y, mass of Y) in float64 at width FMAX."""
        if (kind, weighted) not in self._refs:
            g = ir.graph_on(gr.Graph(self.inc, *(t.cpu() if t is not None else None for t in self.scales(kind, weighted))), DEV)
            x = self._X[kind].double()
            self._refs[kind, weighted] = (ir.hop1(g, x), ir.hop1(g.abs(), x.abs()),
                                          ir.incidence_aggr(g, x), ir.incidence_aggr(g.abs(), x.abs()))
        return self._refs[kind, weighted]

    # the three calls under test; sc = (degE, degV, W)
    def pull(self, plan, X, sc, variant="pull", out=None, workspace=None):
        return plan.aggregate(self.ptr, self.ind, X, *sc, variant=variant, out=out, workspace=workspace, bind_scales=False)

    def hop0(self, plan, X, sc):
        return plan.gather_rows(0, self.ptr, self.ind, X, sc[0], sc[2])

    def hop1(self, plan, Xe, sc):
        return plan.gather_rows(1, self.ptr, self.ind, Xe, sc[1], None)


_CASES = {}


@pytest.fixture
def case(hg):
    def get(name):
        if name not in _CASES:
            _CASES.clear()  # one graph at a time: its float64 answers are kept while its option sets run
            torch.cuda.empty_cache()
            _CASES[name] = _Case(name)
        return _CASES[name]
    return get


def _masks(plan, graph, opts):
    """The masks this plan accepts; that `default` and `wide` reach all nine is asserted, not assumed."""
    has_lat = plan.has_latency_schedule()
    assert has_lat == ir.HOP_SETS_WITH_LAT[opts] == ir.expect_latency_schedule(plan.nnz, plan.info["short_max"]), (graph, opts)
    masks = ir.hop_masks(has_lat)
    print("reach %s/%s: short_max %d, masks %s" % (graph, opts, plan.info["short_max"], list(masks)))
    return masks


def _kinds(masks):
    return sorted({m % 3 for m in masks})


@pytest.mark.parametrize("graph,opts", CELLS)
def test_exact_integers_two_calls_and_guards(case, graph, opts):
    """Checks 2 and 8."""
    c = case(graph)
    plan = c.plan(opts)
    masks = _masks(plan, graph, opts)
    top = max(ir.unweighted_mass_bound(c.inc))
    assert top * ir.SCALE_PRODUCT_MAX < 2 ** 24 and top * ir.SCALE_PRODUCT_MAX / ir.SCALE_GRANULE < 2 ** 24, (graph, top)
    for weighted in (False, True):
        sc = c.scales("int", weighted)
        want_xe, _, want_y, _ = c.ref("int", weighted)
        for F in ir.HOP_WIDTHS:
            X = c.X("int", F)
            for m in masks:
                what = "%s/%s F %d weighted %s mask %d" % (graph, opts, F, weighted, m)
                plan.pin(F, "pull", m)
                nws = (plan.workspace_bytes(F) + 3) // 4
                ybuf, Y = _guarded(torch.float32, c.N, F)
                wbuf, ws = _guarded(torch.float32, nws)
                c.pull(plan, X, sc, out=Y, workspace=ws.view(torch.uint8))
                again = c.pull(plan, X, sc)
                Xe = c.hop0(plan, X, sc)
                assert torch.equal(Xe.double(), want_xe[:, :F]), "Xe is not the exact answer: " + what
                assert torch.equal(Y.double(), want_y[:, :F]), "Y is not the exact answer: " + what
                assert torch.equal(c.hop1(plan, Xe, sc).double(), want_y[:, :F]), "hop 1 alone is not exact: " + what
                assert _same(again, Y), "two calls differ: " + what
                assert _guards_intact(ybuf) and _guards_intact(wbuf), "guard bands: " + what
                assert not bool(torch.isnan(Y).any()), "elements of Y left unwritten: " + what
            plan.unpin(F)


@pytest.mark.parametrize("graph,opts", CELLS)
def test_float64_accuracy_and_composition(case, graph, opts):
    """Checks 3 and 4."""
    c = case(graph)
    plan = c.plan(opts)
    masks = _masks(plan, graph, opts)
    kinds = _kinds(masks)
    worst = [0.0, 0.0]
    for weighted in (False, True):
        sc = c.scales("randn", weighted)
        ref_xe, mass_xe, ref_y, mass_y = c.ref("randn", weighted)
        for F in ir.HOP_WIDTHS:
            X = c.X("randn", F)
            xe_of = {}
            for m in masks:
                k0 = m % 3
                what = "%s/%s F %d weighted %s mask %d" % (graph, opts, F, weighted, m)
                plan.pin(F, "pull", m)
                Y, Xe = c.pull(plan, X, sc), c.hop0(plan, X, sc)
                assert _same(Y, c.hop1(plan, Xe, sc)), "pull is not hop 0 into hop 1: " + what
                if k0 not in xe_of:
                    xe_of[k0] = Xe
                    worst[0] = max(worst[0], ir.within_on_device(Xe, ref_xe[:, :F], mass_xe[:, :F], gr.FP32_C, what + " Xe"))
                assert _same(Xe, xe_of[k0]), "hop 0 depends on hop 1's kernel: " + what
                worst[1] = max(worst[1], ir.within_on_device(Y, ref_y[:, :F], mass_y[:, :F], gr.FP32_C, what + " Y"))
            for k1 in kinds:  # one Xe, hop 1 under every k0
                ys = []
                for k0 in kinds:
                    plan.pin(F, "pull", k0 + 3 * k1)
                    ys.append(c.hop1(plan, xe_of[0], sc))
                assert all(_same(y, ys[0]) for y in ys), "hop 1 depends on hop 0's kernel: %s/%s F %d k1 %d" % (graph, opts, F, k1)
            if F in NOT_LANES16 and 1 in kinds:  # no 16-byte lanes: kind 0 is the general kernel
                assert _same(xe_of[0], xe_of[1]), "kinds 0 and 1 differ at F = %d: %s/%s" % (F, graph, opts)
            plan.unpin(F)
    print("%s/%s: max |err| / mass: Xe %.3g, Y %.3g (bound %g)" % (graph, opts, worst[0], worst[1], gr.FP32_C))


@pytest.mark.parametrize("graph,opts", CELLS)
def test_pin_names_the_kernel(case, graph, opts):
    """Checks 1a and 1b."""
    c = case(graph)
    plan, general, fresh = c.plan(opts), c.plan(opts, row_stream=False), c.plan(opts, tag="never pinned")
    _masks(plan, graph, opts)
    for weighted in (False, True):
        sc = c.scales("randn", weighted)
        for F in ir.HOP_WIDTHS:
            X = c.X("randn", F)
            what = "%s/%s F %d weighted %s" % (graph, opts, F, weighted)
            for mask, other, name in ((4, general, "mask 4 against row_stream=False"), (0, fresh, "mask 0 against no pin")):
                plan.pin(F, "pull", mask)
                assert _same(c.pull(plan, X, sc), c.pull(other, X, sc)), "%s, pull: %s" % (name, what)
                Xe = c.hop0(other, X, sc)
                assert _same(c.hop0(plan, X, sc), Xe), "%s, gather_rows hop 0: %s" % (name, what)
                assert _same(c.hop1(plan, Xe, sc), c.hop1(other, Xe, sc)), "%s, gather_rows hop 1: %s" % (name, what)
            plan.pin(F, "pull", 4)
            plan.unpin(F)
            assert plan.auto_variant(F) == fresh.auto_variant(F), what
            for variant in ("pull", "auto"):
                assert _same(c.pull(plan, X, sc, variant), c.pull(fresh, X, sc, variant)), "after unpin, %s: %s" % (variant, what)


@pytest.mark.parametrize("graph,hop", [("boundaries", 0), ("boundaries_T", 1)])
def test_the_three_kinds_are_three_kernels(case, graph, hop):
    """Check 1c, on the side that has the long rows: boundaries' hyperedges (hop 0), boundaries_T's vertices (hop 1).  The
    other side's rows have at most 7 entries -- below kLatShortMax, so both schedules keep them in panels and kinds 1 and 2
    cannot differ there; its counts are printed, not asserted."""
    c = case(graph)
    plan = c.plan("default")
    assert plan.has_latency_schedule()
    F = 64
    X = c.X("randn", F)
    lens = np.diff(c.inc.csrptr) if hop == 0 else np.bincount(c.inc.colind, minlength=c.N)
    assert {255, 256, 257, 1023, 1024, 1025, 5000} <= set(lens.tolist())
    plan.pin(F, "pull", 4)
    Xe_fixed = c.hop0(plan, X, NONE)
    out = {0: {}, 1: {}}
    for k in (0, 1, 2):
        plan.pin(F, "pull", k + 3 * k)
        out[0][k] = c.hop0(plan, X, NONE)
        out[1][k] = c.hop1(plan, Xe_fixed, NONE)
    plan.unpin(F)
    diff = {(h, a, b): int((_bits(out[h][a]) != _bits(out[h][b])).sum()) for h in (0, 1) for a, b in ((0, 1), (1, 2))}
    for (h, a, b), n in sorted(diff.items()):
        print("%s hop %d: kinds %d and %d differ in %d of %d elements" % (graph, h, a, b, n, out[h][a].numel()))
    assert diff[hop, 0, 1] > 0, "kinds 0 and 1 gave the same bits on %s hop %d" % (graph, hop)
    assert diff[hop, 1, 2] > 0, "kinds 1 and 2 gave the same bits on %s hop %d" % (graph, hop)


@pytest.mark.parametrize("graph,opts", CELLS)
def test_bf16_rounds_the_fp32_call_once(case, graph, opts):
    """Check 5 (and 8 for the bf16 output)."""
    c = case(graph)
    plan, general = c.plan(opts), c.plan(opts, row_stream=False)
    masks = _masks(plan, graph, opts)
    for weighted in (False, True):
        sc = c.scales("randn", weighted)
        for F in BF16_WIDTHS:
            Xb = c.X("randn", F).to(torch.bfloat16)
            Xf = Xb.float()
            for m in masks:
                plan.pin(F, "pull", m)
                for variant in ("pull", "auto"):
                    what = "%s/%s F %d weighted %s mask %d variant %s" % (graph, opts, F, weighted, m, variant)
                    ybuf, Y = _guarded(torch.bfloat16, c.N, F)
                    c.pull(plan, Xb, sc, variant, out=Y)
                    want = c.pull(plan, Xf, sc, variant).to(torch.bfloat16)
                    assert _same(Y, want), "bf16 is not the rounded fp32 call: " + what
                    assert _guards_intact(ybuf) and not bool(torch.isnan(Y).any()), "guard bands: " + what
            plan.unpin(F)
            got = c.pull(general, Xb, sc)
            assert _same(got, c.pull(general, Xf, sc).to(torch.bfloat16)), "row_stream=False, no pin: %s/%s F %d weighted %s" % (
                graph, opts, F, weighted)


@pytest.mark.parametrize("graph,opts", CELLS)
def test_weighted_entries_run_the_pinned_schedule(case, graph, opts):
    """Check 6."""
    c = case(graph)
    plan = c.plan(opts)
    mask = 8 if 8 in _masks(plan, graph, opts) else 4
    ones = torch.ones(c.nnz, device=DEV)
    for F in ir.WIDTHS:
        X = c.X("randn", F)
        plan.pin(F, "pull", mask)
        for weighted in (False, True):
            sc = c.scales("randn", weighted)
            what = "%s/%s F %d weighted %s mask %d" % (graph, opts, F, weighted, mask)
            ref, ref_xe = c.pull(plan, X, sc), c.hop0(plan, X, sc)
            for name, w in (("NULL", None), ("unit", ones)):
                Xe = torch.empty(c.M, F, device=DEV)
                Y = plan.aggregate_incidence(c.ptr, c.ind, X, w, w, *sc, xe_out=Xe)
                assert _same(Y, ref), "%s weights differ from the unweighted pull: %s" % (name, what)
                assert _same(Xe, ref_xe), "%s weights: xe_out differs from hop 0: %s" % (name, what)
        plan.unpin(F)
    H, C = ir.EXACT_PAIRS[0]
    F = H * C
    X = c.X("randn", F)
    rng = np.random.default_rng(31)
    v2e, e2v = (torch.from_numpy(rng.random((c.nnz, H)).astype(np.float32) + 0.25).to(DEV) for _ in range(2))
    sc = c.scales("randn", True)
    plan.pin(F, "pull", mask)
    Xe = torch.empty(c.M, F, device=DEV)
    Y = plan.aggregate_incidence(c.ptr, c.ind, X, v2e, e2v, *sc, xe_out=Xe, heads=H)
    for h in range(H):
        one_xe = torch.empty(c.M, F, device=DEV)
        one = plan.aggregate_incidence(c.ptr, c.ind, X, v2e[:, h].contiguous(), e2v[:, h].contiguous(), *sc, xe_out=one_xe)
        cols = slice(h * C, (h + 1) * C)
        assert _same(Y[:, cols], one[:, cols]), "Y head %d: %s/%s mask %d" % (h, graph, opts, mask)
        assert _same(Xe[:, cols], one_xe[:, cols]), "xe_out head %d: %s/%s mask %d" % (h, graph, opts, mask)
    plan.unpin(F)


@pytest.mark.parametrize("F", [32, 33])
def test_tuner_and_pin_agree(case, F):
    """Check 7."""
    c = case("ragged")
    tuned_plan, pinned, never = (c.plan("default", tag="%s %d" % (t, F)) for t in ("tuned", "pinned", "never tuned"))
    X = c.X("randn", F)
    left = torch.full((c.N, F), NAN, device=DEV)
    tuned = tuned_plan.tune(c.ptr, c.ind, X, iters=5, out=left)
    print("ragged F %d: tuner chose %s, pull_hop_kernels %d" % (F, tuned["variant"], tuned["pull_hop_kernels"]))
    assert _same(c.pull(tuned_plan, X, NONE, "auto"), left)
    pinned.pin(F, **{k: tuned[k] for k in ("variant", "pull_hop_kernels")})
    assert pinned.auto_variant(F) == tuned["variant"]
    assert _same(c.pull(pinned, X, NONE, "auto"), left), "the pinned plan does not reproduce the tuner's result: %s" % (tuned,)
    assert _same(c.pull(pinned, X, NONE, "pull"), c.pull(tuned_plan, X, NONE, "pull")), "forced pull: %s" % (tuned,)
    base = {v: c.pull(never, X, NONE, v) for v in ("auto", "pull")}
    for p in (pinned, tuned_plan):
        p.unpin(F)
        assert p.auto_variant(F) == never.auto_variant(F)
        for v in ("auto", "pull"):
            assert _same(c.pull(p, X, NONE, v), base[v]), "after unpin, %s" % v
