"""The weighted (WT) and multi-head (WH) row gathers behind hg_aggr_incidence_f32 / hg_aggr_incidence_heads_f32 on every plan
schedule: each graph of _incidence_ref.GRAPHS under each plan-option set of _incidence_ref.option_sets(), all with
row_stream=False, so the unweighted variant="pull" call on the same plan runs the same panels and wave tasks.
test_incidence_schedules_host.py shows what the matrix reaches (full panels, empty rows at a panel's ends, both cuts at
-1 / 0 / +1, partial slots, two fixup levels, the remap's remainder) and vets the integer inputs of check 4.

Widths: single head F in {1, 3, 4, 33, 64}; (H, C) in (2, 6), (4, 3) -- F % 4 == 0 but C % 4 != 0 --, (4, 8) -- 16-byte lanes --,
(8, 40) -- two column tiles, head 6 straddles column 256.

1. NULL and unit weights give the unweighted pull of the same plan bit for bit (xe_out: its hop 1, hg_gather_rows_f32), with
   and without degE / degV / W; powers of two, another per head, scale it exactly; two calls agree; guards stay.
2. Head h's columns of Y and xe_out have the bits of the single-head call on the same plan, weights from a softmax.
3. Signed random weights with 10 % exact zeros, v2e and e2v distinct, each alone and both, with the scales and without: Y
   and xe_out within FP32_C of the mass of the float64 answer (test_incidence_aggr.test_accuracy_against_float64's bound).
4. Integer X and weights whose every partial sum is exact in fp32: Y and xe_out equal the float64 answer exactly on all
   seven option sets, and so each other bit for bit.
5. `wide`, the largest panel the weighted entry's LDS formula lets through: checks 1 and 3; one panel row more: a weighted
   call is refused and writes nothing, the NULL-weight call still runs.
6. The same on a plan after Plan.tune.
"""
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

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV, SENTINEL, _bits = ar.DEV, ar.SENTINEL, ar.bits
GUARD = 64  # floats: 256 bytes, so a guarded output keeps its 16-byte alignment
SINGLE_F = max(max(ir.WIDTHS), 32)  # the single-head inputs are drawn once at this width; narrower calls take its first columns
KINDS = [("single", F) for F in ir.WIDTHS] + list(ir.PAIRS)
WIDE_KINDS = [("single", 32), (4, 8)]
CELLS = [(g, s) for g in ir.GRAPHS for s in ir.OPTION_SETS if s != "wide"]
COMBOS = ("both", "v2e", "e2v")


def _guarded(*shape):
    """(buffer, view): a SENTINEL-filled buffer and the output inside it, GUARD words on either side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _written_inside_guards(buf, view):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()) and not bool((view == SENTINEL).any())


def _col(t, h):
    return None if t is None else t[:, h].contiguous()


def _hop1(graph, x, v2e, heads):
    """Hop 1's table in float64, head h's columns weighted by column h of v2e."""
    C = x.shape[1] // heads
    return torch.cat([ir.hop1(graph, x[:, h * C:(h + 1) * C], None if v2e is None else (v2e if heads == 1 else v2e[:, h]))
                      for h in range(heads)], 1)


def _aggr(graph, x, v2e, e2v, heads):
    return hr.incidence_aggr(graph, x, v2e, e2v, heads) if heads > 1 else ir.incidence_aggr(graph, x, v2e, e2v)


def _abs(t):
    return None if t is None else t.abs()


class _Case:
    """One graph on the device: its plans (one per option set), scales, inputs per kind of width and the float64 answers,
    which depend on the graph alone and are shared by the option sets."""

    def __init__(self, hg, name):
        self.name = name
        self.inc = inc = synth.cora_shape() if name == "cora" else ir.schedule_graph(name)
        self.h = hg.HyperGraph.from_incidence(inc, DEV, data_name=name, ngs=1 << 30)
        self.ptr, self.ind = self.h.H_T_csrptr, self.h.H_T_colind
        self.N, self.M, self.nnz = inc.N, inc.M, inc.nnz
        rng = np.random.default_rng(11)
        self.W = torch.from_numpy(rng.random(inc.M).astype(np.float32) + 0.5).to(DEV)
        self.degE, self.degV = self.h.degE.reshape(-1), self.h.degV.reshape(-1)  # degE = inf on empty hyperedges
        self._plans, self._inputs, self._graphs, self._refs, self._soft = {}, {}, {}, {}, {}

    def plan(self, opts):
        """The plan of an option set (a name of ir.option_sets()) or of explicit make_opts keywords."""
        from hypergef_amd.plan import Plan, make_opts
        key = opts if isinstance(opts, str) else tuple(sorted(opts.items()))
        if key not in self._plans:
            kw = ir.option_sets()[opts] if isinstance(opts, str) else opts
            self._plans[key] = Plan.from_tensors(self.N, self.ptr, self.ind, make_opts(row_stream=False, **kw))
        return self._plans[key]

    def scales(self, on):
        return (self.degE, self.degV, self.W) if on else (None, None, None)

    def graph(self, on):
        """The _grad_ref.Graph with these scales, on the device: the float64 answers are computed there (ir.graph_on)."""
        if on not in self._graphs:
            self._graphs[on] = ir.graph_on(gr.Graph(self.inc, *self.scales(on)), DEV)
        return self._graphs[on]

    def inputs(self, kind):
        """(X, v2e, e2v, heads) on the device: X normal, the weights signed with 10 % exact zeros.  kind ("single", F): the
        first F columns of one [N, SINGLE_F] draw and weights [nnz]; kind (H, C): X [N, H C], weights [nnz, H]."""
        heads, F = (1, SINGLE_F) if kind[0] == "single" else (kind[0], kind[0] * kind[1])
        key = (heads, F)
        if key not in self._inputs:
            rng = np.random.default_rng(100 + 7 * heads + F)
            X = rng.standard_normal((self.N, F)).astype(np.float32)
            w = rng.standard_normal((2, self.nnz) + (() if heads == 1 else (heads,))).astype(np.float32)
            w[rng.random(w.shape) < 0.1] = 0.0
            self._inputs[key] = tuple(torch.from_numpy(a.copy()).to(DEV) for a in (X, w[0], w[1])) + (heads,)
        X, v2e, e2v, heads = self._inputs[key]
        return (X[:, :kind[1]].contiguous() if kind[0] == "single" else X), v2e, e2v, heads

    def ref(self, kind, what, on):
        """(Y, mass of Y, hop 1's table, its mass) in float64 for the inputs of `kind` with the weight arrays `what` names; the
        mass is the same expression on absolute values (_grad_ref).  Computed once per graph, never modified; a narrower
        single-head kind takes the first columns."""
        full = ("single", SINGLE_F) if kind[0] == "single" else kind
        key = (full, what, on)
        if key not in self._refs:
            X, v2e, e2v, heads = self.inputs(full)
            x, a, b = X.double(), (v2e.double() if what != "e2v" else None), (e2v.double() if what != "v2e" else None)
            g = self.graph(on)
            xkey = (full, a is not None, on, "xe")
            if xkey not in self._refs:
                self._refs[xkey] = (_hop1(g, x, a, heads), _hop1(g.abs(), x.abs(), _abs(a), heads))
            self._refs[key] = (_aggr(g, x, a, b, heads), _aggr(g.abs(), x.abs(), _abs(a), _abs(b), heads)) + self._refs[xkey]
        out = self._refs[key]
        return tuple(t[:, :kind[1]] for t in out) if kind[0] == "single" else out

    def softmax_weights(self, H):
        """Positive weights [nnz, H] per hop, a softmax's output over each hyperedge / each vertex (scores of max |.| = 4)."""
        if H not in self._soft:
            g = torch.Generator(device=DEV).manual_seed(51)
            sv, se = torch.randn(self.N, H, device=DEV, generator=g), torch.randn(self.M, H, device=DEV, generator=g)
            sv, se = sv * (4.0 / float(sv.abs().max())), se * (4.0 / float(se.abs().max()))
            p = self.plan("default")
            self._soft[H] = (p.incidence_attention(self.ptr, self.ind, sv, se, "hyperedge", 0.2, heads=H),
                             p.incidence_attention(self.ptr, self.ind, sv, se, "vertex", 0.2, heads=H))
        return self._soft[H]


_CASES = {}


@pytest.fixture
def case(hg):
    def get(name):
        if name not in _CASES:
            _CASES.clear()  # one graph at a time: its float64 answers are kept while its option sets run
            torch.cuda.empty_cache()
            _CASES[name] = _Case(hg, name)
        return _CASES[name]
    return get


def _check_unit_weights(c, plan, kinds, what):
    """Check 1 on one plan."""
    for kind in kinds:
        X, _, _, heads = c.inputs(kind)
        F, C = X.shape[1], X.shape[1] // heads
        wshape = (c.nnz,) if heads == 1 else (c.nnz, heads)
        ones = torch.ones(wshape, device=DEV)
        if heads == 1:
            kv, ke = torch.tensor([-3.0], device=DEV), torch.tensor([5.0], device=DEV)
        else:  # another power per head
            kv = torch.tensor([(h % 5) - 2 for h in range(heads)], device=DEV, dtype=torch.float32)
            ke = torch.tensor([(h % 3) - 1 for h in range(heads)], device=DEV, dtype=torch.float32)
        pv, pe = ((ones.view(c.nnz, heads) * torch.exp2(k)).view(wshape) for k in (kv, ke))
        for on in (True, False):
            degE, degV, W = c.scales(on)
            msg = "%s %s scales %s" % (what, kind, on)
            ref = plan.aggregate(c.ptr, c.ind, X, degE, degV, W, variant="pull", bind_scales=False)
            ref_xe = plan.gather_rows(0, c.ptr, c.ind, X, degE, W)
            for name, wv, we in (("NULL", None, None), ("unit", ones, ones)):
                ybuf, Y = _guarded(c.N, F)
                xbuf, Xe = _guarded(c.M, F)
                plan.aggregate_incidence(c.ptr, c.ind, X, wv, we, degE, degV, W, xe_out=Xe, out=Y, heads=heads)
                again = plan.aggregate_incidence(c.ptr, c.ind, X, wv, we, degE, degV, W, heads=heads)
                assert torch.equal(_bits(Y), _bits(ref)), "%s weights differ from the unweighted pull: %s" % (name, msg)
                assert torch.equal(_bits(Xe), _bits(ref_xe)), "%s weights: xe_out differs from the unweighted hop 1: %s" % (name, msg)
                assert torch.equal(_bits(again), _bits(Y)), "two calls differ (%s weights): %s" % (name, msg)
                assert _written_inside_guards(ybuf, Y) and _written_inside_guards(xbuf, Xe), "guards (%s weights): %s" % (name, msg)
            got = plan.aggregate_incidence(c.ptr, c.ind, X, pv, pe, degE, degV, W, heads=heads)
            want = ref * torch.exp2(kv + ke).repeat_interleave(C)
            assert torch.equal(_bits(got), _bits(want)), "power-of-two weights do not scale the pull exactly: " + msg


def _check_accuracy(c, plan, kinds, what):
    """Check 3 on one plan."""
    for kind in kinds:
        X, v2e, e2v, heads = c.inputs(kind)
        F = X.shape[1]
        for on in (True, False):
            degE, degV, W = c.scales(on)
            for combo in COMBOS:
                wv, we = (v2e if combo != "e2v" else None), (e2v if combo != "v2e" else None)
                Xe = torch.empty(c.M, F, device=DEV)
                Y = plan.aggregate_incidence(c.ptr, c.ind, X, wv, we, degE, degV, W, xe_out=Xe, heads=heads)
                y, y_mass, xe, xe_mass = c.ref(kind, combo, on)
                msg = "%s %s scales %s weights %s" % (what, kind, on, combo)
                print("%s: max |err| / mass: Y %.3g, xe_out %.3g" % (
                    msg, float(((Y.double() - y).abs() / y_mass.clamp(min=gr.TINY)).max()) if y.numel() else 0.0,
                    float(((Xe.double() - xe).abs() / xe_mass.clamp(min=gr.TINY)).max()) if xe.numel() else 0.0))
                gr.assert_within(Y, y, y_mass, gr.FP32_C, msg + " Y")
                gr.assert_within(Xe, xe, xe_mass, gr.FP32_C, msg + " xe_out")


@pytest.mark.parametrize("graph,opts", CELLS)
def test_unit_and_null_weights_are_the_unweighted_pull(case, graph, opts):
    c = case(graph)
    _check_unit_weights(c, c.plan(opts), KINDS, "%s/%s" % (graph, opts))


@pytest.mark.parametrize("graph,opts", CELLS)
def test_head_columns_equal_the_single_head_calls(case, graph, opts):
    c = case(graph)
    plan = c.plan(opts)
    for H, C in ir.PAIRS:
        F = H * C
        X = c.inputs((H, C))[0]
        v2e, e2v = c.softmax_weights(H)
        none, full = (None, None, None), c.scales(True)
        for wv, we, scales in ((v2e, e2v, none), (v2e, None, full), (None, e2v, full), (v2e, e2v, full)):
            what = "%s/%s (%d, %d) v2e %s e2v %s scales %s" % (graph, opts, H, C, wv is not None, we is not None, scales[0] is not None)
            ybuf, Y = _guarded(c.N, F)
            xbuf, Xe = _guarded(c.M, F)
            plan.aggregate_incidence(c.ptr, c.ind, X, wv, we, *scales, xe_out=Xe, out=Y, heads=H)
            assert _written_inside_guards(ybuf, Y) and _written_inside_guards(xbuf, Xe), what
            for h in range(H):
                one_xe = torch.empty(c.M, F, device=DEV)
                one = plan.aggregate_incidence(c.ptr, c.ind, X, _col(wv, h), _col(we, h), *scales, xe_out=one_xe)
                cols = slice(h * C, (h + 1) * C)
                assert torch.equal(_bits(Y[:, cols]), _bits(one[:, cols])), "Y head %d: %s" % (h, what)
                assert torch.equal(_bits(Xe[:, cols]), _bits(one_xe[:, cols])), "xe_out head %d: %s" % (h, what)


@pytest.mark.parametrize("graph,opts", CELLS)
def test_accuracy_against_float64(case, graph, opts):
    c = case(graph)
    _check_accuracy(c, c.plan(opts), KINDS, "%s/%s" % (graph, opts))


@pytest.mark.parametrize("graph", ir.GRAPHS)
def test_every_schedule_gives_the_same_exact_answer(case, graph):
    """The inputs are those test_incidence_schedules_host.test_integer_inputs_stay_exact_in_fp32 vets: no sum can round, so
    no rounding bound is involved."""
    c = case(graph)
    g = c.graph(False)
    for heads, F in [(1, max(ir.WIDTHS))] + [(h, h * cc) for h, cc in ir.EXACT_PAIRS]:
        Xn, an, bn = ir.integer_inputs(c.inc, F, heads)
        Xd, v2e, e2v = (torch.from_numpy(t).to(DEV) for t in (Xn, an, bn))
        want = _aggr(g, Xd.double(), v2e.double(), e2v.double(), heads)
        want_xe = _hop1(g, Xd.double(), v2e.double(), heads)
        for Fw in (ir.WIDTHS if heads == 1 else (F,)):
            X = Xd[:, :Fw].contiguous()
            first = None
            for opts in ir.OPTION_SETS:
                what = "%s/%s heads %d F %d" % (graph, opts, heads, Fw)
                Xe = torch.empty(c.M, Fw, device=DEV)
                Y = c.plan(opts).aggregate_incidence(c.ptr, c.ind, X, v2e, e2v, xe_out=Xe, heads=heads)
                assert torch.equal(Y.double(), want[:, :Fw]), "Y is not the exact answer: " + what
                assert torch.equal(Xe.double(), want_xe[:, :Fw]), "xe_out is not the exact answer: " + what
                if first is None:
                    first = (Y, Xe)
                assert torch.equal(_bits(Y), _bits(first[0])) and torch.equal(_bits(Xe), _bits(first[1])), "bits differ: " + what


@pytest.mark.parametrize("graph", ["ragged", "boundaries"])
def test_largest_panel_the_lds_takes(case, graph):
    """(4 * panel_rows + 1 + 2 * panel_nnz) * 4 bytes of LDS at panel_nnz = 16384: panel_rows = 2047 is 12 bytes short of the
    160 KiB a workgroup can have."""
    c = case(graph)
    plan = c.plan("wide")
    assert ir.weighted_lds_bytes(plan.info["panel_rows"], plan.info["panel_nnz"]) <= ir.LDS_BYTES
    assert ir.weighted_lds_bytes(plan.info["panel_rows"] + 1, plan.info["panel_nnz"]) > ir.LDS_BYTES
    _check_unit_weights(c, plan, WIDE_KINDS, "%s/wide" % graph)
    _check_accuracy(c, plan, WIDE_KINDS, "%s/wide" % graph)


@pytest.mark.parametrize("graph", ["ragged", "boundaries"])
def test_one_panel_row_more_is_refused_for_weights_only(case, graph):
    from hypergef_amd import _lib
    c = case(graph)
    plan = c.plan(dict(panel_rows=ir.wide_panel_rows() + 1, panel_nnz=ir.PANEL_NNZ_MAX))
    for kind in WIDE_KINDS:
        X, v2e, e2v, heads = c.inputs(kind)
        F = X.shape[1]
        Y, Xe = torch.full((c.N, F), SENTINEL, device=DEV), torch.full((c.M, F), SENTINEL, device=DEV)
        for wv, we in ((v2e, e2v), (v2e, None), (None, e2v)):
            with pytest.raises(_lib.HgError, match="LDS") as err:
                plan.aggregate_incidence(c.ptr, c.ind, X, wv, we, *c.scales(True), xe_out=Xe, out=Y, heads=heads)
            assert err.value.status == _lib.HG_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((Y == SENTINEL).all()) and bool((Xe == SENTINEL).all()), kind
        for on in (True, False):  # no weight array: the unweighted instances, whose LDS holds no weights
            degE, degV, W = c.scales(on)
            got = plan.aggregate_incidence(c.ptr, c.ind, X, None, None, degE, degV, W, xe_out=Xe, out=Y, heads=heads)
            assert torch.equal(_bits(got), _bits(plan.aggregate(c.ptr, c.ind, X, degE, degV, W, variant="pull", bind_scales=False)))
            assert torch.equal(_bits(Xe), _bits(plan.gather_rows(0, c.ptr, c.ind, X, degE, W)))


@pytest.mark.parametrize("graph", ["toy", "ragged", "cora"])
def test_tuned_plan(case, graph):
    """After Plan.tune at F = 32 the weighted entry runs, per hop, the schedule of the kernel the tuner pinned for that width
    (aggr_incidence: sched_lat where it pinned the latency schedule, else sched), and so does the forced pull call.  Which
    kernels the tuner pins is a timing outcome: the assertions hold whatever it pins, and that this test runs aggr_incidence's
    sched_lat branch is not guaranteed.  The `lat` option set runs the same schedule geometry (short_max = kLatShortMax)
    unconditionally."""
    c = case(graph)
    plan = c.plan(dict())
    assert c.nnz <= 1 << 18  # the plan has a latency schedule to pin
    X = c.inputs(("single", 32))[0]
    info = plan.tune(c.ptr, c.ind, X, iters=5)
    print("%s: tuned pull_hop_kernels %d, variant %s" % (graph, info["pull_hop_kernels"], info["variant"]))
    _check_unit_weights(c, plan, WIDE_KINDS, "%s/tuned" % graph)
    _check_accuracy(c, plan, WIDE_KINDS, "%s/tuned" % graph)
    # and not left to the tuner: the plan's schedule, then the latency schedule, named on both hops with Plan.pin (kind 0
    # is kind 1 on these row_stream=False plans; WIDE_KINDS are both 32 columns wide)
    assert plan.has_latency_schedule()
    for mask in (1 + 3 * 1, 2 + 3 * 2, 1 + 3 * 2, 2 + 3 * 1):
        plan.pin(32, "pull", mask)
        _check_unit_weights(c, plan, WIDE_KINDS, "%s/pinned %d" % (graph, mask))
        _check_accuracy(c, plan, WIDE_KINDS, "%s/pinned %d" % (graph, mask))
    plan.unpin(32)
