"""Every lane shape of every launcher in hg_kernels.hip once: a launcher that sends a width to another (LPR, VEC) instance
than the kernel's lane layout expects reads and writes other columns, which no check of the compiled kernels can see.

One tiny hypergraph (40 vertices, 24 hyperedges): hyperedge 0 has 39 members, hyperedge 5 none, vertex 39 is isolated and
vertex 0 lies in every non-empty hyperedge, so that under the `small` plan options (_incidence_ref.option_sets) both hops
have panels, wave tasks with partial slots and fixups -- asserted from the plan's schedule.

Widths: 4-byte lanes F in (1, 2, 3, 5, 9, 17, 33) -> LPR 1 .. 64; 16-byte lanes F in (4, 8, 16, 32, 64, 128, 256) -> LPR
1 .. 64; F = 260: a second column tile.  Inputs are drawn once at 260 columns, a call takes the first F.

Comparisons are those of each operator's own test.  X in {-1, 0, 1} and weights in {-2 .. 2} (_incidence_ref.integer_inputs)
keep every partial sum an integer below 2^24, so the sums, the dots and the push path's atomics equal the float64 answer
exactly in any order; max / min and their select are compared bit for bit with _reduce_ref; the attention gather with the
composition incidence_attention + aggregate_incidence, bit for bit (test_fused_attention_gpu); a bf16 form with the float32
call on the widened rows, rounded once, bit for bit (test_incidence_bf16_gpu); hyperedge_dot and rows_dot within
test_scale_grads_gpu's bounds, 2 FP32_C + (F + 2) 2^-24 and FP32_C + (F + 1) 2^-24 of the mass.

The hub pass is not reached here: the plan builds one only for vertices of 256 and more incidences (hub_min_deg).
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
import _reduce_ref as rr  # noqa: E402
import _scale_grad_ref as sg  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV, U, _bits = ar.DEV, ar.U, ar.bits
LANE4_WIDTHS = (1, 2, 3, 5, 9, 17, 33)
LANE16_WIDTHS = (4, 8, 16, 32, 64, 128, 256)
WIDTHS = LANE4_WIDTHS + LANE16_WIDTHS + (260,)
FMAX = max(WIDTHS)
SLOPE = 0.2


def _tiny():
    rng = np.random.default_rng(7)
    N, M = 40, 24
    rows = []
    for e in range(M):
        if e == 0:
            members = np.arange(N - 1)  # cut into wave tasks, the last slot partial
        elif e == 5:
            members = np.zeros(0, np.int64)
        else:
            members = np.union1d([0], rng.choice(np.arange(1, N - 1), size=int(rng.integers(1, 5)), replace=False))
        rows.append(np.sort(members).astype(np.int32))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return synth.Incidence(N, M, ptr, np.concatenate(rows).astype(np.int32), name="tiny")


class _Case:
    """The graph on the device, its plans, the inputs at FMAX columns and the float64 references (CPU), built once."""

    def __init__(self):
        from hypergef_amd.plan import Plan, make_opts
        self.inc = inc = _tiny()
        assert inc.N == 40 and inc.M == 24 and inc.csrptr[6] == inc.csrptr[5] and inc.N - 1 not in inc.colind
        self.ptr, self.ind = torch.from_numpy(inc.csrptr).to(DEV), torch.from_numpy(inc.colind).to(DEV)
        self.N, self.M, self.nnz = inc.N, inc.M, inc.nnz
        # panels, wave tasks and fixups only: no streaming row gather
        self.tasks = Plan.from_tensors(inc.N, self.ptr, self.ind, make_opts(row_stream=False, **ir.option_sets()["small"]))
        self.stream = Plan.from_tensors(inc.N, self.ptr, self.ind, make_opts(**ir.option_sets()["small"]))
        self.g = gr.Graph(inc)
        self.idx = sg.Index(inc)
        self.E, self.V = rr.entries(inc)
        rng = np.random.default_rng(19)
        Xn, an, bn = ir.integer_inputs(inc, FMAX)
        _, a2, b2 = ir.integer_inputs(inc, 2, heads=2)
        self.X, self.v2e, self.e2v, self.v2e2, self.e2v2 = (torch.from_numpy(t) for t in (Xn, an, bn, a2, b2))
        self.B = torch.from_numpy(rng.integers(-1, 2, (inc.M, FMAX)).astype(np.float32))   # a hyperedge table
        self.A2 = torch.from_numpy(rng.integers(-1, 2, (inc.N, FMAX)).astype(np.float32))  # a second vertex table
        self.R = {0: torch.from_numpy(rng.standard_normal((inc.N, FMAX)).astype(np.float32)),
                  1: torch.from_numpy(rng.standard_normal((inc.M, FMAX)).astype(np.float32))}
        self.degE, self.degV, self.W = (torch.from_numpy(s) for s in ir.power_of_two_scales(inc))
        self.gs = gr.Graph(inc, self.degE, self.degV, self.W)

    def dev(self, t, F=None):
        return (t if F is None else t[:, :F]).contiguous().to(DEV)


_CASE = []


@pytest.fixture
def case(hg):
    if not _CASE:
        _CASE.append(_Case())
    return _CASE[0]


def _exact(got, want, what):
    assert torch.equal(got.double().cpu(), want), what + ": not the exact float64 answer"


def test_the_plan_has_panels_tasks_and_fixups(case):
    for plan in (case.tasks, case.stream):
        for hop in (0, 1):
            s = plan.schedule(hop)
            assert len(s["panels"]) > 0 and len(s["tasks"]) > 0 and len(s["fixups"]) > 0, (hop, {k: len(v) for k, v in s.items()})


@pytest.mark.parametrize("F", WIDTHS)
def test_plain_gather_pull_stream_fused_and_push(case, F):
    """launch_gather and launch_fixups (the panel / task schedule), launch_stream_rows (pinned kind 0), launch_fused and
    launch_push: integer inputs, with power-of-two scales and without."""
    c = case
    X = c.dev(c.X, F)
    for g, sc in ((c.g, (None, None, None)), (c.gs, tuple(c.dev(t) for t in (c.degE, c.degV, c.W)))):
        x = c.X[:, :F].double()
        want_xe, want_y = ir.hop1(g, x), ir.incidence_aggr(g, x)
        what = "F %d scales %s" % (F, sc[0] is not None)
        xe = c.tasks.gather_rows(0, c.ptr, c.ind, X, sc[0], sc[2])
        _exact(xe, want_xe, "hop 0 " + what)
        _exact(c.tasks.gather_rows(1, c.ptr, c.ind, xe, sc[1], None), want_y, "hop 1 " + what)
        _exact(c.tasks.aggregate(c.ptr, c.ind, X, *sc, variant="pull", bind_scales=False), want_y, "pull " + what)
        c.stream.pin(F, "pull", 0)
        try:
            _exact(c.stream.aggregate(c.ptr, c.ind, X, *sc, variant="pull", bind_scales=False), want_y, "streamed pull " + what)
            _exact(c.stream.gather_rows(0, c.ptr, c.ind, X, sc[0], sc[2]), want_xe, "streamed hop 0 " + what)
        finally:
            c.stream.unpin(F)
        _exact(c.tasks.aggregate(c.ptr, c.ind, X, *sc, variant="fused", bind_scales=False), want_y, "fused " + what)
        _exact(c.tasks.aggregate(c.ptr, c.ind, X, *sc, variant="push_atomic", bind_scales=False), want_y, "push " + what)


@pytest.mark.parametrize("F", WIDTHS)
def test_weighted_and_per_head_gather(case, F):
    """launch_gather_weighted; launch_gather_heads with heads = 2 where F is even."""
    c = case
    X, x = c.dev(c.X, F), c.X[:, :F].double()
    for heads, a, b in ((1, c.v2e, c.e2v), (2, c.v2e2, c.e2v2)):
        if F % heads:
            continue
        xe = torch.empty(c.M, F, device=DEV)
        Y = c.tasks.aggregate_incidence(c.ptr, c.ind, X, c.dev(a), c.dev(b), xe_out=xe, heads=heads)
        what = "F %d heads %d" % (F, heads)
        want = hr.incidence_aggr(c.g, x, a.double(), b.double(), heads) if heads > 1 else ir.incidence_aggr(c.g, x, a.double(), b.double())
        _exact(Y, want, "Y " + what)
        want_xe = torch.cat([ir.hop1(c.g, x[:, h * (F // heads):(h + 1) * (F // heads)], a.double().reshape(c.nnz, heads)[:, h])
                             for h in range(heads)], 1)
        _exact(xe, want_xe, "xe_out " + what)


@pytest.mark.parametrize("F", WIDTHS)
def test_attention_gather(case, F):
    """launch_gather_attention: the bits of aggregate_incidence on the coefficients incidence_attention writes."""
    c = case
    X = c.dev(c.R[0], F)
    for heads in (1, 2):
        if F % heads:
            continue
        gen = torch.Generator().manual_seed(5 + heads)
        sv, se = torch.randn(c.N, heads, generator=gen).to(DEV), torch.randn(c.M, heads, generator=gen).to(DEV)
        if heads == 1:
            sv, se = sv.reshape(-1), se.reshape(-1)
        for group in ar.GROUPS:
            alpha = c.tasks.incidence_attention(c.ptr, c.ind, sv, se, group, SLOPE, heads=heads)
            xe, xe2 = torch.empty(c.M, F, device=DEV), torch.empty(c.M, F, device=DEV)
            want = c.tasks.aggregate_incidence(c.ptr, c.ind, X, alpha, alpha, xe_out=xe, heads=heads)
            got = c.tasks.aggregate_incidence_attention(c.ptr, c.ind, X, sv, se, group, SLOPE, xe_out=xe2, heads=heads)
            what = "F %d heads %d %s" % (F, heads, group)
            assert torch.equal(_bits(got), _bits(want)), "Y differs from the composition: " + what
            assert torch.equal(_bits(xe2), _bits(xe)), "xe_out differs from the composition: " + what


@pytest.mark.parametrize("F", WIDTHS)
def test_max_min_and_select(case, F):
    """launch_gather_reduce, modes 1 to 3."""
    c = case
    for hop in (0, 1):
        src = c.R[hop][:, :F].contiguous()
        ndst = c.M if hop == 0 else c.N
        gs = torch.from_numpy(np.random.default_rng(3 + hop).integers(-3, 4, (ndst, F)).astype(np.float32))
        for op in rr.OPS:
            what = "F %d hop %d %s" % (F, hop, op)
            val, arg = rr.reduce_hop(c.inc, hop, src, op, c.E, c.V)
            dst, got_arg = c.tasks.gather_rows_reduce(hop, c.ptr, c.ind, c.dev(src), op)
            assert torch.equal(got_arg.cpu(), arg.to(torch.int32)), "arg: " + what
            assert torch.equal(_bits(dst.cpu()), _bits(val.contiguous())), "dst is not the winner's bits: " + what
            sel = c.tasks.gather_rows_select(hop, c.ptr, c.ind, c.dev(gs), c.dev(arg.to(torch.int32)))
            _exact(sel, rr.select_grad(c.inc, hop, gs.double(), arg, c.E, c.V), "select " + what)


@pytest.mark.parametrize("F", WIDTHS)
def test_dots(case, F):
    """launch_incidence_dot, launch_incidence_dot_heads, launch_hyperedge_dot and launch_rows_dot."""
    c = case
    A, B, A2 = c.X[:, :F], c.B[:, :F], c.A2[:, :F]
    for heads in (1, 2):
        if F % heads:
            continue
        what = "F %d heads %d" % (F, heads)
        got = c.tasks.incidence_dot(c.ptr, c.ind, c.dev(A), c.dev(B), heads=heads)
        _exact(got.reshape(c.nnz, heads), hr.dot(c.idx, A, B, heads), "incidence_dot " + what)
        wa, wb = (c.v2e, c.e2v) if heads == 1 else (c.v2e2, c.e2v2)
        got = c.tasks.hyperedge_dot(c.ptr, c.ind, c.dev(A), c.dev(A2), c.dev(wa), c.dev(wb), heads=heads)
        ref = sg.edge_dot(c.idx, A.double(), wa.double(), A2.double(), wb.double(), heads)
        mass = sg.edge_dot(c.idx, A.double().abs(), wa.double().abs(), A2.double().abs(), wb.double().abs(), heads)
        gr.assert_within(got, ref, mass, 2 * gr.FP32_C + (F + 2) * U, "hyperedge_dot " + what)
    got = c.tasks.rows_dot(c.dev(A), c.dev(A2))
    gr.assert_within(got, (A.double() * A2.double()).sum(1), (A.double() * A2.double()).abs().sum(1), gr.FP32_C + (F + 1) * U,
                     "rows_dot F %d" % F)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else _bits(a),
                                                                     b.view(torch.int16) if b.dtype == torch.bfloat16 else _bits(b))


@pytest.mark.parametrize("F", [F for F in WIDTHS if F % 4 == 0])
def test_bf16_rows(case, F):
    """The (src, dst) and (A, B) forms of bf16 rows: the unweighted, weighted and per-head gathers, the fixups with bf16
    rows of Y, the dots, and the fused and pull calls on bf16 X."""
    c = case
    bf = torch.bfloat16
    X32 = c.dev(c.X, F)
    Xb = X32.to(bf)  # {-1, 0, 1}: exact
    for variant in ("pull", "fused"):
        want = c.tasks.aggregate(c.ptr, c.ind, X32, variant=variant).to(bf)
        assert _same(c.tasks.aggregate(c.ptr, c.ind, Xb, variant=variant), want), "F %d %s on bf16 X" % (F, variant)
    for heads in (1, 2):
        if (F // heads) % 4:
            continue
        for w in (None, c.v2e if heads == 1 else c.v2e2):
            wd = None if w is None else c.dev(w)
            for hop in (0, 1):
                s32 = X32 if hop == 0 else c.dev(c.B, F)
                ndst = c.M if hop == 0 else c.N
                want = c.tasks.gather_rows_incidence(hop, c.ptr, c.ind, s32, wd, heads=heads)
                for sdt, ddt in ((bf, torch.float32), (torch.float32, bf), (bf, bf)):
                    out = torch.empty(ndst, F, dtype=ddt, device=DEV)
                    got = c.tasks.gather_rows_incidence(hop, c.ptr, c.ind, s32.to(sdt), wd, heads=heads, out=out)
                    assert _same(got, want.to(ddt)), "F %d heads %d hop %d weights %s: %s -> %s" % (F, heads, hop, w is not None, sdt, ddt)
        A32, B32 = X32, c.dev(c.B, F)
        want = c.tasks.incidence_dot(c.ptr, c.ind, A32, B32, heads=heads)
        for adt, bdt in ((bf, torch.float32), (torch.float32, bf), (bf, bf)):
            got = c.tasks.incidence_dot(c.ptr, c.ind, A32.to(adt), B32.to(bdt), heads=heads)
            assert _same(got, want), "incidence_dot F %d heads %d: %s, %s" % (F, heads, adt, bdt)
