"""The max / min row gather and its select-gather (hg_gather_rows_reduce_f32, hg_gather_rows_select_f32, behind them
gather_rows_reduce_kernel and fixup_rows_reduce_kernel) on every plan schedule: each graph of _incidence_ref.GRAPHS under the
option sets default, lat, small, unit, odd, dfs, and `wide` on ragged and boundaries, all with row_stream=False.
test_reduce_schedules_host.py shows what this matrix reaches: panels with several rows per lane group at every lane width,
ties that lie across partial slots, first-level fixup groups and a wave task's lane groups, and every (VEC, LPR) lane shape.

Widths: _reduce_ref.CORE_WIDTHS on every cell, SWEEP_WIDTHS in addition on SWEEP_CELLS.  Inputs (_reduce_ref.draw, once per
graph and hop at the widest F, a call takes the first columns): randn, ties ({-1, -0.0, +0.0, 1}), inf (randn with +-inf and
one all -inf row), const (1.0).  scaleA = 1 / len (inf on an empty row), scaleB in [0.5, 1.5).  Max, min and a select of
integers never round: every check but the randn select is a comparison of bits; that one is _grad_ref.FP32_C of the mass.

1. Forward: arg equals _reduce_ref.reduce_hop's; dst has the bits of (src[ind[arg]] * scaleA) * scaleB in float32 torch; empty
   rows are +0.0 / -1; on const, arg is the row's smallest position; every option set of a graph gives the first one's bits;
   without scales the value is the winner's own bits.
2. On every call dst and arg_out lie between 256-byte guards in sentinel-filled buffers, and the workspace is exactly
   reduce_workspace_bytes(F) bytes between guards with its float half poisoned to +inf (max) / -inf (min) and its int32 half
   to 0: a slot read that the call did not write wins.  Guards stay; no sentinel stays inside.
3. Select-gather on the reference winners of (max, ties), (min, randn), (max, inf): integer gs times a per-row power of two
   equals float64 select_grad exactly; randn gs within FP32_C of the mass, two calls the same bits; workspace poisoned to
   2^20; gs, arg and src offset by 4 bytes (4-byte lanes) at F = 8 on every cell and at F = 128 (two column tiles) on
   ragged/small give the aligned call's bits and the float64 select.
4. The three sweep cells over SWEEP_WIDTHS, randn and ties.
5. `wide`: checks 1 and 3; one panel row more: both entries refuse (HG_ERR_UNSUPPORTED, "LDS") and write nothing, the sum
   gather still runs.
6. Plan.pin(F, "pull", mask) for mask in (0, 4, 8, 5, 7): the unpinned plan's bits.
7. ops.reduce_aggr, all 16 (first, second) pairs on integer inputs and power-of-two scales against _reduce_ref.reduce_aggr64:
   exact without a mean, FP32_C of the mass with one.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402
import _grad_ref as gr  # noqa: E402
import _incidence_ref as ir  # noqa: E402
import _reduce_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

DEV, SENTINEL = ar.DEV, ar.SENTINEL
ISENTINEL = -12345   # no arg: those are -1 or a position
GUARD = 64           # words: 256 bytes, so a guarded output keeps its 16-byte alignment
WS_GUARD = 256       # bytes
WS_BYTE = 0xA5
SELECT_POISON = 2.0 ** 20
INF = float("inf")


def _bits(t):
    return t.view(torch.int32)


def _guarded(shape, dtype, fill):
    """(buffer, view): a buffer filled with `fill` and the output inside it, GUARD words on either side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guard_flags(buf, view, fill, written=True):
    """0-dim bool tensors: the guards hold `fill`; no (written) or only (not written) `fill` inside."""
    inside = (view != fill).all() if written else (view == fill).all()
    return (buf[:GUARD] == fill).all() & (buf[buf.numel() - GUARD:] == fill).all(), inside


def _workspace(plan, F, poison):
    """(buffer, workspace, offset): exactly reduce_workspace_bytes(F) bytes, 256-byte aligned, inside a WS_BYTE-filled
    byte buffer; the float half (first, as reduce_hop in hg_api.hip lays them out) filled with `poison`, the int32 half 0."""
    need = plan.reduce_workspace_bytes(F)
    assert need > 0 and need % 512 == 0
    buf = torch.full((need + 3 * WS_GUARD,), WS_BYTE, dtype=torch.uint8, device=DEV)
    off = WS_GUARD + (-(buf.data_ptr() + WS_GUARD)) % 256
    ws = buf[off:off + need]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == need
    ws[:need // 2].view(torch.float32).fill_(poison)
    ws[need // 2:].view(torch.int32).fill_(0)
    return buf, ws, off


def _workspace_flag(buf, ws, off):
    return (buf[:off] == WS_BYTE).all() & (buf[off + ws.numel():] == WS_BYTE).all()


def _check(flags, what):
    """One read-back for a call's checks: flags name -> 0-dim bool tensor."""
    names = list(flags)
    got = torch.stack([flags[n] for n in names]).tolist()
    bad = [n for n, ok in zip(names, got) if not ok]
    assert not bad, "%s: %s" % (what, "; ".join(bad))


def _offset(t):
    """A copy of t that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view_as(t).copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


class _Case:
    """One graph on the device: its plans (one per option set), scales, the inputs of _reduce_ref.draw and the references,
    which depend on the graph alone, are computed once at FMAX columns and are never modified."""

    def __init__(self, hg, name):
        self.hg, self.name = hg, name
        self.inc = inc = ir.schedule_graph(name)
        self.ptr = torch.from_numpy(inc.csrptr).to(DEV)
        self.ind = torch.from_numpy(inc.colind).to(DEV)
        self.E, self.V = rr.entries(inc, DEV)
        self.len = tuple(torch.from_numpy(n).to(DEV) for n in rr.row_lengths(inc))
        rng = np.random.default_rng(3)
        self.sA = tuple(1.0 / n.float() for n in self.len)  # inf on an empty row: must not reach the result
        self.sB = tuple(torch.from_numpy(rng.random(n.numel()).astype(np.float32) + 0.5).to(DEV) for n in self.len)
        self.first = tuple(torch.from_numpy(rr.first_positions(inc, hop)).to(DEV).to(torch.int32) for hop in (0, 1))
        self._plans, self._src, self._ref, self._sel_in, self._sel_ref, self.seen = {}, {}, {}, {}, {}, {}

    def plan(self, opts):
        from hypergef_amd.plan import Plan, make_opts
        key = opts if isinstance(opts, str) else tuple(sorted(opts.items()))
        if key not in self._plans:
            kw = ir.option_sets()[opts] if isinstance(opts, str) else opts
            self._plans[key] = Plan.from_tensors(self.inc.N, self.ptr, self.ind, make_opts(row_stream=False, **kw))
        return self._plans[key]

    def nrows(self, hop):
        return (self.inc.M, self.inc.N) if hop == 0 else (self.inc.N, self.inc.M)  # (dst, src)

    def src(self, hop, kind, F):
        if (hop, kind) not in self._src:
            self._src[hop, kind] = torch.from_numpy(rr.draw(self.inc, hop, kind)).to(DEV)
        return self._src[hop, kind][:, :F].contiguous()

    def ref(self, hop, op, kind):
        """(value, arg as int32, the bits of the scaled dst) at FMAX columns."""
        key = (hop, op, kind)
        if key not in self._ref:
            val, arg = rr.reduce_hop(self.inc, hop, self.src(hop, kind, rr.FMAX), op, self.E, self.V)
            want = (val * self.sA[hop].reshape(-1, 1)) * self.sB[hop].reshape(-1, 1)
            want = torch.where(arg < 0, torch.zeros_like(want), want)
            self._ref[key] = (val, arg.to(torch.int32), _bits(want.contiguous()), arg)
        return self._ref[key]

    def select_inputs(self, hop):
        """(integers in -3 .. 3 times a per-row power of two, randn), [rows of hop's dst, FMAX]."""
        if hop not in self._sel_in:
            ndst = self.nrows(hop)[0]
            gen = torch.Generator(device=DEV).manual_seed(40 + hop)
            pow2 = torch.tensor([0.5, 1.0, 2.0, 4.0], device=DEV)[torch.randint(0, 4, (ndst,), device=DEV, generator=gen)]
            gi = torch.randint(-3, 4, (ndst, rr.FMAX), device=DEV, generator=gen).float() * pow2.reshape(-1, 1)
            self._sel_in[hop] = (gi, torch.randn(ndst, rr.FMAX, device=DEV, generator=gen))
        return self._sel_in[hop]

    def select_ref(self, hop, op, kind):
        """float64, FMAX columns: (the select of the integer gs, of the randn gs, the latter's mass)."""
        key = (hop, op, kind)
        if key not in self._sel_ref:
            arg64 = self.ref(hop, op, kind)[3]
            gi, gn = self.select_inputs(hop)
            self._sel_ref[key] = tuple(rr.select_grad(self.inc, hop, t, arg64, self.E, self.V)
                                       for t in (gi.double(), gn.double(), gn.double().abs()))
        return self._sel_ref[key]


_CASES = {}


@pytest.fixture
def case(hg):
    def get(name):
        if name not in _CASES:
            _CASES.clear()  # one graph at a time: its references are kept while its option sets run
            torch.cuda.empty_cache()
            _CASES[name] = _Case(hg, name)
        return _CASES[name]
    return get


# ---- checks 1 and 2: one forward call --------------------------------------------------------------------------------------

def _forward(c, plan, opts, hop, op, kind, F, what, scaled=True, src=None, remember=True):
    """One guarded call on a poisoned workspace, compared with the reference; returns (dst, arg)."""
    what = "%s hop %d %s %s F=%d%s" % (what, hop, op, kind, F, "" if scaled else " no scales")
    ndst = c.nrows(hop)[0]
    val, arg32, want_bits, _ = c.ref(hop, op, kind)
    if src is None:
        src = c.src(hop, kind, F)
    dbuf, dst = _guarded((ndst, F), torch.float32, SENTINEL)
    abuf, arg = _guarded((ndst, F), torch.int32, ISENTINEL)
    wbuf, ws, off = _workspace(plan, F, INF if op == "max" else -INF)
    sA, sB = (c.sA[hop], c.sB[hop]) if scaled else (None, None)
    got = plan.gather_rows_reduce(hop, c.ptr, c.ind, src, op, sA, sB, out=dst, arg_out=arg, workspace=ws)
    assert got[0] is dst and got[1] is arg
    empty = c.len[hop] == 0
    flags = {"arg differs from the reference": (arg == arg32[:, :F]).all()}
    if scaled:
        flags["dst is not (src[ind[arg]] * scaleA) * scaleB"] = (_bits(dst) == want_bits[:, :F]).all()
    else:
        flags["dst is not the winner's bits"] = (_bits(dst) == _bits(val)[:, :F]).all()
    flags["an empty row is not +0.0 / -1"] = (((arg == -1) & (_bits(dst) == 0)) | ~empty.reshape(-1, 1)).all()
    if kind == "const":
        flags["const: arg is not the row's smallest position"] = (arg == c.first[hop].reshape(-1, 1)).all()
    flags["dst guards"], flags["a sentinel is left in dst"] = _guard_flags(dbuf, dst, SENTINEL)
    flags["arg_out guards"], flags["a sentinel is left in arg_out"] = _guard_flags(abuf, arg, ISENTINEL)
    flags["workspace guards"] = _workspace_flag(wbuf, ws, off)
    key = (hop, op, kind, F, scaled)
    if remember and key in c.seen:
        name, d0, a0 = c.seen[key]
        flags["bits differ between the option sets %s and %s" % (name, opts)] = (_bits(dst) == _bits(d0)).all() & (arg == a0).all()
    _check(flags, what)
    if remember and key not in c.seen:
        c.seen[key] = (opts, dst, arg)
    return dst, arg


def _check_forward(c, opts, widths, kinds, what):
    plan = c.plan(opts)
    for F in widths:
        for hop in (0, 1):
            for op in rr.OPS:
                for kind in kinds:
                    _forward(c, plan, opts, hop, op, kind, F, what)
    for hop in (0, 1):  # once per cell without scales
        _forward(c, plan, opts, hop, "max", "ties", 65, what, scaled=False)


# ---- check 3: one select call ----------------------------------------------------------------------------------------------

def _select(c, plan, hop, op, kind, F, what, misaligned=False):
    what = "%s select of hop %d (%s, %s) F=%d%s" % (what, hop, op, kind, F, " offset by 4 bytes" if misaligned else "")
    nsrc = c.nrows(hop)[1]
    arg = c.ref(hop, op, kind)[1][:, :F].contiguous()
    gi, gn = (t[:, :F].contiguous() for t in c.select_inputs(hop))
    want, want_n, mass_n = (t[:, :F] for t in c.select_ref(hop, op, kind))
    if misaligned:
        arg, gi = _offset(arg), _offset(gi)

    def run(gs):
        obuf, out = _guarded((nsrc, F), torch.float32, SENTINEL)
        wbuf, ws, off = _workspace(plan, F, SELECT_POISON)
        assert plan.gather_rows_select(hop, c.ptr, c.ind, gs, arg, out=out, workspace=ws) is out
        return out, _guard_flags(obuf, out, SENTINEL) + (_workspace_flag(wbuf, ws, off),)

    got, (g0, g1, g2) = run(gi)
    _check({"integer gs: not the float64 select": (got.double() == want).all(), "dsrc guards": g0,
            "a sentinel is left in dsrc": g1, "workspace guards": g2}, what)
    if misaligned:
        return
    got_n, (g0, g1, g2) = run(gn)
    again, _ = run(gn)
    _check({"two calls differ": (_bits(got_n) == _bits(again)).all(), "dsrc guards": g0, "a sentinel is left in dsrc": g1,
            "workspace guards": g2}, what + " randn gs")
    ir.within_on_device(got_n, want_n, mass_n, gr.FP32_C, what + " randn gs")


def _check_select(c, opts, widths, winners, what):
    plan = c.plan(opts)
    for F in widths:
        for hop in (0, 1):
            for op, kind in winners:
                _select(c, plan, hop, op, kind, F, what)


def _check_misaligned(c, opts, F, what):
    """Rows offset by 4 bytes take the 4-byte lanes: max / min give the aligned call's bits (which _forward compares with the
    reference), the select of the integer gs the float64 answer."""
    plan = c.plan(opts)
    assert rr.lane_shape(F, aligned=False)[0] == 1 and rr.lane_shape(F)[0] == 4
    for hop in (0, 1):
        for op in rr.OPS:
            src = c.src(hop, "randn", F)
            a = _forward(c, plan, opts, hop, op, "randn", F, what, remember=False)
            b = _forward(c, plan, opts, hop, op, "randn", F, what + " src offset by 4 bytes", src=_offset(src), remember=False)
            assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]), "%s hop %d %s F=%d: offset src" % (what, hop, op, F)
        _select(c, plan, hop, "max", "ties", F, what, misaligned=True)


@pytest.mark.parametrize("graph,opts", [(g, s) for g, s in rr.cells() if s != "wide"])
def test_forward_equals_the_reference(case, graph, opts):
    c = case(graph)
    _check_forward(c, opts, rr.CORE_WIDTHS, rr.KINDS, "%s/%s" % (graph, opts))


@pytest.mark.parametrize("graph,opts", [(g, s) for g, s in rr.cells() if s != "wide"])
def test_select_gather(case, graph, opts):
    c = case(graph)
    what = "%s/%s" % (graph, opts)
    _check_select(c, opts, rr.CORE_WIDTHS, rr.SELECT_WINNERS, what)
    _check_misaligned(c, opts, rr.MISALIGNED_F, what)
    if (graph, opts) == rr.MISALIGNED_TILES_CELL:
        assert rr.lane_shape(rr.MISALIGNED_TILES_F, aligned=False) == (1, 64, 2)
        _check_misaligned(c, opts, rr.MISALIGNED_TILES_F, what)


# ---- check 4: the lane-width sweep -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph,opts", rr.SWEEP_CELLS)
def test_lane_width_sweep(case, graph, opts):
    c = case(graph)
    what = "%s/%s" % (graph, opts)
    _check_forward(c, opts, rr.SWEEP_WIDTHS, rr.SWEEP_KINDS, what)
    _check_select(c, opts, rr.SWEEP_WIDTHS, [w for w in rr.SELECT_WINNERS if w[1] in rr.SWEEP_KINDS], what)


# ---- check 5: the largest panel, and the refusal one panel row above it --------------------------------------------------

@pytest.mark.parametrize("graph", rr.WIDE_GRAPHS)
def test_largest_panel_the_lds_takes(case, graph):
    c = case(graph)
    plan = c.plan("wide")
    assert ir.weighted_lds_bytes(plan.info["panel_rows"], plan.info["panel_nnz"]) <= ir.LDS_BYTES
    assert ir.weighted_lds_bytes(plan.info["panel_rows"] + 1, plan.info["panel_nnz"]) > ir.LDS_BYTES
    what = "%s/wide" % graph
    _check_forward(c, "wide", rr.CORE_WIDTHS, rr.KINDS, what)
    _check_select(c, "wide", rr.CORE_WIDTHS, rr.SELECT_WINNERS, what)
    _check_misaligned(c, "wide", rr.MISALIGNED_F, what)


@pytest.mark.parametrize("graph", rr.WIDE_GRAPHS)
def test_one_panel_row_more_is_refused(case, graph):
    from hypergef_amd import _lib
    c = case(graph)
    plan = c.plan(dict(panel_rows=ir.wide_panel_rows() + 1, panel_nnz=ir.PANEL_NNZ_MAX))
    F = 33
    for hop in (0, 1):
        ndst, nsrc = c.nrows(hop)
        src = c.src(hop, "randn", F)
        dst = torch.full((ndst, F), SENTINEL, device=DEV)
        arg = torch.full((ndst, F), ISENTINEL, dtype=torch.int32, device=DEV)
        dsrc = torch.full((nsrc, F), SENTINEL, device=DEV)
        for op in rr.OPS:
            with pytest.raises(_lib.HgError, match="LDS") as err:
                plan.gather_rows_reduce(hop, c.ptr, c.ind, src, op, c.sA[hop], c.sB[hop], out=dst, arg_out=arg)
            assert err.value.status == _lib.HG_ERR_UNSUPPORTED
        with pytest.raises(_lib.HgError, match="LDS") as err:
            plan.gather_rows_select(hop, c.ptr, c.ind, c.select_inputs(hop)[0][:, :F].contiguous(),
                                    c.ref(hop, "max", "ties")[1][:, :F].contiguous(), out=dsrc)
        assert err.value.status == _lib.HG_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((dst == SENTINEL).all()) and bool((arg == ISENTINEL).all()) and bool((dsrc == SENTINEL).all()), hop
        # the unweighted sum stages no positions: it runs, and on integers its sum is exact in any order
        xi = torch.from_numpy(np.random.default_rng(5).integers(-3, 4, (nsrc, F)).astype(np.float32)).to(DEV)
        rows, other = (c.E, c.V) if hop == 0 else (c.V, c.E)
        want = torch.zeros(ndst, F, dtype=torch.float64, device=DEV).index_add_(0, rows, xi.double()[other])
        assert 3 * int(c.len[hop].max()) < 2 ** 24
        assert torch.equal(plan.gather_rows(hop, c.ptr, c.ind, xi).double(), want), "the sum gather on hop %d" % hop


# ---- check 6: pinned kernels -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", rr.PIN_GRAPHS)
def test_pinned_kernels_give_the_unpinned_bits(case, graph):
    c = case(graph)
    plan = c.plan("default")
    assert plan.has_latency_schedule()
    winners = (("max", "ties"), ("min", "randn"))
    for F in rr.PIN_WIDTHS:
        base, base_sel = {}, {}
        for hop in (0, 1):
            for op in rr.OPS:
                for kind in rr.SWEEP_KINDS:
                    base[hop, op, kind] = _forward(c, plan, "default", hop, op, kind, F, "%s unpinned" % graph, remember=False)
            gi = c.select_inputs(hop)[0][:, :F].contiguous()
            for op, kind in winners:
                base_sel[hop, op, kind] = plan.gather_rows_select(hop, c.ptr, c.ind, gi, c.ref(hop, op, kind)[1][:, :F].contiguous())
        try:
            for mask in rr.PIN_MASKS:  # kind 0 falls back to the plan's schedule, kind 2 is the latency schedule, per hop
                plan.pin(F, "pull", mask)
                what = "%s pinned %d" % (graph, mask)
                for (hop, op, kind), (d0, a0) in base.items():
                    d, a = _forward(c, plan, "default", hop, op, kind, F, what, remember=False)
                    assert torch.equal(_bits(d), _bits(d0)) and torch.equal(a, a0), "%s hop %d %s %s F=%d" % (what, hop, op, kind, F)
                for (hop, op, kind), s0 in base_sel.items():
                    _select(c, plan, hop, op, kind, F, what)
                    s = plan.gather_rows_select(hop, c.ptr, c.ind, c.select_inputs(hop)[0][:, :F].contiguous(),
                                                c.ref(hop, op, kind)[1][:, :F].contiguous())
                    # integer gs: exact on either schedule, so the same bits (randn gs are summed in each schedule's order)
                    assert torch.equal(_bits(s), _bits(s0)), "%s select of hop %d (%s, %s) F=%d" % (what, hop, op, kind, F)
        finally:
            plan.unpin(F)


# ---- check 7: ops.reduce_aggr, all sixteen pairs ---------------------------------------------------------------------------

def _device_mean_hop(ops, c, X, degE, W):
    """Hop 0 of reduce_aggr(first='mean') as ops.reduce_aggr forms it: the sum scaled by the single factor degE * W / |e|,
    non-finite factors set to 0."""
    num = None
    for s in (degE, W):
        if s is not None:
            num = s if num is None else num * s
    s = (1.0 if num is None else num) / c.len[0].float()
    s = torch.where(torch.isfinite(s), s, torch.zeros_like(s))
    return ops.incidence_gather(c.ptr, c.ind, X, to="hyperedge", scale_a=s)


@pytest.mark.parametrize("second", rr.PAIR_REDUCES)
@pytest.mark.parametrize("first", rr.PAIR_REDUCES)
@pytest.mark.parametrize("graph", rr.PAIR_GRAPHS)
def test_reduce_aggr_pairs(case, graph, first, second):
    """Without a mean nothing rounds (test_reduce_schedules_host.test_pair_inputs_stay_exact_in_fp32): Y and dX equal float64.
    With one, FP32_C of the mass, the mass pass following the real pass's winners.  A comparison after a mean compares
    values that float32 has rounded, where two hyperedges whose means are equal as rationals may differ in the last bit: there
    the float64 pass is given the exact winners of the device's own float32 table (reduce_hop on it never rounds)."""
    from hypergef_amd import plan as planmod
    c = case(graph)
    ops, inc = c.hg.ops, c.inc
    exact = "mean" not in (first, second)
    planmod.set_default_opts(planmod.make_opts(row_stream=False, **ir.option_sets()["small"]))
    try:
        for F in rr.PAIR_WIDTHS:
            Xn, dYn = rr.pair_inputs(inc, F)
            X, dY = torch.from_numpy(Xn).to(DEV), torch.from_numpy(dYn).to(DEV)
            scales = tuple(torch.from_numpy(s).to(DEV) for s in ir.power_of_two_scales(inc))
            for degE, degV, W in (scales, (None, None, None)) if F == rr.PAIR_WIDTHS[-1] else (scales,):
                what = "%s reduce_aggr(%s, %s) F=%d scales %s" % (graph, first, second, F, degE is not None)
                x = X.clone().requires_grad_(True)
                Y = ops.reduce_aggr(c.ptr, c.ind, x, first, second, degE, degV, W)
                Y.backward(dY)
                win = ([], [])
                if first == "mean" and second in rr.OPS:
                    xe = _device_mean_hop(ops, c, X, degE, W)
                    val, arg = rr.reduce_hop(inc, 1, xe, second, c.E, c.V)
                    got = ops.incidence_gather(c.ptr, c.ind, xe, to="vertex", scale_a=degV, num_nodes=inc.N, reduce=second)
                    want = val if degV is None else val * degV.reshape(-1, 1)
                    assert torch.equal(_bits(Y.detach()), _bits(got)) and torch.equal(_bits(got), _bits(want.contiguous())), \
                        what + ": hop 1 is not the exact winner of the device's hop 0 table"
                    win[1].append(arg)
                d64 = tuple(None if s is None else s.double() for s in (degE, degV, W))
                x64 = X.double().requires_grad_(True)
                y64 = rr.reduce_aggr64(c, x64, first, second, d64[0], d64[1], d64[2], win)
                (gx,) = torch.autograd.grad(y64, x64, dY.double())
                if exact:
                    assert torch.equal(Y.detach().double(), y64.detach()), what + ": Y is not the float64 answer"
                    assert torch.equal(x.grad.double(), gx), what + ": dX is not the float64 answer"
                else:
                    xa = X.double().abs().requires_grad_(True)
                    ym = rr.reduce_aggr64(c, xa, first, second, d64[0], d64[1], d64[2], win)  # the same winners
                    (mx,) = torch.autograd.grad(ym, xa, dY.double().abs())
                    ir.within_on_device(Y.detach(), y64.detach(), ym.detach(), gr.FP32_C, what + " Y")
                    ir.within_on_device(x.grad, gx, mx, gr.FP32_C, what + " dX")
    finally:
        planmod.set_default_opts(None)
