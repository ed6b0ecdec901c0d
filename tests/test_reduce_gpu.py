"""Max / min / mean in the row gather and the select-gather backward on the device (hg_gather_rows_reduce_f32,
hg_gather_rows_select_f32, ops.incidence_gather(reduce=...), ops.reduce_aggr, models.HyperGsysUniSAGE).

Graphs.  `crafted`: one hyperedge of each length in LENS over 1100 vertices -- the panel / wave-task boundary (short_max = 32)
at 31 / 32 / 33 and the split boundary (split_len = 512) at 511 / 512 / 513 -- `craftedT` its transpose, so that the vertex
rows have those lengths in hop 1, and `dup`, crafted plus a hyperedge that lists vertex 5 twice.  Plans: the default one; the
same with the latency schedule pinned (has_latency_schedule(): rows above 8 entries become wave tasks); and
make_opts(short_max=4, split_len=8), under which the 1025 row is cut into 129 wave tasks -- more than add_fixups' fan of 32
(hg_schedule.cpp), so it is summed in two levels; test_the_small_split_plan_has_first_level_fixups reads that off the plan's
schedule (a fixup record whose fourth word, pad, is positive).  Widths: WIDTHS; 33 and 260 take column tiles.
Inputs: randn; values from {-1, -0.0, +0.0, 1}; randn with +-inf sprinkled in and one destination row whose entries are all
-inf.  NaN is unspecified and not tested.

1. arg equals the reference exactly; dst is (src[ind[arg]] * scaleA) * scaleB evaluated in float32 torch, bit for bit; empty
   rows are +0.0 / -1 under scaleA = inf; max and min alike.
2. The three plans give identical bits; two calls agree; a misaligned src (4-byte lanes) agrees; a captured replay equals the
   eager call after one warm call.
3. Select-gather: integer gradients and power-of-two scales equal the float64 reference exactly on all three plans; randn
   gradients stay within _grad_ref.FP32_C of the mass (the sum of the absolute values selected), the sum gather's bound; on
   tie-free input the reference itself equals float64 torch scatter_reduce autograd; a duplicate's gradient arrives once.
4. reduce='mean' equals reduce='sum' with scale_a = 1 / len, bit for bit.
5. reduce_aggr(first='max', second='sum') against hgnnaggr_max on graphs without an empty hyperedge (there the old operator
   writes -1e5 * degE and record 0, the new one 0 and -1): outputs bit for bit, indices_t[arg] == record, the new dX within
   the atomic class's bound (_grad_ref.any_order_c) of the float64 adjoint.  The two dX are compared on `regular`, where every
   vertex has four hyperedges: hgnnaggr_max's backward is the reference's rule, T[e] * degV[winner] with T = the hyperedge
   sums of the unscaled gradient, and equals the adjoint (degV applied to each member's gradient before the sum) only where
   degV is the same for the members of a hyperedge -- on the cora shape the two differ by that rule, not by rounding.
6. HyperGsysUniSAGE for (mean, sum), (max, mean), (sum, max) against a float64 restatement (_reduce_ref.hop64) whose max takes the
   winner-only gradient; the inputs are small integers, so Z = X W^T is exact in both precisions and the winners cannot
   differ by rounding.  A captured training step replays to the bits of the eager step.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402
import _grad_ref as gr  # noqa: E402
import _reduce_ref as rr  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV, _bits = ar.DEV, ar.bits
LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025)
WIDTHS = (1, 3, 4, 8, 32, 33, 64, 128, 260)
FMAX = max(WIDTHS)
OPS = ("max", "min")
KINDS = ("randn", "ties", "inf")
PLANS = ("default", "latency", "split")


def crafted(dup=False):
    rng = np.random.default_rng(7)
    N = 1100
    rows = [np.sort(rng.choice(N, size=n, replace=False)).astype(np.int32) for n in LENS]
    if dup:
        rows.append(np.array([5, 5, 9], np.int32))
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    return synth.Incidence(N, len(rows), ptr, np.concatenate(rows), name="crafted-dup" if dup else "crafted")


def _make(name):
    if name == "crafted":
        return crafted()
    if name == "craftedT":
        return ar.transpose(crafted())
    if name == "dup":
        return crafted(dup=True)
    if name == "random":
        return synth.random_incidence(3000, 2000, 6.0, empty_frac=0.1)
    if name == "powerlaw":
        return synth.powerlaw(50_000, 200_000)
    if name == "cora":
        return synth.cora_shape()
    if name == "regular":  # hyperedge e = {e, e + 1, e + 3, e + 7} mod N: every vertex lies in exactly four hyperedges
        N = 2048
        mem = np.sort((np.arange(N)[:, None] + np.array([0, 1, 3, 7])[None, :]) % N, axis=1)
        return synth.Incidence(N, N, np.arange(0, 4 * N + 1, 4, dtype=np.int32), mem.reshape(-1).astype(np.int32), name="regular")
    raise KeyError(name)


class _G:
    """One graph on the device with its plans, inputs (drawn once at FMAX columns; a call takes the first F) and the
    references, which are computed once per (hop, op, kind, F) and shared by the tests."""

    def __init__(self, hg, name):
        self.hg, self.name = hg, name
        self.inc = inc = _make(name)
        self.ptr = torch.from_numpy(inc.csrptr).to(DEV)
        self.ind = torch.from_numpy(inc.colind).to(DEV)
        self.E, self.V = rr.entries(inc, DEV)
        self.len = (torch.bincount(self.E, minlength=inc.M), torch.bincount(self.V, minlength=inc.N))
        self._plans, self._src, self._ref = {}, {}, {}
        rng = np.random.default_rng(3)
        # scaleA = 1 / len: inf on an empty row, which must not reach the result; scaleB in [0.5, 1.5)
        self.sA = tuple((1.0 / n.float()) for n in self.len)
        self.sB = tuple(torch.from_numpy(rng.random(n.numel()).astype(np.float32) + 0.5).to(DEV) for n in self.len)

    def plan(self, which, F):
        from hypergef_amd.plan import Plan, make_opts
        if which not in self._plans:
            opts = make_opts(short_max=4, split_len=8) if which == "split" else None
            self._plans[which] = Plan.from_tensors(self.inc.N, self.ptr, self.ind, opts)
        p = self._plans[which]
        if which == "latency":
            if not p.has_latency_schedule():
                return None
            p.pin(F, "pull", 8)  # kernel 2, the latency schedule, for both hops
        return p

    def nrows(self, hop):
        return (self.inc.M, self.inc.N) if hop == 0 else (self.inc.N, self.inc.M)  # (dst, src)

    def src(self, hop, kind, F):
        key = (hop, kind)
        if key not in self._src:
            nsrc = self.nrows(hop)[1]
            rng = np.random.default_rng(100 + 10 * hop + KINDS.index(kind))
            if kind == "ties":
                x = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), size=(nsrc, FMAX))
            else:
                x = rng.standard_normal((nsrc, FMAX)).astype(np.float32)
            if kind == "inf":
                u = rng.random(x.shape)
                x[u < 0.05] = np.inf
                x[u > 0.95] = -np.inf
                x[self.all_inf_members(hop)] = -np.inf
            self._src[key] = torch.from_numpy(x).to(DEV)
        return self._src[key][:, :F].contiguous()

    def all_inf_row(self, hop):
        """The first destination row of at least two entries: the 'inf' input makes all its entries -inf."""
        return int(torch.nonzero(self.len[hop] >= 2)[0])

    def all_inf_members(self, hop):
        rows, other = (self.E, self.V) if hop == 0 else (self.V, self.E)
        return other[rows == self.all_inf_row(hop)].cpu().numpy()

    def ref(self, hop, op, kind, F):
        key = (hop, op, kind, F)
        if key not in self._ref:
            self._ref[key] = rr.reduce_hop(self.inc, hop, self.src(hop, kind, F), op, self.E, self.V)
        return self._ref[key]


_GRAPHS = {}


@pytest.fixture
def graph(hg):
    def get(name):
        if name not in _GRAPHS:
            _GRAPHS[name] = _G(hg, name)
        return _GRAPHS[name]
    return get


def _eq(a, b):
    return torch.equal(_bits(a), _bits(b))


def _expected_dst(g, hop, src, arg):
    """(src[ind[arg]] * scaleA) * scaleB in float32 torch; +0.0 where arg = -1."""
    other = g.V if hop == 0 else g.E
    cols = torch.arange(src.shape[1], device=DEV).reshape(1, -1).expand_as(arg)
    val = src[other[arg.clamp(min=0).long()], cols]
    want = (val * g.sA[hop].reshape(-1, 1)) * g.sB[hop].reshape(-1, 1)
    return torch.where(arg < 0, torch.zeros_like(want), want)


def test_the_small_split_plan_has_first_level_fixups(graph):
    for name, hop in (("crafted", 0), ("craftedT", 1), ("dup", 0)):
        g = graph(name)
        fix = g.plan("split", 8).schedule(hop)["fixups"]
        assert (fix[:, 3] > 0).any(), (name, hop)  # pad > 0: a first-level fixup
        tasks = g.plan("split", 8).schedule(hop)["tasks"]
        assert (tasks[:, 3] >= 0).sum() > 32
        # and the default plan cuts the 513 and 1025 rows into partial slots with one final fixup each
        d = g.plan("default", 8).schedule(hop)
        assert len(d["fixups"]) == 2 and (d["fixups"][:, 3] == 0).all() and len(d["panels"]) > 0


# ---- 1 and 2: the forward ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("name", ["crafted", "craftedT", "dup"])
def test_forward_equals_the_reference_on_every_schedule(graph, name, F):
    g = graph(name)
    for hop in (0, 1):
        ndst = g.nrows(hop)[0]
        empty = g.len[hop] == 0
        for op in OPS:
            for kind in KINDS:
                src = g.src(hop, kind, F)
                ref_v, ref_a = g.ref(hop, op, kind, F)
                first = None
                for which in PLANS:
                    plan = g.plan(which, F)
                    if plan is None:
                        continue
                    what = "%s hop %d %s %s F=%d plan %s" % (name, hop, op, kind, F, which)
                    dst, arg = plan.gather_rows_reduce(hop, g.ptr, g.ind, src, op, g.sA[hop], g.sB[hop])
                    assert arg.dtype == torch.int32 and tuple(arg.shape) == (ndst, F) == tuple(dst.shape), what
                    assert torch.equal(arg, ref_a.to(torch.int32)), what
                    assert _eq(dst, _expected_dst(g, hop, src, arg)), what
                    if bool(empty.any()):
                        assert bool((arg[empty] == -1).all()) and not bool(_bits(dst[empty]).any()), what
                    if first is None:
                        first = (dst, arg)
                        dst2, arg2 = plan.gather_rows_reduce(hop, g.ptr, g.ind, src, op, g.sA[hop], g.sB[hop])
                        assert _eq(dst, dst2) and torch.equal(arg, arg2), "two calls: " + what
                    else:
                        assert _eq(dst, first[0]) and torch.equal(arg, first[1]), "schedules differ: " + what
                # without scales the value is the winner's bits
                if kind == "ties":
                    dst, arg = g.plan("default", F).gather_rows_reduce(hop, g.ptr, g.ind, src, op)
                    assert _eq(dst, ref_v) and torch.equal(arg, ref_a.to(torch.int32)), what
                if kind == "inf" and op == "max":  # the all -inf row: its first position wins
                    r = g.all_inf_row(hop)
                    rows = g.E if hop == 0 else g.V
                    assert int(first[1][r, 0]) == int(torch.nonzero(rows == r)[0]) and bool((first[1][r] == first[1][r, 0]).all())


@pytest.mark.parametrize("name", ["random", "powerlaw"])
def test_wider_shapes(graph, name):
    g, F = graph(name), 32
    plan = g.plan("default", F)
    for hop in (0, 1):
        for op in OPS:
            for kind in ("randn", "ties"):
                src = g.src(hop, kind, F)
                ref_v, ref_a = g.ref(hop, op, kind, F)
                dst, arg = plan.gather_rows_reduce(hop, g.ptr, g.ind, src, op, g.sA[hop], g.sB[hop])
                what = "%s hop %d %s %s" % (name, hop, op, kind)
                assert torch.equal(arg, ref_a.to(torch.int32)), what
                assert _eq(dst, _expected_dst(g, hop, src, arg)), what
        # the select-gather on integers: exact
        _, arg = g.ref(hop, "max", "ties", F)
        gs = torch.randint(-3, 4, arg.shape, device=DEV).float()
        got = plan.gather_rows_select(hop, g.ptr, g.ind, gs, arg.to(torch.int32))
        assert torch.equal(got.double(), rr.select_grad(g.inc, hop, gs.double(), arg, g.E, g.V)), "%s select hop %d" % (name, hop)


def test_misaligned_rows_take_the_narrow_lanes_and_give_the_same_bits(graph):
    g, F = graph("crafted"), 8
    plan = g.plan("default", F)
    for hop in (0, 1):
        src = g.src(hop, "randn", F)
        buf = torch.empty(src.numel() + 1, device=DEV)
        off = buf[1:].view_as(src).copy_(src)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        a = plan.gather_rows_reduce(hop, g.ptr, g.ind, src, "max", g.sA[hop], g.sB[hop])
        b = plan.gather_rows_reduce(hop, g.ptr, g.ind, off, "max", g.sA[hop], g.sB[hop])
        assert _eq(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("hop", [0, 1])
def test_captured_replay(graph, hop):
    g, F = graph("crafted" if hop == 0 else "craftedT"), 32
    plan = g.plan("default", F)
    src = g.src(hop, "randn", F).clone()
    ndst, nsrc = g.nrows(hop)
    dst, arg = torch.empty(ndst, F, device=DEV), torch.empty(ndst, F, dtype=torch.int32, device=DEV)
    gs, dsrc = torch.randn(ndst, F, device=DEV), torch.empty(nsrc, F, device=DEV)
    ws = torch.empty(plan.reduce_workspace_bytes(F), dtype=torch.uint8, device=DEV)

    def run():
        plan.gather_rows_reduce(hop, g.ptr, g.ind, src, "min", g.sA[hop], g.sB[hop], out=dst, arg_out=arg, workspace=ws)
        plan.gather_rows_select(hop, g.ptr, g.ind, gs, arg, out=dsrc, workspace=ws)

    run()  # the warm call: uploads the permutation
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        run()
    src.copy_(g.src(hop, "ties", F))
    run()
    want = (dst.clone(), arg.clone(), dsrc.clone())
    dst.fill_(7.0), arg.fill_(7), dsrc.fill_(7.0)
    graph_.replay()
    torch.cuda.synchronize()
    assert _eq(dst, want[0]) and torch.equal(arg, want[1]) and _eq(dsrc, want[2])
    assert torch.equal(arg, g.ref(hop, "min", "ties", F)[1].to(torch.int32))


# ---- 3: the select-gather ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("name", ["crafted", "craftedT", "dup"])
def test_select_gather(graph, name, F):
    g = graph(name)
    gen = torch.Generator(device=DEV).manual_seed(F)
    for hop in (0, 1):
        ndst, nsrc = g.nrows(hop)
        pow2 = torch.tensor([0.5, 1.0, 2.0, 4.0], device=DEV)[torch.randint(0, 4, (ndst,), device=DEV, generator=gen)]
        for op, kind in (("max", "ties"), ("min", "randn"), ("max", "inf")):
            _, arg64 = g.ref(hop, op, kind, F)
            arg = arg64.to(torch.int32)
            gi = torch.randint(-3, 4, (ndst, F), device=DEV, generator=gen).float()
            gs = gi * pow2.reshape(-1, 1)  # exact
            want = rr.select_grad(g.inc, hop, gs.double(), arg64, g.E, g.V)
            gn = torch.randn(ndst, F, device=DEV, generator=gen)
            want_n = rr.select_grad(g.inc, hop, gn.double(), arg64, g.E, g.V)
            mass_n = rr.select_grad(g.inc, hop, gn.double().abs(), arg64, g.E, g.V)
            first = None
            for which in PLANS:
                plan = g.plan(which, F)
                if plan is None:
                    continue
                what = "%s hop %d %s %s F=%d plan %s" % (name, hop, op, kind, F, which)
                got = plan.gather_rows_select(hop, g.ptr, g.ind, gs, arg)
                assert tuple(got.shape) == (nsrc, F) and torch.equal(got.double(), want), what
                got_n = plan.gather_rows_select(hop, g.ptr, g.ind, gn, arg)
                gr.assert_within(got_n, want_n.cpu(), mass_n.cpu(), gr.FP32_C, what)
                assert _eq(got_n, plan.gather_rows_select(hop, g.ptr, g.ind, gn, arg)), "two calls: " + what
        # tie-free input: the reference is torch's amax / amin autograd in float64
        src = g.src(hop, "randn", F).double().requires_grad_(True)
        rows, other = (g.E, g.V) if hop == 0 else (g.V, g.E)
        for op in OPS:
            vals = src[other]
            out = torch.zeros(ndst, F, dtype=torch.float64, device=DEV).scatter_reduce(
                0, rows.reshape(-1, 1).expand_as(vals), vals, "amax" if op == "max" else "amin", include_self=False)
            gn = torch.randn(ndst, F, device=DEV, generator=gen)
            (tg,) = torch.autograd.grad(out, src, gn.double())
            _, arg64 = g.ref(hop, op, "randn", F)
            ours = rr.select_grad(g.inc, hop, gn.double(), arg64, g.E, g.V)
            # both are float64 sums formed by atomics in no fixed order: equal up to float64 rounding
            assert torch.allclose(ours, tg, rtol=1e-12, atol=1e-12), "reference against torch autograd: %s hop %d %s" % (name, hop, op)


def test_autograd_and_the_duplicate(graph):
    """Through ops.incidence_gather: vertex 5 holds the largest value, so it wins every hyperedge that lists it -- the last
    one lists it twice -- and its gradient is the number of those hyperedges, not of their positions."""
    g, F = graph("dup"), 8
    ops = g.hg.ops
    x = torch.zeros(g.inc.N, F, device=DEV)
    x[5] = 10.0
    x.requires_grad_(True)
    dst, arg = ops.incidence_gather(g.ptr, g.ind, x, to="hyperedge", reduce="max", return_index=True)
    assert not arg.requires_grad and arg.dtype == torch.int32
    dst.backward(torch.ones_like(dst))
    holds5 = torch.unique(g.E[g.V == 5])
    assert bool((x.grad[5] == float(holds5.numel())).all())
    assert int((g.V == 5).sum()) == holds5.numel() + 1  # one position more than hyperedges
    last = g.inc.M - 1
    assert bool((arg[last] == int(g.inc.csrptr[last])).all())  # the first of the two positions
    _, ref_a = rr.reduce_hop(g.inc, 0, x.detach(), "max", g.E, g.V)
    want = rr.select_grad(g.inc, 0, torch.ones(g.inc.M, F, dtype=torch.float64, device=DEV), ref_a, g.E, g.V)
    assert torch.equal(x.grad.double(), want)
    # the scales reach the gradient; min, to the vertices
    xe = torch.randn(g.inc.M, F, device=DEV).requires_grad_(True)
    s = torch.full((g.inc.N,), 0.5, device=DEV)
    y = ops.incidence_gather(g.ptr, g.ind, xe, to="vertex", reduce="min", scale_a=s, num_nodes=g.inc.N)
    gy = torch.randint(-3, 4, y.shape, device=DEV).float()
    y.backward(gy)
    _, ref_a = rr.reduce_hop(g.inc, 1, xe.detach(), "min", g.E, g.V)
    assert torch.equal(xe.grad.double(), rr.select_grad(g.inc, 1, (gy * 0.5).double(), ref_a, g.E, g.V))


# ---- 4: the mean -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["crafted", "random"])
def test_mean_is_the_sum_scaled_by_the_reciprocal_length(graph, name):
    g, F = graph(name), 33
    ops = g.hg.ops
    for hop, to in enumerate(("hyperedge", "vertex")):
        src = g.src(hop, "randn", F)
        recip = torch.where(g.len[hop] > 0, 1.0 / g.len[hop].float(), torch.zeros(1, device=DEV))
        for s in (None, g.sB[hop]):
            mean = ops.incidence_gather(g.ptr, g.ind, src, to=to, scale_a=s, num_nodes=g.inc.N, reduce="mean")
            want = ops.incidence_gather(g.ptr, g.ind, src, to=to, scale_a=recip, scale_b=s, num_nodes=g.inc.N)
            assert _eq(mean, want), (name, to)
            assert not bool(_bits(mean[g.len[hop] == 0]).any())
        plan = g.hg.plan.cached_plan(g.inc.N, g.ptr, g.ind)
        assert _eq(plan.row_recip(hop, g.ptr), recip)


# ---- 5: against hgnnaggr_max ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cora", "regular"])
def test_against_hgnnaggr_max(graph, name):
    g, F = graph(name), 32
    hg, ops, inc = g.hg, g.hg.ops, g.inc
    assert int(g.len[0].min()) > 0  # no empty hyperedge: there the two operators differ by design
    h = hg.HyperGraph.from_incidence(inc, DEV, data_name=name, ngs=1 << 30)
    ptr, ind = h.H_T_csrptr, h.H_T_colind
    W = torch.ones(inc.M, 1, device=DEV)
    X = g.src(0, "randn", F)
    gy = torch.randn(inc.N, F, device=DEV)
    x_old = X.clone().requires_grad_(True)
    out_old, record = ops.hgnnaggr_max(ptr, ind, x_old, h.degE, h.degV, W)
    out_old.backward(gy)
    x_new = X.clone().requires_grad_(True)
    out_new = ops.reduce_aggr(ptr, ind, x_new, "max", "sum", h.degE, h.degV, W)
    out_new.backward(gy)
    assert _eq(out_new, out_old)
    _, arg = ops.incidence_gather(ptr, ind, X, to="hyperedge", reduce="max", scale_a=h.degE, scale_b=W, return_index=True)
    assert torch.equal(ind[arg.long()], record)
    # float64: dXe = (H^T (gy * degV)) * degE * W, then the select
    G = gr.Graph(inc, h.degE, h.degV, W)
    ge = G.v2e(gr.f64(gy) * G.degV.reshape(-1, 1)) * G.se.reshape(-1, 1)
    ge_mass = G.v2e(gr.f64(gy).abs() * G.degV.reshape(-1, 1)) * G.se.reshape(-1, 1)
    arg_cpu = arg.cpu().long()
    want = rr.select_grad(inc, 0, ge, arg_cpu)
    mass = rr.select_grad(inc, 0, ge_mass, arg_cpu)
    c = gr.any_order_c(inc)
    gr.assert_within(x_new.grad, want, mass, c, "select-gather dX")
    if name == "regular":
        gr.assert_within(x_old.grad, want, mass, c, "atomic dX")
        gr.assert_within(x_new.grad, gr.f64(x_old.grad), mass, 2 * c, "the two dX")


# ---- 6: the layer ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first,second", [("mean", "sum"), ("max", "mean"), ("sum", "max")])
def test_unisage(graph, first, second):
    g = graph("random")
    hg, inc = g.hg, g.inc
    h = hg.HyperGraph.from_incidence(inc, DEV, data_name="random", ngs=1 << 30)
    Fin, Fout = 8, 16
    rng = np.random.default_rng(9)
    X = torch.from_numpy(rng.integers(-3, 4, size=(inc.N, Fin)).astype(np.float32)).to(DEV)
    W0 = torch.from_numpy(rng.integers(-2, 3, size=(Fout, Fin)).astype(np.float32)).to(DEV)
    gy = torch.from_numpy(rng.integers(-2, 3, size=(inc.N, Fout)).astype(np.float32)).to(DEV)
    model = hg.HyperGsysUniSAGE(h, Fin, Fout, first, second).to(DEV)
    with torch.no_grad():
        model.W.weight.copy_(W0)
    x = X.clone().requires_grad_(True)
    y = model(x)
    y.backward(gy)

    win = ([], [])  # the winners of hop 0 and hop 1, filled by the real pass and followed by the mass pass

    def f64_layer(x64, w64):
        z = x64 @ w64.t()
        return z + rr.hop64(g, 1, rr.hop64(g, 0, z, first, win[0]), second, win[1])

    x64, w64 = X.double().requires_grad_(True), W0.double().requires_grad_(True)
    y64 = f64_layer(x64, w64)
    gx, gw = torch.autograd.grad(y64, (x64, w64), gy.double())
    # the masses: the same layer, same winners, on absolute values
    xa, wa = X.double().abs().requires_grad_(True), W0.double().abs().requires_grad_(True)
    ym = f64_layer(xa, wa)
    mx, mw = torch.autograd.grad(ym, (xa, wa), gy.double().abs())
    what = "UniSAGE(%s, %s)" % (first, second)
    gr.assert_within(y, y64.detach().cpu(), ym.detach().cpu(), gr.FP32_C, what + " forward")
    gr.assert_within(model.W.weight.grad, gw.cpu(), mw.cpu(), gr.FP32_C, what + " dW")
    gr.assert_within(x.grad, gx.cpu(), mx.cpu(), gr.FP32_C, what + " dX")

    # A captured training step replays to the eager step's bits.  The layer is a fresh one whose every backward runs on
    # the side stream (test_scale_grads_gpu._step_and_capture: a gradient accumulator made by a backward on the default
    # stream, whose graph is still alive -- y above -- would draw that stream into the capture).
    from hypergef_amd import plan as planmod
    del y, x
    layer = hg.HyperGsysUniSAGE(h, Fin, Fout, first, second).to(DEV)
    opt = torch.optim.SGD(layer.parameters(), lr=2.0 ** -10)

    def restore():
        with torch.no_grad():
            layer.W.weight.copy_(W0)

    def train_step():
        opt.zero_grad(set_to_none=True)
        (layer(X) * gy).sum().backward()
        opt.step()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        restore()
        train_step()  # warm: everything a first call allocates or uploads
        restore()
        train_step()  # the eager step
        eager = layer.W.weight.detach().clone()
        restore()
        opt.zero_grad(set_to_none=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert not torch.equal(eager, W0)
    planmod.clear_pack_cache()  # cached packings are keyed on version counters a replay does not advance
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        train_step()
    planmod.clear_pack_cache()
    restore()
    graph_.replay()
    torch.cuda.synchronize()
    assert _eq(layer.W.weight.detach(), eager), what + ": the captured step differs from the eager step"
    planmod.clear_pack_cache()
