"""The linear layer on bf16 rows with its linear on the bf16 MFMA (-m gpu): Plan.aggregate_linear_bf16 /
hg_aggr_linear_res_bf16, the rows kernel, the weight packing, and the operator layer under Options(linear_bf16="mfma").

The contract (include/hg_aggr.h): T_out is the fp32 entry's combined row on the widened operands rounded to bf16 once,
bit for bit; Y = round_bf16(act(T_out . Wb^T)) with exact products and fp32 accumulation.  The bound on Y follows from
that, not from a run:  |Y - yref| <= 2^-8 (|yref| + e) + e  with yref = act(T_out . Wb^T) in float64 and
e = 2 F_in 2^-24 (|T_out| . |Wb|^T)  -- fp32 accumulation of F_in exact products (F_in 2^-24 of their absolute sum in
any order), doubled for the matrix pipe's internal grouping, then one bf16 rounding (unit roundoff 2^-8) of a value
within e of yref.  relu is monotone and 1-Lipschitz: it does not widen the bound."""
import ctypes

import numpy as np
import pytest
import torch

import _grad_ref as gr
from hypergef_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
VARIANTS = ("auto", "fused", "pull")
F_INS = (32, 64, 128)
F_OUTS = (16, 64, 80, 128)  # 80: five column tiles, the clamped tile of the panels' two-tiles-per-wave form
GUARD = 128  # elements: 256 bytes of bf16, so the guarded view keeps its alignment
TILE = 16384  # fused_tile_bytes: 32 slots and rows per panel at F = 128, whatever the graph's size


def _edited(inc, lone, big, hub_deg):
    """`inc` with vertex `lone` taken out of every hyperedge, one hyperedge of `big` members appended and vertex 0 put
    into the first `hub_deg` hyperedges (0: left alone)."""
    edges = [set(inc.colind[inc.csrptr[e]:inc.csrptr[e + 1]].tolist()) - {lone} for e in range(inc.M)]
    edges.append(set(range(1, 1 + big)) - {lone})
    for e in range(hub_deg):
        edges[e].add(0)
    sizes = np.array([len(s) for s in edges], np.int64)
    ptr = np.zeros(len(edges) + 1, np.int64)
    np.cumsum(sizes, out=ptr[1:])
    ind = np.concatenate([np.sort(np.fromiter(s, np.int32, len(s))) for s in edges]) if ptr[-1] else np.zeros(0, np.int32)
    return synth.Incidence(inc.N, len(edges), ptr.astype(np.int32), ind.astype(np.int32), "edited")


GRAPHS = {
    # whole vertices only: every row of an F_in = 128 fused call is multiplied inside its panel
    "panels": lambda: _edited(synth.random_incidence(300, 220, 4.0, seed=5, max_size=8, empty_frac=0.1), 299, 40, 0),
    # vertex 0 in 70 hyperedges, more than a panel's 32 slots at F = 128: cut into pieces, summed by the fixup pass
    "split": lambda: _edited(synth.random_incidence(300, 220, 4.0, seed=6, max_size=8, empty_frac=0.1), 299, 40, 70),
}


def _bits(t):
    return t.contiguous().view(torch.int16)


def _guarded(*shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV, dtype=BF)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _fused_shape(plan, F):
    """hg_debug_fused_shape: (panels, rows, rows padded to 16-row tiles, ..., cap, rows_cap, n_mat, ...)."""
    from hypergef_amd import _lib
    fn = _lib.lib().hg_debug_fused_shape
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    out = np.zeros(9, np.int64)
    _lib.check(fn(plan._h, F, 0, out.ctypes.data_as(ctypes.c_void_p)))
    return out


class _Case:
    """One graph on the device: plan, scales, inputs drawn once at the widest widths and never modified."""

    def __init__(self, name):
        from hypergef_amd import plan as planmod
        self.name, self.inc = name, GRAPHS[name]()
        inc = self.inc
        self.ptr, self.ind = torch.from_numpy(inc.csrptr).to(DEV), torch.from_numpy(inc.colind).to(DEV)
        self.plan = planmod.Plan.from_tensors(inc.N, self.ptr, self.ind, planmod.make_opts(fused_tile_bytes=TILE))
        rng = np.random.default_rng(17)
        dev = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV, dt)  # noqa: E731
        self.X = dev(rng.standard_normal((inc.N, 128)), BF)
        self.R = dev(rng.standard_normal((inc.N, 128)), BF)
        self.Wl = dev(rng.standard_normal((128, 128)) / 8, BF)
        self.scales = tuple(dev(rng.random(n) + 0.5) for n in (inc.M, inc.N, inc.M))  # degE, degV, W
        self.info = {F: self.plan.prepare(F) for F in F_INS}
        self.shape128 = _fused_shape(self.plan, 128)


@pytest.fixture(scope="module")
def case(hg):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Case(name)
        return cache[name]
    return get


def test_the_graphs_hold_what_the_cases_need(hg, case):
    """Panels of at most 16 and of 17 .. 32 rows, an empty hyperedge, a vertex in no hyperedge, and (graph 'split') hyperedges
    the pre-pass materialises and a split vertex, which puts both kernels to work at F_in = 128."""
    for name in GRAPHS:
        cs = case(name)
        inc = cs.inc
        sizes = np.diff(inc.csrptr)
        deg = np.bincount(inc.colind, minlength=inc.N)
        assert (sizes == 0).any() and (deg == 0).any() and inc.N <= 400
        info = cs.info[128]
        assert sizes.max() > info["t_big"], info
        if name == "split":  # (the launch-bound 'panels' graph cuts its long hyperedge into sub-slots instead)
            assert info["n_mat"] >= 1, info
        panels, rows, padded = (int(v) for v in cs.shape128[:3])
        assert 0 < int(cs.shape128[6]) <= 32  # rows_cap: a panel is one or two 16-row tiles
        n32, n16 = padded // 16 - panels, 2 * panels - padded // 16
        assert n16 >= 1 and n32 >= 1, (panels, rows, padded)
        split = info["n_split"] + info["n_hub"]
        assert (split > 0) == (name == "split"), info
        for F_out in F_OUTS:
            assert cs.plan.linear_bf16_path(128, F_out, "fused") == (3 if name == "split" else 1)
            assert cs.plan.linear_bf16_path(128, F_out, "pull") == 2
            for F_in in (32, 64):
                assert cs.plan.linear_bf16_path(F_in, F_out, "fused") == 2
        assert cs.plan.linear_bf16_path(128, 256, "fused") == 2  # wider than the panels' staged matrix phase


# with / without scales, residual, ca != 1, relu, T_out, cb on the device
COMBOS = [
    dict(),
    dict(scales=True, t_out=True),
    dict(res=True, ca=0.75, cb=0.5, relu=True, t_out=True),
    dict(scales=True, res=True, ca=1.0, cb=1.25, cb_dev=True, t_out=True),
    dict(scales=True, ca=-0.5, relu=True, t_out=True),
    dict(res=True, ca=0.9, cb=0.1, relu=True),
]


def _y_bound(Y, T, Wl, relu, F_in, what):
    t, w = T.double(), Wl.double()
    yref = t @ w.t()
    if relu:
        yref = torch.relu(yref)
    e = 2 * F_in * 2.0 ** -24 * (t.abs() @ w.abs().t())
    err = (Y.double() - yref).abs()
    bad = ~(err <= 2.0 ** -8 * (yref.abs() + e) + e)  # every element; a NaN is outside
    assert not bool(bad.any()), "%s: %d of %d elements of Y outside the bound, max err %g" % (
        what, int(bad.sum()), bad.numel(), float(err.max()))


@pytest.mark.parametrize("F_in", F_INS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_contract(hg, case, name, F_in):
    from hypergef_amd import plan as planmod
    cs = case(name)
    plan, N = cs.plan, cs.inc.N
    X, R = cs.X[:, :F_in].contiguous(), cs.R[:, :F_in].contiguous()
    X32, R32 = X.float(), R.float()
    ws = torch.empty(max(plan.linear_workspace_bytes(F_in), 256) + 256, dtype=torch.uint8, device=DEV)
    n_cases = 0
    for F_out in F_OUTS:
        Wl = cs.Wl[:F_out, :F_in].contiguous()
        packed = planmod.pack_linear_bf16(Wl)
        assert packed.numel() * 2 == 2 * F_out * F_in
        for variant in VARIANTS:
            path = plan.linear_bf16_path(F_in, F_out, variant)
            if F_in == 128 and variant == "fused":
                assert path & 1, "the in-panel epilogue must run at F_in = 128 on the fused variant"
                assert bool(path & 2) == (name == "split")
            for combo in COMBOS:
                what = "%s %d->%d %s %s" % (name, F_in, F_out, variant, combo)
                degE, degV, W = cs.scales if combo.get("scales") else (None, None, None)
                res = R if combo.get("res") else None
                ca, cbv, relu = combo.get("ca", 1.0), combo.get("cb", 0.0), combo.get("relu", False)
                cb = torch.tensor([cbv], device=DEV) if combo.get("cb_dev") else cbv
                kw = dict(degE=degE, degV=degV, W=W, variant=variant, ca=ca, cb=cb, relu=relu)
                T = torch.empty(N, F_in, dtype=BF, device=DEV) if combo.get("t_out") else None
                Y = plan.aggregate_linear_bf16(cs.ptr, cs.ind, X, Wl, residual=res, t_out=T, **kw)
                assert Y.dtype == BF and tuple(Y.shape) == (N, F_out)
                # 1. T_out: the fp32 entry's combined row, rounded once
                T32 = torch.empty(N, F_in, device=DEV)
                plan.aggregate_linear(cs.ptr, cs.ind, X32, Wl.float(), residual=None if res is None else R32, t_out=T32, **kw)
                want_T = T32.to(BF)
                if T is not None:
                    same = _bits(T) == _bits(want_T)
                    assert bool(same.all()), "%s: T_out differs from the rounded fp32 row at %d elements" % (what, int((~same).sum()))
                # 2. Y against the float64 product of the call's own T_out (the rounded fp32 row where none was asked for)
                Tc = T if T is not None else want_T
                _y_bound(Y, Tc, Wl, relu, F_in, what)
                # 3 + 4. the same bits again, with the caller's workspace, packing and guarded outputs; guards untouched
                ybuf, Yg = _guarded(N, F_out)
                tbuf, Tg = _guarded(N, F_in)
                Y2 = plan.aggregate_linear_bf16(cs.ptr, cs.ind, X, Wl, residual=res, t_out=Tg if T is not None else None,
                                                out=Yg, workspace=ws, packed=packed, **kw)
                assert Y2 is Yg and torch.equal(_bits(Y), _bits(Yg)), "%s: a second call gives other bits" % what
                if T is not None:
                    assert torch.equal(_bits(T), _bits(Tg)), "%s: T_out of a second call differs" % what
                else:
                    assert bool(torch.isnan(tbuf).all())
                assert _guards_intact(ybuf) and _guards_intact(tbuf), "%s: a guard band was written" % what
                # 5. the rows kernel on the same rows
                if combo.get("t_out") and variant == "fused":
                    Yr = planmod.linear_rows_bf16(Tc, Wl, packed=packed)
                    _y_bound(Yr, Tc, Wl, False, F_in, what + " rows kernel")
                n_cases += 1
    assert n_cases == len(F_OUTS) * len(VARIANTS) * len(COMBOS)


def test_isolated_vertex_gives_plus_zero(hg, case):
    cs = case("panels")
    lone = int(np.flatnonzero(np.bincount(cs.inc.colind, minlength=cs.inc.N) == 0)[0])
    for F_in in F_INS:
        for variant in ("fused", "pull"):
            Y = cs.plan.aggregate_linear_bf16(cs.ptr, cs.ind, cs.X[:, :F_in].contiguous(), cs.Wl[:64, :F_in].contiguous(),
                                              variant=variant)
            assert bool((_bits(Y[lone]) == 0).all()), (F_in, variant)


def test_rows_kernel_guards_and_ragged_row_counts(hg, case):
    """hg_linear_rows_bf16 at row counts around its 16-row wave tiles and 64-row workgroups, F_out below and above F_in."""
    from hypergef_amd import plan as planmod
    cs = case("panels")
    for F_in in F_INS:
        for F_out in (16, 80, 256):
            Wl = (torch.randn(F_out, F_in, device=DEV, generator=torch.Generator(device=DEV).manual_seed(F_out)) / 8).to(BF)
            for rows in (1, 15, 17, 64, 65, 300):
                T = cs.X[:rows, :F_in].contiguous()
                ybuf, Yg = _guarded(rows, F_out)
                Y = planmod.linear_rows_bf16(T, Wl, out=Yg)
                _y_bound(Y, T, Wl, False, F_in, "rows %d %d->%d" % (rows, F_in, F_out))
                assert _guards_intact(ybuf)


# ---- operator level -------------------------------------------------------------------------------------------------

def _opts(hg, **kw):
    return hg.ops.Options(linear_bf16="mfma", fuse_linear="always", **kw)


@pytest.fixture(scope="module")
def op_case(hg):
    inc = GRAPHS["split"]()
    hyperg = hg.HyperGraph.from_incidence(inc, DEV, data_name="bf16-linear")
    return inc, hyperg, gr.Graph(inc, hyperg.degE, hyperg.degV, None)


def _randn(*shape, seed, dtype=BF):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV, dtype)


@pytest.mark.parametrize("F_in,F_out", [(32, 48), (64, 64), (128, 128), (128, 64)])
def test_hgnnaggr_linear_operator(hg, op_case, F_in, F_out):
    """Forward: bf16 out, within the sum of both forms' bounds of the torch form (each against float64: the torch form
    rounds the GEMM and the aggregation, 2; the mfma form the combined row and the result, 2).  Gradients: the two-step
    backward on the bf16 paths, at the bound test_gradients.py has for it (2 roundings, 3 under the adjoint rule)."""
    inc, hyperg, graph = op_case
    x, wl, G = _randn(inc.N, F_in, seed=1), (_randn(F_out, F_in, seed=2, dtype=torch.float32) / F_in ** 0.5).to(BF), _randn(inc.N, F_out, seed=3)
    args = (hyperg.H_T_csrptr, hyperg.H_T_colind)
    for rule in ("reference", "adjoint"):
        for variant in ("auto", "fused", "pull"):
            xg, wg = x.clone().requires_grad_(True), wl.clone().requires_grad_(True)
            y = hg.ops.hgnnaggr_linear(*args, xg, wg, hyperg.degE, hyperg.degV, None, options=_opts(hg, backward=rule, variant=variant))
            gx, gw = torch.autograd.grad(y, (xg, wg), G)
            assert y.dtype == gx.dtype == gw.dtype == BF
            ref = gr.evaluate(lambda g, x, w: gr.hgnnaggr_linear(g, x, w, rule), graph, {"x": x, "w": wl}, G, ["x", "w"])
            what = "mfma hgnnaggr_linear %dx%d %s %s" % (F_in, F_out, rule, variant)
            gr.assert_within(y, ref[0], ref[2], gr.bf16_c(2), what + " out")
            c = gr.bf16_c(2 if rule == "reference" else 3)
            gr.assert_within(gx, ref[1]["x"], ref[3]["x"], c, what + " dx")
            gr.assert_within(gw, ref[1]["w"], ref[3]["w"], c, what + " dw")
            yt = hg.ops.hgnnaggr_linear(*args, x, wl, hyperg.degE, hyperg.degV, None,
                                        options=hg.ops.Options(fuse_linear="always", variant=variant))
            gr.assert_within(y, yt, ref[2], gr.bf16_c(2) + gr.bf16_c(2), what + " against the torch form")


@pytest.mark.parametrize("F", [64, 128])
def test_aggr_res_linear_operator(hg, op_case, F):
    """act((ca Aggr(X) + cb R) M^T): forward 2 roundings on the mfma form (combined row, result) against the torch form's 5;
    gradients for X, M, R and a tensor cb at test_gradients.py's bound for the bf16 backward (5)."""
    inc, hyperg, graph = op_case
    x, m = _randn(inc.N, F, seed=21), (_randn(F, F, seed=22, dtype=torch.float32) / 8).to(BF)
    res, G = _randn(inc.N, F, seed=23), _randn(inc.N, F, seed=24)
    args = (hyperg.H_T_csrptr, hyperg.H_T_colind)
    for ca, cbv, relu, cb_tensor in ((0.9, 0.25, True, False), (1.0, 1.25, False, True), (-0.5, 0.25, True, True)):
        for rule in ("reference", "adjoint"):
            t = {"x": x.clone().requires_grad_(True), "m": m.clone().requires_grad_(True), "r": res.clone().requires_grad_(True)}
            names = ["x", "m", "r"]
            if cb_tensor:
                t["cb"] = torch.tensor(cbv, device=DEV, dtype=BF).requires_grad_(True)
                names.append("cb")
            cbq = float(torch.tensor(cbv, dtype=BF)) if cb_tensor else cbv  # what the layer's bf16 parameter holds
            y = hg.ops.aggr_res_linear(*args, t["x"], t["m"], residual=t["r"], ca=ca, cb=t.get("cb", cbv), degE=hyperg.degE,
                                       degV=hyperg.degV, relu=relu, options=_opts(hg, backward=rule))
            assert y.dtype == BF
            got = dict(zip(names, torch.autograd.grad(y, [t[n] for n in names], G)))
            mask = (y.detach() > 0).cpu() if relu else None
            fn = lambda g, x, m, r, ca, cb, mask: gr.aggr_res_linear(g, x, m, rule, residual=r, ca=ca, cb=cb, mask=mask)  # noqa: E731
            inputs = {"x": x, "m": m, "r": res, "ca": ca, "cb": torch.tensor(cbq, dtype=torch.float64) if cb_tensor else cbv, "mask": mask}
            ref = gr.evaluate(fn, graph, inputs, G, names)
            what = "mfma aggr_res_linear F=%d ca=%g %s" % (F, ca, rule)
            gr.assert_within(y, ref[0], ref[2], gr.bf16_c(2), what + " out")
            for n in names:
                gr.assert_within(got[n], ref[1][n], ref[3][n], gr.bf16_c(5), "%s d%s" % (what, n))
            with torch.no_grad():
                yt = hg.ops.aggr_res_linear(*args, x, m, residual=res, ca=ca, cb=cbq, degE=hyperg.degE, degV=hyperg.degV,
                                            relu=False, options=hg.ops.Options(fuse_linear="always", backward=rule))
                ym = hg.ops.aggr_res_linear(*args, x, m, residual=res, ca=ca, cb=cbq, degE=hyperg.degE, degV=hyperg.degV,
                                            relu=False, options=_opts(hg, backward=rule))
            pre = gr.evaluate(fn, graph, dict(inputs, mask=None), G, [])
            gr.assert_within(ym, yt, pre[2], gr.bf16_c(2) + gr.bf16_c(5), what + " against the torch form")


def test_default_options_keep_the_torch_form_bit_for_bit(hg, op_case):
    """linear_bf16 = 'torch' (the default): every output of both operators on bf16 input is what it was before the option
    existed -- torch's GEMM around the bf16 aggregation, written out here."""
    from hypergef_amd.plan import cached_plan
    inc, hyperg, _ = op_case
    ptr, ind = hyperg.H_T_csrptr, hyperg.H_T_colind
    degE, degV = hyperg.degE.reshape(-1), hyperg.degV.reshape(-1)
    plan = cached_plan(inc.N, ptr, ind)
    assert hg.ops.Options().linear_bf16 == "torch" and hg.ops.current_options().linear_bf16 == "torch"
    for F_in, F_out in ((32, 32), (64, 16), (128, 128)):
        x, wl, res = _randn(inc.N, F_in, seed=31), (_randn(F_out, F_in, seed=32, dtype=torch.float32) / 8).to(BF), _randn(inc.N, F_in, seed=33)
        for mode in ("auto", "always", "never"):
            opt = hg.ops.Options(fuse_linear=mode)
            y = hg.ops.hgnnaggr_linear(ptr, ind, x, wl, degE, degV, None, options=opt)
            want = plan.aggregate(ptr, ind, torch.nn.functional.linear(x, wl).contiguous(), degE, degV, None)
            assert y.dtype == BF and torch.equal(_bits(y), _bits(want)), (F_in, F_out, mode)
            for relu in (False, True):
                y = hg.ops.aggr_res_linear(ptr, ind, x, wl, residual=res, ca=0.75, cb=0.5, degE=degE, degV=degV, relu=relu, options=opt)
                T = plan.aggregate(ptr, ind, x, degE, degV, None) * 0.75
                T = T + res * 0.5
                want = T @ wl.t()
                if relu:
                    want = torch.relu(want)
                assert y.dtype == BF and torch.equal(_bits(y), _bits(want)), (F_in, F_out, mode, relu)


class _Args:
    pass


@pytest.mark.parametrize("model", ["HGNN", "UniGCNII"])
def test_bf16_models_train_and_replay_as_a_graph(hg, model):
    """HGsysHGNN and UniGCNII in bf16 under linear_bf16 = 'mfma': a training step runs, and replays as a hipGraph after
    one warm call (the capture pattern of the other suites: side stream, warm-up, capture, replay)."""
    from hypergef_amd import models, plan as planmod
    inc = GRAPHS["split"]()
    hyperg = hg.HyperGraph.from_incidence(inc, DEV, data_name="bf16-linear-model")
    args = _Args()
    args.model, args.backend, args.nlayer, args.nhid, args.dropout = model, "hgsys", 2, 64, 0.0
    args.first_aggr, args.options, args.activation, args.input_drop = "sum", _opts(hg), "relu", 0.0
    torch.manual_seed(0)
    net = _build_model(models, args, hyperg, nfeat=32, nclass=16).to(DEV).to(BF)
    X = _randn(inc.N, 32, seed=41)
    target = torch.randint(0, 16, (inc.N,), generator=torch.Generator().manual_seed(42)).to(DEV)
    opt = torch.optim.SGD(net.parameters(), lr=1e-2)
    calls = []
    real = planmod.Plan.aggregate_linear_bf16

    def spy(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)
    planmod.Plan.aggregate_linear_bf16 = spy
    try:
        def step():
            opt.zero_grad(set_to_none=False)
            out = net(X)
            loss = torch.nn.functional.nll_loss(out.float(), target)
            loss.backward()
            opt.step()
            return loss

        loss0 = float(step())  # the warm call: plans, packings, bindings, torch's own lazy state
        assert calls and np.isfinite(loss0)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            planmod.clear_pack_cache()
            step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        planmod.clear_pack_cache()
        with torch.cuda.graph(graph):
            loss = step()
        losses = []
        for _ in range(3):
            graph.replay()
            losses.append(float(loss))
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in losses) and losses[-1] < loss0, (loss0, losses)
    finally:
        planmod.Plan.aggregate_linear_bf16 = real
        planmod.clear_pack_cache()


def _build_model(models, args, hyperg, nfeat, nclass):
    if args.model == "HGNN":
        return models.HGsysHGNN(args, hyperg, nfeat, args.nhid, nclass, args.nlayer, args.first_aggr, 1)
    return models.UniGCNII(args, hyperg, nfeat, args.nhid, nclass, args.nlayer, 1)
