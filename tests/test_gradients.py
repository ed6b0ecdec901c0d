"""Every operator's gradients against the float64 reference (tests/_grad_ref.py), under both backward rules.

Each case runs the library's forward and backward on the GPU, then the same formula in float64 on the CPU through
torch.autograd with the reference's "reference" / "adjoint" rule, and checks every output and input gradient at
|got - ref| <= c * max(mass, TINY) per element (c: _grad_ref.FP32_C, or bf16_c(k) for k bf16 roundings on the path).
Nothing here compares the library with itself.  Gradients of degE / degV / W are None by design and not checked.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _grad_ref as gr  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RULES = ("reference", "adjoint")
BIG_ROWS = 4096  # ops._rows_times / ops._wgrad run the library's kernels from this many rows on

SHAPES = {
    "cora": synth.cora_shape,                                                             # N = 2708: torch GEMMs
    "pubmed": synth.pubmed_shape,                                                         # N = 19717: library GEMMs
    "ragged": lambda: synth.random_incidence(700, 450, 7.0, seed=3, empty_frac=0.1),       # empty edges, lone vertices
    "powerlaw": lambda: synth.powerlaw(20000, 60000, seed=3, max_size=4096),              # hub vertices: hub pass
    "n4096": lambda: synth.random_incidence(BIG_ROWS, 2500, 4.0, seed=11, empty_frac=0.02),  # the switch itself
}


class _Case:
    """One shape on the device (HyperGraph, a random W) and its float64 graphs, built once per module."""

    def __init__(self, hg, name):
        self.inc = inc = SHAPES[name]()
        self.hyperg = hg.HyperGraph.from_incidence(inc, DEV, data_name=name)
        self.W = torch.from_numpy((np.random.default_rng(7).random(inc.M) + 0.5).astype(np.float32)).to(DEV)
        h = self.hyperg
        self.scales = {"all": (h.degE, h.degV, self.W), "deg": (h.degE, h.degV, None), "none": (None, None, None)}
        self._graphs = {}

    def graph(self, kind):
        if kind not in self._graphs:
            self._graphs[kind] = gr.Graph(self.inc, *self.scales[kind])
        return self._graphs[kind]


@pytest.fixture(scope="module")
def case(hg):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Case(hg, name)
        return cache[name]
    return get


def _randn(*shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV, dtype)


class _PathCounter:
    """Counts the calls of the names ops imported, ops.linear_rows / ops.linear_wgrad, and records the operand widths
    (the way test_bf16_autograd counts the fp32 aggregation): which backward GEMMs ran is asserted, not assumed."""

    def __init__(self, monkeypatch):
        from hypergef_amd import ops
        self.rows, self.wgrad = [], []
        real_rows, real_wgrad = ops.linear_rows, ops.linear_wgrad

        def rows(X, weight, *a, **k):
            self.rows.append((X.shape[0], tuple(weight.shape)))
            return real_rows(X, weight, *a, **k)

        def wgrad(A, B):
            self.wgrad.append((A.shape[0], A.shape[1], B.shape[1]))
            return real_wgrad(A, B)
        monkeypatch.setattr(ops, "linear_rows", rows)
        monkeypatch.setattr(ops, "linear_wgrad", wgrad)

    def reset(self):
        self.rows.clear()
        self.wgrad.clear()


def _check(what, got_out, out, out_mass, got_grads, grads, grad_mass, c_out, c_grad):
    gr.assert_within(got_out, out, out_mass, c_out, what + " out")
    for k in grads:
        gr.assert_within(got_grads[k], grads[k], grad_mass[k], c_grad, "%s d%s" % (what, k))


# ---- the sum family: hgnnaggr, unignnaggrdeg, unignnaggr ------------------------------------------------------------

SUM_OPS = {"hgnnaggr": "all", "unignnaggrdeg": "deg", "unignnaggr": "none"}
VARIANTS = ("auto", "pull", "fused", "push_atomic", "push_groups")
ANY_ORDER = ("push_atomic", "push_groups")  # fp32 atomics: gr.any_order_c
WIDTHS = (1, 3, 32, 100, 128)


def _sum_op(hg, name, cs, x, opt):
    h = cs.hyperg
    sched = (h.group_key, h.group_row, h.group_start, h.group_end, h.H_T_csrptr, h.H_T_colind, x)
    degE, degV, W = cs.scales[SUM_OPS[name]]
    if name == "hgnnaggr":
        return hg.ops.hgnnaggr(*sched, degE, degV, W, options=opt)
    if name == "unignnaggrdeg":
        return hg.ops.unignnaggrdeg(*sched, degE, degV, options=opt)
    return hg.ops.unignnaggr(*sched, options=opt)


@pytest.mark.parametrize("shape", ["cora", "pubmed", "ragged", "powerlaw"])
@pytest.mark.parametrize("op", list(SUM_OPS))
def test_sum_family_gradients(hg, case, shape, op):
    """Every variant (the push kernels' fp32 atomics add in any order: gr.any_order_c on their rows), a width
    from {1, 3, 32, 100, 128} per variant that rotates with the shape and operator so that every variant meets every
    width across the parametrisation, both backward rules."""
    cs = case(shape)
    graph = cs.graph(SUM_OPS[op])
    shift = list(SHAPES).index(shape) + list(SUM_OPS).index(op)
    c_any = gr.any_order_c(cs.inc)
    for i, variant in enumerate(VARIANTS):
        F = WIDTHS[(i + shift) % len(WIDTHS)]
        c = c_any if variant in ANY_ORDER else gr.FP32_C
        x = _randn(cs.inc.N, F, seed=i)
        G = _randn(cs.inc.N, F, seed=100 + i)
        for rule in RULES:
            xg = x.clone().requires_grad_(True)
            y = _sum_op(hg, op, cs, xg, hg.ops.Options(variant=variant, backward=rule))
            gx, = torch.autograd.grad(y, xg, G)
            ref = gr.evaluate(lambda g, x: gr.sum_aggr(g, x, rule), graph, {"x": x}, G, ["x"])
            _check("%s %s F=%d %s %s" % (op, shape, F, variant, rule), y, ref[0], ref[2], {"x": gx}, ref[1], ref[3],
                   c, c)


@pytest.mark.parametrize("shape", ["cora", "ragged", "powerlaw"])
def test_sum_family_bf16_gradients(hg, case, shape):
    """bf16 features on auto / fused / pull.  The kernel accumulates in fp32 and rounds the output once: one bf16
    rounding for the output and the reference-rule gradient; the adjoint rule first rounds grad * degV to bf16
    (ops._times_degV): two."""
    cs = case(shape)
    for j, op in enumerate(SUM_OPS):
        graph = cs.graph(SUM_OPS[op])
        for i, variant in enumerate(("auto", "fused", "pull")):
            F = (3, 32, 100)[(i + j) % 3]
            x = _randn(cs.inc.N, F, seed=i, dtype=torch.bfloat16)
            G = _randn(cs.inc.N, F, seed=50 + i, dtype=torch.bfloat16)
            for rule in RULES:
                xg = x.clone().requires_grad_(True)
                y = _sum_op(hg, op, cs, xg, hg.ops.Options(variant=variant, backward=rule))
                gx, = torch.autograd.grad(y, xg, G)
                assert y.dtype == gx.dtype == torch.bfloat16
                k = 2 if (rule == "adjoint" and graph.degV is not None) else 1
                ref = gr.evaluate(lambda g, x: gr.sum_aggr(g, x, rule), graph, {"x": x}, G, ["x"])
                _check("bf16 %s %s F=%d %s %s" % (op, shape, F, variant, rule), y, ref[0], ref[2], {"x": gx}, ref[1],
                       ref[3], gr.bf16_c(1), gr.bf16_c(k))


# ---- hgnnaggr_linear ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["cora", "pubmed", "ragged"])
@pytest.mark.parametrize("F_in,F_out", [(32, 32), (64, 16), (128, 128), (128, 64), (20, 7), (64, 7)])
def test_hgnnaggr_linear_gradients(hg, case, shape, F_in, F_out):
    """Fused and unfused forwards (fuse_linear always / auto / never; linear_math bf16x6 at F_in = 128), widths the
    epilogue takes and does not, the class-count widths of ops._wgrad's pad path; gradients of X and the weight."""
    cs = case(shape)
    graph = cs.graph("all")
    degE, degV, W = cs.scales["all"]
    N = cs.inc.N
    x = _randn(N, F_in, seed=1)
    wl = _randn(F_out, F_in, seed=2) / F_in ** 0.5
    G = _randn(N, F_out, seed=3)
    ptr, ind = cs.hyperg.H_T_csrptr, cs.hyperg.H_T_colind
    for fuse in ("always", "auto", "never"):
        for rule in RULES:
            math = "bf16x6" if F_in == 128 and rule == "adjoint" else "f32"
            opt = hg.ops.Options(fuse_linear=fuse, backward=rule, linear_math=math)
            xg, wg = x.clone().requires_grad_(True), wl.clone().requires_grad_(True)
            y = hg.ops.hgnnaggr_linear(ptr, ind, xg, wg, degE, degV, W, options=opt)
            gx, gw = torch.autograd.grad(y, (xg, wg), G)
            ref = gr.evaluate(lambda g, x, w: gr.hgnnaggr_linear(g, x, w, rule), graph, {"x": x, "w": wl}, G,
                              ["x", "w"])
            _check("hgnnaggr_linear %s %dx%d %s %s %s" % (shape, F_in, F_out, fuse, rule, math), y, ref[0], ref[2],
                   {"x": gx, "w": gw}, ref[1], ref[3], gr.FP32_C, gr.FP32_C)


@pytest.mark.parametrize("F_in,F_out", [(32, 32), (64, 16), (20, 7)])
def test_hgnnaggr_linear_bf16_gradients(hg, case, F_in, F_out):
    """bf16: torch's GEMM (one rounding) then the bf16 aggregation (one): output 2 roundings.  Backward: dZ = Aggr(G)
    rounds once (reference rule) or twice (adjoint: grad * degV first), then one GEMM each for dX and dW: 2 or 3."""
    cs = case("cora")
    graph = cs.graph("all")
    degE, degV, W = cs.scales["all"]
    N = cs.inc.N
    x = _randn(N, F_in, seed=4, dtype=torch.bfloat16)
    wl = (_randn(F_out, F_in, seed=5) / F_in ** 0.5).to(torch.bfloat16)
    G = _randn(N, F_out, seed=6, dtype=torch.bfloat16)
    for rule in RULES:
        xg, wg = x.clone().requires_grad_(True), wl.clone().requires_grad_(True)
        y = hg.ops.hgnnaggr_linear(cs.hyperg.H_T_csrptr, cs.hyperg.H_T_colind, xg, wg, degE, degV, W,
                                   options=hg.ops.Options(backward=rule))
        gx, gw = torch.autograd.grad(y, (xg, wg), G)
        assert y.dtype == gx.dtype == gw.dtype == torch.bfloat16
        ref = gr.evaluate(lambda g, x, w: gr.hgnnaggr_linear(g, x, w, rule), graph, {"x": x, "w": wl}, G, ["x", "w"])
        _check("bf16 hgnnaggr_linear %dx%d %s" % (F_in, F_out, rule), y, ref[0], ref[2], {"x": gx, "w": gw}, ref[1],
               ref[3], gr.bf16_c(2), gr.bf16_c(2 if rule == "reference" else 3))


# ---- aggr_res_linear ------------------------------------------------------------------------------------------------

# (ca, cb kind, residual, relu, gradients wanted, (F_in, F_out)).  cb kinds: "float"; "grad" = a device tensor that
# needs a gradient (UniGIN's 1 + eps); "const" = a device tensor that does not.
RES_CASES = [
    (1.0, "float", True, True, "all", (64, 64)),
    (0.9, "float", True, True, "all", (64, 64)),
    (0.9, "grad", True, False, "all", (64, 64)),
    (0.9, "const", True, True, "all", (32, 48)),
    (1e-3, "float", True, False, "all", (64, 64)),
    (2.0 ** -130, "float", True, True, "all", (64, 64)),    # subnormal in fp32
    (2.0 ** -130, "const", True, False, "r", (20, 20)),
    (0.0, "float", True, True, "all", (64, 64)),           # UniGCNII at alpha = 1
    (0.0, "const", True, False, "all", (64, 64)),
    (0.0, "grad", True, True, "all", (128, 64)),
    (-0.5, "float", True, True, "all", (64, 64)),
    (-0.5, "grad", True, False, "cb", (64, 64)),
    (0.9, "float", False, True, "all", (64, 64)),
    (1.0, "float", False, False, "m", (32, 32)),
    (-0.5, "float", False, False, "x", (20, 20)),
    (0.0, "float", False, True, "all", (64, 64)),
    (0.9, "float", True, True, "x", (64, 64)),
    (0.9, "float", True, True, "m", (64, 64)),
    (0.9, "float", True, True, "r", (64, 64)),
    (1.0, "grad", True, False, "cb", (64, 64)),
    (1e-3, "grad", True, True, "x", (128, 128)),
]


def _res_id(c):
    return "ca%g-%s-%s-%s-%s-%dx%d" % (c[0], c[1] if c[2] else "nores", "res" if c[2] else "", "relu" if c[3] else "lin",
                                        c[4], c[5][0], c[5][1])


@pytest.mark.parametrize("shape", ["cora", "pubmed"])
@pytest.mark.parametrize("cfg", RES_CASES, ids=[_res_id(c) for c in RES_CASES])
def test_aggr_res_linear_gradients(hg, case, shape, cfg):
    """act((ca Aggr(X) + cb R) M^T), degE / degV as in UniGCNII, for ca in {1, 0.9, 1e-3, 2^-130, 0, -0.5}, cb a float or
    a tensor with or without a gradient, with and without residual and relu, and each input's gradient asked for alone
    as well as all together (need_t and every needs_input_grad branch).  The relu mask is the kernel's own (out > 0);
    it must agree with the float64 pre-activation's sign wherever that is clear of the bound."""
    ca, cb_kind, has_res, relu, want, (F_in, F_out) = cfg
    cs = case(shape)
    graph = cs.graph("deg")
    degE, degV, _ = cs.scales["deg"]
    N = cs.inc.N
    x = _randn(N, F_in, seed=11)
    m = _randn(F_out, F_in, seed=12) / F_in ** 0.5
    res = _randn(N, F_in, seed=13) if has_res else None
    cbv = 0.3
    G = _randn(N, F_out, seed=14)
    names = [n for n in ("x", "m", "r", "cb") if (n != "r" or has_res) and (n != "cb" or (has_res and cb_kind == "grad"))]
    wrt = names if want == "all" else [want]
    for rule in RULES:
        t = {"x": x.clone(), "m": m.clone(), "r": None if res is None else res.clone(),
             "cb": torch.tensor(cbv, device=DEV) if cb_kind != "float" else cbv}
        for n in wrt:
            t[n].requires_grad_(True)
        y = hg.ops.aggr_res_linear(cs.hyperg.H_T_csrptr, cs.hyperg.H_T_colind, t["x"], t["m"], residual=t["r"], ca=ca,
                                   cb=t["cb"], degE=degE, degV=degV, relu=relu, options=hg.ops.Options(backward=rule))
        got = dict(zip(wrt, torch.autograd.grad(y, [t[n] for n in wrt], G)))
        mask = (y.detach() > 0).cpu() if relu else None
        inputs = {"x": x, "m": m, "r": res, "cb": torch.tensor(cbv, dtype=torch.float64) if cb_kind != "float" else cbv,
                  "ca": ca, "mask": mask}
        fn = lambda g, x, m, r, cb, ca, mask: gr.aggr_res_linear(g, x, m, rule, residual=r, ca=ca, cb=cb, mask=mask)
        ref = gr.evaluate(fn, graph, inputs, G, wrt)
        what = "aggr_res_linear %s %s %s" % (shape, _res_id(cfg), rule)
        _check(what, y, ref[0], ref[2], got, ref[1], ref[3], gr.FP32_C, gr.FP32_C)
        if relu:
            pre = gr.aggr_res_linear_pre(graph, gr.f64(x), gr.f64(m), gr.f64(res), ca, cbv)
            pre_mass = gr.aggr_res_linear_pre(graph.abs(), gr.f64(x).abs(), gr.f64(m).abs(),
                                              None if res is None else gr.f64(res).abs(), abs(ca), abs(cbv))
            gr.assert_mask_agrees(y, pre, pre_mass, gr.FP32_C, what)


def test_aggr_res_linear_bf16_gradients(hg, case):
    """bf16 (the torch form around the bf16 aggregation).  Roundings on the longest paths: forward T = Aggr(X) (1),
    * ca (1), + R * cb (2: the product, the sum), out = T M^T (1): 5 for the output; dM = dP^T T: T's 4 and the
    GEMM's 1 = 5; dX: dT = dP M (1; a folded ca rounds M * ca first: 1), the adjoint's * degV (1), the aggregation (1),
    * ca (1): 4; dR: dT (up to 2) and * cb (1): 3.  The bound takes 5 for every gradient."""
    cs = case("cora")
    graph = cs.graph("deg")
    degE, degV, _ = cs.scales["deg"]
    N, F = cs.inc.N, 64
    bf = torch.bfloat16
    x, m = _randn(N, F, seed=21, dtype=bf), (_randn(F, F, seed=22) / 8).to(bf)
    res, G = _randn(N, F, seed=23, dtype=bf), _randn(N, F, seed=24, dtype=bf)
    for ca, cb, relu in ((0.9, 0.1, True), (0.0, 1.0, False), (-0.5, 0.25, True)):
        for rule in RULES:
            t = {"x": x.clone().requires_grad_(True), "m": m.clone().requires_grad_(True),
                 "r": res.clone().requires_grad_(True)}
            y = hg.ops.aggr_res_linear(cs.hyperg.H_T_csrptr, cs.hyperg.H_T_colind, t["x"], t["m"], residual=t["r"],
                                       ca=ca, cb=cb, degE=degE, degV=degV, relu=relu,
                                       options=hg.ops.Options(backward=rule))
            got = dict(zip(("x", "m", "r"), torch.autograd.grad(y, (t["x"], t["m"], t["r"]), G)))
            mask = (y.detach() > 0).cpu() if relu else None
            fn = lambda g, x, m, r, ca, cb, mask: gr.aggr_res_linear(g, x, m, rule, residual=r, ca=ca, cb=cb, mask=mask)
            ref = gr.evaluate(fn, graph, {"x": x, "m": m, "r": res, "ca": ca, "cb": cb, "mask": mask}, G,
                              ["x", "m", "r"])
            _check("bf16 aggr_res_linear ca=%g %s" % (ca, rule), y, ref[0], ref[2], got, ref[1], ref[3], gr.bf16_c(5),
                   gr.bf16_c(5))


# ---- ops.Linear -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,F_in,F_out,path", [
    (6000, 64, 64, "rows+wgrad"),  # both library kernels
    (6000, 64, 7, "pad"),          # class count: wgrad on 16-column padded operands, dX on torch
    (6000, 20, 32, "pad"),         # F_in = 20: the pad path on the other operand
    (6000, 128, 48, "torch"),      # widths neither kernel takes
    (BIG_ROWS, 32, 32, "rows+wgrad"),
    (BIG_ROWS - 1, 64, 64, "torch"),  # one row short of the switch
])
def test_linear_module_gradients(hg, monkeypatch, rows, F_in, F_out, path):
    from hypergef_amd import ops
    paths = _PathCounter(monkeypatch)
    torch.manual_seed(rows + F_in + F_out)
    lin = ops.Linear(F_in, F_out).to(DEV)
    x = _randn(rows, F_in, seed=31)
    G = _randn(rows, F_out, seed=32)
    xg = x.clone().requires_grad_(True)
    y = lin(xg)
    gx, gw, gb = torch.autograd.grad(y, (xg, lin.weight, lin.bias), G)
    fn = lambda g, x, w, b: gr.linear(x, w, b)
    ref = gr.evaluate(fn, None, {"x": x, "w": lin.weight, "b": lin.bias}, G, ["x", "w", "b"])
    _check("Linear %d %dx%d" % (rows, F_in, F_out), y, ref[0], ref[2], {"x": gx, "w": gw, "b": gb}, ref[1], ref[3],
           gr.FP32_C, gr.FP32_C)
    if path == "rows+wgrad":
        assert paths.rows == [(rows, (F_in, F_out))] and paths.wgrad == [(rows, F_out, F_in)]
    elif path == "pad":
        assert paths.wgrad == [(rows, F_out + (-F_out) % 16, F_in + (-F_in) % 16)]
    else:
        assert paths.rows == [] and paths.wgrad == []


# ---- the layers, on both sides of the 4096-row switch ---------------------------------------------------------------

@pytest.mark.parametrize("shape", ["cora", "pubmed", "n4096"])
@pytest.mark.parametrize("layer", ["HGNN", "UniGIN", "UniGCNII"])
def test_layer_gradients(hg, case, monkeypatch, shape, layer):
    """HyperGsysHGNN / HyperGsysUinGINConv / HyperGsysUniGCNII (alpha = 0.1, 1 and 0) against their float64 formulas,
    every parameter's and input's gradient, both rules; below 4096 rows the backward GEMMs must be torch's, from 4096
    on the library's (asserted through the calls of ops.linear_rows / ops.linear_wgrad)."""
    from hypergef_amd import models, ops
    cs = case(shape)
    N = cs.inc.N
    big = N >= BIG_ROWS
    paths = _PathCounter(monkeypatch)
    torch.manual_seed(41)
    if layer == "HGNN":
        runs = [((64, 64), None), ((128, 64), None)]
    elif layer == "UniGIN":
        runs = [((64, 64), None), ((32, 32), None)]
    else:
        runs = [((64, 64), 0.1), ((64, 64), 1.0), ((64, 64), 0.0)]
    for (F_in, F_out), alpha in runs:
        if layer == "HGNN":
            mod = models.HyperGsysHGNN(cs.hyperg, F_in, F_out, "sum").to(DEV)
        elif layer == "UniGIN":
            mod = models.HyperGsysUinGINConv(cs.hyperg, F_in, F_out, "sum").to(DEV)
            mod.eps.data.fill_(0.25)
        else:
            mod = models.HyperGsysUniGCNII(cs.hyperg, F_in, F_out).to(DEV)
        x = _randn(N, F_in, seed=42)
        x0 = _randn(N, F_in, seed=43)
        G = _randn(N, F_out, seed=44)
        beta = 0.4
        for rule in RULES:
            xg, x0g = x.clone().requires_grad_(True), x0.clone().requires_grad_(True)
            with ops.options(backward=rule):
                y = mod(xg, x0g, alpha, beta, relu=True) if layer == "UniGCNII" else mod(xg)
            params = {"x": xg, "w": mod.W.weight}
            if layer == "UniGIN":
                params["eps"] = mod.eps
            if layer == "UniGCNII":
                params["x0"] = x0g
            paths.reset()
            got = dict(zip(params, torch.autograd.grad(y, list(params.values()), G)))
            torch.cuda.synchronize()
            what = "%s %s %dx%d alpha=%s %s" % (layer, shape, F_in, F_out, alpha, rule)
            if layer == "HGNN":
                fn = lambda g, x, w: gr.hgnnaggr_linear(g, x, w, rule)
                ref = gr.evaluate(fn, cs.graph("deg"), {"x": x, "w": mod.W.weight}, G, list(params))
            elif layer == "UniGIN":
                fn = lambda g, x, w, eps: gr.unigin(g, x, w, eps, rule)
                ref = gr.evaluate(fn, cs.graph("none"), {"x": x, "w": mod.W.weight, "eps": mod.eps}, G, list(params))
            else:
                mask = (y.detach() > 0).cpu()
                fn = lambda g, x, x0, w, k, mask: gr.unigcnii(g, x, x0, w, rule, *k, mask)
                k = (1 - alpha, alpha, 1 - beta, beta)
                ref = gr.evaluate(fn, cs.graph("deg"), {"x": x, "x0": x0, "w": mod.W.weight, "k": k, "mask": mask}, G,
                                  list(params))
            _check(what, y, ref[0], ref[2], got, ref[1], ref[3], gr.FP32_C, gr.FP32_C)
            if big:
                assert paths.rows and paths.wgrad, "%s: the backward GEMMs did not run on the library's kernels" % what
                assert all(r == N for r, _ in paths.rows) and all(w[0] == N for w in paths.wgrad), what
            else:
                assert not paths.rows and not paths.wgrad, "%s: the library's GEMM kernels ran below %d rows" % (
                    what, BIG_ROWS)
