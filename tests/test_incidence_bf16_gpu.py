"""bf16 feature rows on the incidence path (hg_aggr_incidence_heads_bf16, hg_gather_rows_incidence_heads_bf16,
hg_incidence_dot_heads_bf16 and the layers above them).  The contract is "fp32 in between, the fp32 call's order, one
rounding", so every comparison is bitwise against the float32 call on the widened inputs -- no tolerance anywhere.

Graphs: toy, boundaries, ragged+dups (_incidence_ref); plan-option sets default, small, lat, all with row_stream=False:
between them panels, wave tasks, partial slots, two fixup levels and the latency schedule.  Widths: single head
F in {4, 64, 260}; (H, C) in (4, 8), (8, 40); (4, 3) for the widen-and-round fallback.  Inputs are randn rounded to bf16; the
weights come from the segment softmax, and signed random weights with 10 % exact zeros.

1. Plan.aggregate_incidence on bf16 X: Y and xe_out, every weight combination, with and without the scales.
2. Plan.gather_rows_incidence, io = 1, 2, 3 at both hops, inside guard words; hop 0 into hop 1 gives the two-hop Y.
3. Plan.incidence_dot, the three mixed forms.
4. Autograd through ops.incidence_aggr / incidence_gather / incidence_dot with Options(incidence_bf16="rows").
5. HypergraphAttnConv(...).to(bfloat16), additive and dot, H in {1, 4} (the TypeError of the float32-only operators before).
6. The C entries' refusals: status, hg_last_error, nothing written.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402
import _incidence_ref as ir  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = ar.DEV
SENTINEL = -12352.0  # a bf16 number (-193 * 2^6): a guard word reads back the same in either dtype
BF, F32 = torch.bfloat16, torch.float32
GUARD_BYTES = 256  # on either side of a guarded output: keeps 16-byte alignment
GRAPHS = ("toy", "boundaries", "ragged+dups")
SETS = ("default", "small", "lat")
KINDS = [(1, 4), (1, 64), (1, 260), (4, 8), (8, 40), (4, 3)]  # (H, C); (4, 3): C % 4 != 0, widen / float32 call / round
COMBOS = ("both", "v2e", "e2v", "neither")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _guarded(dtype, *shape):
    """(buffer, view): a SENTINEL-filled buffer of `dtype` and the output inside it, GUARD_BYTES on either side."""
    n, g = int(np.prod(shape)), GUARD_BYTES // torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * g,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[g:g + n].view(*shape)


def _guards_intact(buf, view):
    g = (buf.numel() - view.numel()) // 2
    return bool((buf[:g] == SENTINEL).all()) and bool((buf[-g:] == SENTINEL).all())


def _randn(shape, seed, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV).to(dtype)


class _Case:
    """One graph on the device: its plans (one per option set, row_stream=False), scales and the inputs of every kind."""

    def __init__(self, hg, name):
        from hypergef_amd.plan import Plan
        self.name, self.Plan = name, Plan
        self.inc = inc = ir.schedule_graph(name)
        self.h = hg.HyperGraph.from_incidence(inc, DEV, data_name="bf16-" + name, ngs=1 << 30)
        self.ptr, self.ind = self.h.H_T_csrptr, self.h.H_T_colind
        self.N, self.M, self.nnz = inc.N, inc.M, inc.nnz
        rng = np.random.default_rng(11)
        self.W = torch.from_numpy(rng.random(inc.M).astype(np.float32) + 0.5).to(DEV)
        self.degE, self.degV = self.h.degE.reshape(-1).contiguous(), self.h.degV.reshape(-1).contiguous()
        self.empty = torch.from_numpy(np.diff(inc.csrptr) == 0).to(DEV)
        assert name == "boundaries" or (bool(self.empty.any()) and bool(torch.isinf(self.degE[self.empty]).all()))
        self._plans, self._inputs = {}, {}

    def plan(self, opts):
        from hypergef_amd.plan import make_opts
        if opts not in self._plans:
            self._plans[opts] = self.Plan.from_tensors(self.N, self.ptr, self.ind, make_opts(row_stream=False, **ir.option_sets()[opts]))
        return self._plans[opts]

    def scales(self, on):
        return (self.degE, self.degV, self.W) if on else (None, None, None)

    def inputs(self, kind):
        """X bf16 [N, H C], Xe bf16 [M, H C] (a table for hop 1 and the dot), fp32 rows Xf / Xef that bf16 does not hold, and
        two weight sets (v2e, e2v): the segment softmax's coefficients, and signed random weights with 10 % exact zeros."""
        if kind not in self._inputs:
            H, C = kind
            F, seed = H * C, 1000 * H + C
            shape = (self.nnz,) if H == 1 else (self.nnz, H)
            sshape = lambda n: (n,) if H == 1 else (n, H)  # noqa: E731
            plan = self.plan("default")
            soft = tuple(plan.incidence_attention(self.ptr, self.ind, _randn(sshape(self.N), seed + 1 + i), _randn(sshape(self.M), seed + 3 + i),
                                                  group, 0.2, heads=H) for i, group in enumerate(("hyperedge", "vertex")))
            signed = []
            for i in range(2):
                w = _randn(shape, seed + 5 + i)
                w[_randn(shape, seed + 7 + i) > 1.2816] = 0.0  # the upper 10 % of a normal draw
                signed.append(w.contiguous())
            self._inputs[kind] = dict(Xb=_randn((self.N, F), seed, BF), Xeb=_randn((self.M, F), seed + 9, BF),
                                      Xf=_randn((self.N, F), seed + 10), Xef=_randn((self.M, F), seed + 11),
                                      soft=soft, signed=tuple(signed))
        return self._inputs[kind]


_CASES = {}


@pytest.fixture
def case(hg):
    def get(name):
        if name not in _CASES:
            _CASES[name] = _Case(hg, name)
        return _CASES[name]
    return get


def _pick(weights, combo):
    return (weights[0] if combo in ("both", "v2e") else None), (weights[1] if combo in ("both", "e2v") else None)


# ---- 1. the two-hop entry -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opts", SETS)
@pytest.mark.parametrize("name", GRAPHS)
def test_aggregate_incidence_equals_the_rounded_fp32_call(case, name, opts):
    c = case(name)
    plan = c.plan(opts)
    for kind in KINDS:
        H, C = kind
        inp = c.inputs(kind)
        Xb, Xf = inp["Xb"], inp["Xb"].float()
        for on in (True, False):
            degE, degV, W = c.scales(on)
            for wname, combo in [(w, k) for w in ("soft", "signed") for k in COMBOS[:3]] + [("none", "neither")]:
                v2e, e2v = _pick(inp.get(wname, (None, None)), combo)
                what = "%s/%s (H, C) = %s %s %s scales %s" % (name, opts, kind, wname, combo, on)
                xe32 = torch.empty(c.M, H * C, device=DEV)
                y32 = plan.aggregate_incidence(c.ptr, c.ind, Xf, v2e, e2v, degE, degV, W, xe_out=xe32, heads=H)
                ybuf, Y = _guarded(BF, c.N, H * C)
                xbuf, xe = _guarded(F32, c.M, H * C)
                got = plan.aggregate_incidence(c.ptr, c.ind, Xb, v2e, e2v, degE, degV, W, xe_out=xe, out=Y, heads=H)
                assert got is Y and _eq(Y, y32.to(BF)), what
                assert _eq(xe, xe32), what + ": xe_out"
                assert _guards_intact(ybuf, Y) and _guards_intact(xbuf, xe), what
                assert bool(torch.isfinite(Y.float()).all()), what
                if on:  # degE = inf on an empty hyperedge: its row of the table is exactly 0, not inf * 0
                    assert not bool(xe[c.empty].any()), what
                # without xe_out (the table in the workspace) and without out
                assert _eq(plan.aggregate_incidence(c.ptr, c.ind, Xb, v2e, e2v, degE, degV, W, heads=H), Y), what
                if combo == "neither":  # the unweighted instances: the pull call on bf16 rows of the same plan
                    assert _eq(plan.aggregate(c.ptr, c.ind, Xb, degE, degV, W, variant="pull", bind_scales=False), Y), what


def test_plan_level_refusals(case):
    c = case("toy")
    plan = c.plan("default")
    inp = c.inputs((1, 4))
    with pytest.raises(TypeError, match="float32"):
        plan.aggregate_incidence(c.ptr, c.ind, inp["Xb"], inp["soft"][0].to(BF), None)
    with pytest.raises(TypeError, match="float32"):
        plan.aggregate_incidence(c.ptr, c.ind, inp["Xb"], xe_out=torch.empty(c.M, 4, dtype=BF, device=DEV))
    with pytest.raises(TypeError, match="dtype"):
        plan.aggregate_incidence(c.ptr, c.ind, inp["Xb"], out=torch.empty(c.N, 4, device=DEV))
    with pytest.raises(TypeError, match="float32"):
        plan.gather_rows_incidence(0, c.ptr, c.ind, inp["Xb"], inp["soft"][0].to(BF))
    with pytest.raises(TypeError, match="float32"):
        plan.incidence_dot(c.ptr, c.ind, inp["Xb"], inp["Xeb"], out=torch.empty(c.nnz, dtype=BF, device=DEV))


# ---- 2. one hop ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opts", SETS)
@pytest.mark.parametrize("name", GRAPHS)
def test_gather_rows_incidence_mixed_forms(case, name, opts):
    c = case(name)
    plan = c.plan(opts)
    for kind in KINDS:
        H, C = kind
        F = H * C
        inp = c.inputs(kind)
        for wname in ("soft", "signed", "none"):
            for hop in (0, 1):
                w = None if wname == "none" else inp[wname][hop]
                ndst = c.M if hop == 0 else c.N
                sA, sB = (c.degE, c.W) if hop == 0 else (c.degV, None)
                srcb = inp["Xb"] if hop == 0 else inp["Xeb"]
                srcf = inp["Xf"] if hop == 0 else inp["Xef"]  # fp32 rows that are no bf16 numbers
                for io in (1, 2, 3):
                    src = srcb if io & 1 else srcf
                    what = "%s/%s (H, C) = %s %s hop %d io %d" % (name, opts, kind, wname, hop, io)
                    want = plan.gather_rows_incidence(hop, c.ptr, c.ind, src.float(), w, sA, sB, heads=H)
                    buf, out = _guarded(BF if io & 2 else F32, ndst, F)
                    got = plan.gather_rows_incidence(hop, c.ptr, c.ind, src, w, sA, sB, heads=H, out=out)
                    assert got is out and _eq(out, want.to(out.dtype)), what
                    assert _guards_intact(buf, out), what
                # the result's dtype follows src where out does not say otherwise
                assert plan.gather_rows_incidence(hop, c.ptr, c.ind, srcb, w, sA, sB, heads=H).dtype == BF
        # hop 0 (bf16 -> fp32) into hop 1 (fp32 -> bf16) is the two-hop entry
        v2e, e2v = inp["signed"]
        xe = plan.gather_rows_incidence("hyperedge", c.ptr, c.ind, inp["Xb"], v2e, c.degE, c.W, heads=H,
                                        out=torch.empty(c.M, F, device=DEV))
        y = plan.gather_rows_incidence("vertex", c.ptr, c.ind, xe, e2v, c.degV, None, heads=H,
                                       out=torch.empty(c.N, F, dtype=BF, device=DEV))
        xe2 = torch.empty(c.M, F, device=DEV)
        y2 = plan.aggregate_incidence(c.ptr, c.ind, inp["Xb"], v2e, e2v, c.degE, c.degV, c.W, xe_out=xe2, heads=H)
        assert _eq(xe, xe2) and _eq(y, y2), "%s/%s (H, C) = %s: hop 0 into hop 1" % (name, opts, kind)


# ---- 3. the dot -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GRAPHS)
def test_incidence_dot_mixed_forms(case, name):
    c = case(name)
    plan = c.plan("default")
    for kind in KINDS:
        H, C = kind
        inp = c.inputs(kind)
        for io in (1, 2, 3):
            A = inp["Xb"] if io & 1 else inp["Xf"]
            B = inp["Xeb"] if io & 2 else inp["Xef"]
            want = plan.incidence_dot(c.ptr, c.ind, A.float(), B.float(), heads=H)
            buf, out = _guarded(F32, *((c.nnz,) if H == 1 else (c.nnz, H)))
            got = plan.incidence_dot(c.ptr, c.ind, A, B, out=out, heads=H)
            what = "%s (H, C) = %s io %d" % (name, kind, io)
            assert got is out and _eq(out, want), what
            assert _guards_intact(buf, out), what


# ---- 4. autograd ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [(1, 64), (4, 8), (4, 3)])
def test_autograd_of_incidence_aggr(hg, case, kind):
    from hypergef_amd.plan import cached_plan
    ops = hg.ops
    c = case("ragged+dups")
    H, C = kind
    inp = c.inputs(kind)
    rows = ops.Options(incidence_bf16="rows")
    plan = cached_plan(c.N, c.ptr, c.ind)  # the plan the operators run on
    X = inp["Xb"].clone().requires_grad_(True)
    v2e, e2v = (w.clone().requires_grad_(True) for w in inp["signed"])
    degE, degV, W = (t.clone().requires_grad_(True) for t in c.scales(True))
    g = _randn((c.N, H * C), 77, BF)
    Y = ops.incidence_aggr(c.ptr, c.ind, X, v2e, e2v, degE, degV, W, options=rows, heads=H)
    assert Y.dtype == BF
    Y.backward(g)
    # the float32 operators on the widened inputs
    f32 = lambda x, a, b, dv, xe_out=None: plan.aggregate_incidence(  # noqa: E731
        c.ptr, c.ind, x, a.detach(), b.detach(), c.degE, dv, c.W, xe_out=xe_out, heads=H)
    Xe = torch.empty(c.M, H * C, device=DEV)
    assert _eq(Y.detach(), f32(X.detach().float(), v2e, e2v, c.degV, Xe).to(BF))
    P = (g.float() * c.degV.reshape(-1, 1)).to(BF)
    G = torch.empty(c.M, H * C, device=DEV)
    assert X.grad.dtype == BF and _eq(X.grad, f32(P.float(), e2v, v2e, None, G).to(BF))
    assert v2e.grad.dtype == F32 and _eq(v2e.grad, plan.incidence_dot(c.ptr, c.ind, X.detach().float(), G, heads=H).view_as(v2e))
    assert e2v.grad.dtype == F32 and _eq(e2v.grad, plan.incidence_dot(c.ptr, c.ind, P.float(), Xe, heads=H).view_as(e2v))
    for t in (degE, degV, W):  # the scale gradients: the float32 kernels on the widened X and P
        assert t.grad is not None and t.grad.dtype == F32 and t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all())
    q = plan.hyperedge_dot(c.ptr, c.ind, X.detach().float(), P.float(), v2e.detach(), e2v.detach(), heads=H)
    live = ~c.empty
    assert _eq(W.grad[live], (q * c.degE)[live]) and not bool(W.grad[c.empty].any())
    # without a gradient wanted no node is made and the bits are the same
    with torch.no_grad():
        assert _eq(ops.incidence_aggr(c.ptr, c.ind, X, v2e, e2v, degE, degV, W, options=rows, heads=H), Y.detach())
    assert _eq(ops.HGNNAggrIncidence(c.h, X.detach(), v2e.detach(), e2v.detach(), c.degE, c.degV, c.W, options=rows, heads=H),
               Y.detach())


@pytest.mark.parametrize("kind", [(1, 64), (4, 8)])
def test_autograd_of_gather_and_dot(hg, case, kind):
    from hypergef_amd.plan import cached_plan
    ops = hg.ops
    c = case("ragged+dups")
    H, C = kind
    inp = c.inputs(kind)
    rows = ops.Options(incidence_bf16="rows")
    plan = cached_plan(c.N, c.ptr, c.ind)
    hop = lambda to, src, w, sa=None: plan.gather_rows_incidence(to, c.ptr, c.ind, src, w, sa, heads=H)  # noqa: E731
    inv = torch.nan_to_num(c.degE, posinf=0.0)
    # incidence_gather: weighted with a scale, and unweighted (the layer's hyperedge keys)
    for w0 in (inp["signed"][0], None):
        src = inp["Xb"].clone().requires_grad_(True)
        w = None if w0 is None else w0.clone().requires_grad_(True)
        out = ops.incidence_gather(c.ptr, c.ind, src, w, to="hyperedge", scale_a=inv, heads=H, options=rows)
        assert out.dtype == BF and _eq(out.detach(), hop("hyperedge", src.detach().float(), w0, inv).to(BF))
        g = _randn((c.M, H * C), 78, BF)
        out.backward(g)
        gs = g.float() * inv.reshape(-1, 1)  # float32: the mixed hop (fp32 -> bf16) and dot (bf16, fp32)
        assert src.grad.dtype == BF and _eq(src.grad, hop("vertex", gs, w0).to(BF))
        if w is not None:
            assert w.grad.dtype == F32
            assert _eq(w.grad, plan.incidence_dot(c.ptr, c.ind, src.detach().float(), gs, heads=H).view_as(w))
    # incidence_dot: each gradient in its operand's dtype
    for da, db in ((BF, BF), (BF, F32), (F32, BF)):
        A = (inp["Xb"] if da == BF else inp["Xf"]).clone().requires_grad_(True)
        B = (inp["Xeb"] if db == BF else inp["Xef"]).clone().requires_grad_(True)
        out = ops.incidence_dot(c.ptr, c.ind, A, B, heads=H, options=rows)
        assert out.dtype == F32 and _eq(out.detach(), plan.incidence_dot(c.ptr, c.ind, A.detach().float(), B.detach().float(), heads=H))
        g = _randn(tuple(out.shape), 79)
        out.backward(g)
        assert A.grad.dtype == da and _eq(A.grad, hop("vertex", B.detach().float(), g).to(da))
        assert B.grad.dtype == db and _eq(B.grad, hop("hyperedge", A.detach().float(), g).to(db))


# ---- 5. the layer ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("score", ["additive", "dot"])
def test_layer_in_bfloat16(hg, score, heads):
    ops = hg.ops
    inc = synth.random_incidence(300, 40, 150.0, seed=6)
    hyperg = hg.HyperGraph.from_incidence(inc, DEV, data_name="dense-bf16-layer", ngs=1 << 30)
    torch.manual_seed(4)
    kw = dict(heads=heads, score=score, learn_hyperedge_weight=True)
    layer = hg.HypergraphAttnConv(hyperg, 12, 8, **kw).to(DEV).to(BF)
    with torch.no_grad():
        layer.bias.copy_(torch.randn_like(layer.bias))
    X = _randn((inc.N, 12), 5, BF)
    x = X.clone().requires_grad_(True)
    y = layer(x)
    assert y.dtype == BF and tuple(y.shape) == (inc.N, heads * 8)
    with torch.no_grad():
        Z = layer.lin(X)
        alpha = layer.coefficients(Z, X)
        assert Z.dtype == BF and alpha.dtype == F32
        want = ops.incidence_aggr(hyperg.H_T_csrptr, hyperg.H_T_colind, Z.float(), alpha, alpha, hyperg.degE, hyperg.degV,
                                  layer.Wdiag.float(), heads=heads).to(BF) + layer.bias
    assert _eq(y.detach(), want)
    y.backward(_randn(tuple(y.shape), 6, BF))
    assert x.grad is not None and x.grad.dtype == BF and bool(torch.isfinite(x.grad.float()).all())
    for n, p in layer.named_parameters():
        assert p.grad is not None and p.grad.dtype == p.dtype == BF, n
        assert bool(torch.isfinite(p.grad.float()).all()), n
    # fuse_attention=True takes the composed path on bf16 rows without a word
    fused = hg.HypergraphAttnConv(hyperg, 12, 8, fuse_attention=True, **kw).to(DEV).to(BF)
    fused.load_state_dict(layer.state_dict())
    assert _eq(fused(X).detach(), y.detach())
    # the float32 layer keeps the float32 operators: the default options still refuse bf16 rows given to them directly
    with pytest.raises(TypeError, match="no bfloat16 form"):
        ops.incidence_aggr(hyperg.H_T_csrptr, hyperg.H_T_colind, Z, alpha, alpha, heads=heads)


# ---- 6. the C entries' refusals -------------------------------------------------------------------------------------------------

def test_c_level_refusals(hg, case):
    from hypergef_amd import _lib
    from hypergef_amd.plan import Plan, make_opts, _ptr, _stream_handle
    L = _lib.lib()
    c = case("toy")
    plan = c.plan("default")
    host = Plan.from_host(c.N, c.M, c.inc.csrptr, c.inc.colind, opts=make_opts(host_only=True))
    F, H = 16, 4
    nbytes = plan.incidence_workspace_bytes(F)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
    wsb = nbytes
    stream = _stream_handle(torch.device(DEV))
    Xb, Xf = _randn((c.N, F + 4), 1, BF), _randn((c.N, F), 2)  # Xb: room for a view two bytes further on
    Xeb = _randn((c.M, F), 3, BF)
    w = _randn((c.nnz, H), 4)
    off2 = Xb.reshape(-1)[1:1 + c.N * F]  # bf16 rows at a 2-byte-misaligned address
    assert off2.data_ptr() % 8 == 2

    def outputs():
        return (torch.full((c.M, F), SENTINEL, device=DEV), torch.full((c.N, F), SENTINEL, dtype=BF, device=DEV),
                torch.full((c.nnz, H), SENTINEL, device=DEV))

    def gather(p, F, H, src, dst, io):
        return L.hg_gather_rows_incidence_heads_bf16(p._h, 0, F, H, _ptr(c.ptr), _ptr(c.ind), _ptr(src), _ptr(w), None, None,
                                                     _ptr(dst), _ptr(ws), wsb, io, stream)

    def aggr(p, F, H, X, xe, Y):
        return L.hg_aggr_incidence_heads_bf16(p._h, F, H, _ptr(c.ptr), _ptr(c.ind), _ptr(X), _ptr(w), _ptr(w), None, None, None,
                                              _ptr(xe), _ptr(Y), _ptr(ws), wsb, stream)

    def dot(p, F, H, A, B, out, io):
        return L.hg_incidence_dot_heads_bf16(p._h, F, H, _ptr(c.ptr), _ptr(c.ind), _ptr(A), _ptr(B), _ptr(out), io, stream)

    Xb16 = Xb[:, :F].contiguous()
    with torch.cuda.device(DEV):
        cases = [
            ("io = 0", _lib.HG_ERR_INVALID, b"io must be", lambda xe, Y, o: gather(plan, F, H, Xb16, xe, 0)),
            ("io = 0", _lib.HG_ERR_INVALID, b"io must be", lambda xe, Y, o: dot(plan, F, H, Xb16, Xeb, o, 0)),
            ("C % 4", _lib.HG_ERR_UNSUPPORTED, b"C % 4 == 0", lambda xe, Y, o: gather(plan, F, 8, Xb16, xe, 1)),
            ("C % 4", _lib.HG_ERR_UNSUPPORTED, b"C % 4 == 0", lambda xe, Y, o: aggr(plan, F, 8, Xb16, xe, Y)),
            ("C % 4", _lib.HG_ERR_UNSUPPORTED, b"C % 4 == 0", lambda xe, Y, o: dot(plan, F, 8, Xb16, Xeb, o, 3)),
            ("misaligned", _lib.HG_ERR_UNSUPPORTED, b"8-byte aligned", lambda xe, Y, o: gather(plan, F, H, off2, xe, 1)),
            ("misaligned", _lib.HG_ERR_UNSUPPORTED, b"8-byte aligned", lambda xe, Y, o: aggr(plan, F, H, off2, xe, Y)),
            ("misaligned", _lib.HG_ERR_UNSUPPORTED, b"8-byte aligned", lambda xe, Y, o: dot(plan, F, H, off2, Xeb, o, 3)),
            ("misaligned fp32", _lib.HG_ERR_UNSUPPORTED, b"16-byte aligned",
             lambda xe, Y, o: gather(plan, F, H, Xf.reshape(-1)[1:], Y, 2)),
            ("host-only", _lib.HG_ERR_UNSUPPORTED, b"HG_PLAN_HOST_ONLY", lambda xe, Y, o: gather(host, F, H, Xb16, xe, 1)),
            ("host-only", _lib.HG_ERR_UNSUPPORTED, b"HG_PLAN_HOST_ONLY", lambda xe, Y, o: aggr(host, F, H, Xb16, xe, Y)),
            ("host-only", _lib.HG_ERR_UNSUPPORTED, b"HG_PLAN_HOST_ONLY", lambda xe, Y, o: dot(host, F, H, Xb16, Xeb, o, 3)),
        ]
        for what, status, words, call in cases:
            xe, Y, o = outputs()
            assert call(xe, Y, o) == status, what
            assert words in L.hg_last_error(), (what, L.hg_last_error())
            torch.cuda.synchronize()
            for t in (xe, Y, o):
                assert bool((t == SENTINEL).all()), what
        # and the same arguments, well formed, run
        xe, Y, o = outputs()
        assert gather(plan, F, H, Xb16, xe, 1) == 0 and aggr(plan, F, H, Xb16, None, Y) == 0 and dot(plan, F, H, Xb16, Xeb, o, 3) == 0
        torch.cuda.synchronize()
        for t in (xe, Y, o):
            assert not bool((t == SENTINEL).any())
