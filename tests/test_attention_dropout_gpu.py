"""Attention dropout on the GPU: the fused softmax + dropout and its backward (hg_incidence_attention_dropout_heads_f32 /
_bwd_f32, Plan.incidence_attention_dropout(_backward), ops.incidence_softmax(dropout=...), HypergraphAttnConv(dropout=...)).

Shapes, the smallest that reach every path: the toy graph of the host tests (lane groups of 4); `ragged` (10 % empty
hyperedges, lane groups of 8); `sizes` -- one hyperedge of every size 0 .. 70, which crosses (entries kept in registers) x
(lane-group width) for the widths 4, 8 and 16; `long` -- one hyperedge each of 127, 128, 129, 1023, 1024 and 1025 members, on
both sides of the longest row a lane group takes and of 256 lanes x entries kept (the re-gather tail of a workgroup's
segment) -- and its transpose, which puts the same rows on the vertex side.

Checks a - d and f - i compare bits, and never against the code under test: alpha against the plain softmax; the dropped
coefficients against where(keep, alpha * scale, 0) with keep from the library's host statement of the mask (itself pinned to
the published Philox by tests/test_attention_dropout_host.py) and scale = float32(1) / (float32(1) - float32(p)); the
backward against the existing backward kernel on the pre-masked, pre-scaled gradient.

Check e holds the output and both gradients of ops.incidence_softmax(dropout=p) against float64 (softmax in float64, times
the mask, times 1 / (1 - p)) within the bounds of tests/test_attention_gpu.py, each multiplied by scale:
    output:     |got - ref| <= scale c alpha64,                       c = (L + 16 + 16 Smax) U
    gradients:  |got - ref| <= scale (2 c + (L + D + 8) U) max(mass, TINY)
with alpha64 the undropped float64 coefficient, mass that file's masses for dalpha = keep dout (before the scale), L the
longest group of the side, D the longest segment of the reducing side, U = 2^-24.  Derivation: dropout multiplies the
coefficient (the gradient) by the exact 0 or by scale, so an error bound relative to the coefficient (to the mass, which
is linear in dalpha) is multiplied by scale and nothing else.  What the scaling adds itself -- the rounding of the fp32
scale against 1 / (1 - p) in float64 and of the one product, 2 U relative -- lies inside the slack of those bounds: c
counts L + 4 + 16 Smax roundings and allows 12 more, the gradient's + 8 U covers six operations.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402
import _dropout_ref as dr  # noqa: E402
import _grad_ref as gr  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = ar.DEV
U = ar.U
PDS = (0.1, 0.5)
HEADS = (1, 3)
STATE = (0x0123456789ABCDEF, -0x0EDCBA9876543210)  # {key, sid} as int64


def _long():
    return synth._from_sizes(np.random.default_rng(5), 1100, [127, 128, 129, 1023, 1024, 1025], name="long")


SHAPES = {
    "toy": ar.toy,
    "ragged": lambda: synth.random_incidence(700, 450, 7.0, seed=3, empty_frac=0.1),
    "sizes": lambda: synth._from_sizes(np.random.default_rng(7), 200, list(range(71)), name="sizes"),
    "long": _long,
    "long_T": lambda: ar.transpose(_long()),
}

_bits = ar.bits


class Case(ar.Case):
    """ar.Case with scores, gradients and references for every head count: column h of the H-head arrays is an array of
    its own draw, so the float64 reference of a column is the single-head one."""

    def __init__(self, hg, inc, name):
        super().__init__(hg, inc, name)
        g = torch.Generator().manual_seed(33)
        self.hsv, self.hse, self.hdout = {1: self.sv}, {1: self.se}, {1: self.dalpha}
        for H in HEADS:
            if H > 1:
                sv, se = torch.randn(inc.N, H, generator=g), torch.randn(inc.M, H, generator=g)
                self.hsv[H] = (sv * (4.0 / float(sv.abs().max()))).to(DEV)
                self.hse[H] = (se * (4.0 / float(se.abs().max()))).to(DEV)
                self.hdout[H] = torch.randn(inc.nnz, H, generator=g).to(DEV)
        self.rng = torch.tensor(STATE, dtype=torch.int64, device=DEV)
        self._keep, self._ref64 = {}, {}

    def keep(self, pd, H, rng=None):
        """bool [nnz] / [nnz, H] on the device, from hg_dropout_keep_host."""
        key = (pd, H) if rng is None else None
        if key is None or key not in self._keep:
            k = torch.from_numpy(dr.keep_of_state(self.rng if rng is None else rng, pd, self.inc.nnz, H)).to(DEV)
            k = k.reshape(-1) if H == 1 else k
            if key is None:
                return k
            self._keep[key] = k
        return self._keep[key]

    def ref64(self, H, group, slope):
        """float64 (alpha [nnz, H], Smax) from the fp32 scores: computed once, shared, never modified."""
        key = (H, group, slope)
        if key not in self._ref64:
            sv, se = gr.f64(self.hsv[H]).reshape(-1, H), gr.f64(self.hse[H]).reshape(-1, H)
            cols = [ar.softmax(self.graph, sv[:, h], se[:, h], group, slope) for h in range(H)]
            smax = max(float(ar.raw_score(self.graph, sv[:, h], se[:, h]).abs().max()) for h in range(H))
            self._ref64[key] = (torch.stack(cols, 1), smax)
        return self._ref64[key]


_CASES = {}


@pytest.fixture
def case(hg):
    def get(name):
        if name not in _CASES:
            _CASES[name] = Case(hg, SHAPES[name](), name)  # all five are tiny: they stay
        return _CASES[name]
    return get


def _scale(pd):
    return float(dr.scale(pd))


def _masked(keep, x, pd):
    return torch.where(keep, x * _scale(pd), torch.zeros_like(x))


def test_shapes_reach_every_path(case):
    widths = set()
    for name in SHAPES:
        c = case(name)
        for side in ar.GROUPS:
            widths.add(c.plan.segment_info(side)["width"])
    assert widths == {4, 8, 16}, widths
    info = case("sizes").plan.segment_info("hyperedge")
    assert {w * info["keep"] + d for w in (4, 8, 16) for d in (-1, 0, 1)} <= set(range(71))
    for name, side in (("long", "hyperedge"), ("long_T", "vertex")):
        c = case(name)
        info = c.plan.segment_info(side)
        assert len(info["long_rows"]) == 4 and info["long"] == 128 and 256 * info["keep"] == 1024, (name, info)
        assert {127, 128, 129, 1023, 1024, 1025} <= set(int(x) for x in ar.side_lengths(c.inc, side))


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forward_bits(case, shape, H):
    """a, b, c."""
    c = case(shape)
    sv, se = c.hsv[H], c.hse[H]
    for pd in PDS:
        keep = c.keep(pd, H)
        zero_patterns = []
        for group in ar.GROUPS:
            for slope in ar.SLOPES:
                what = "%s H %d %s p %g slope %g" % (shape, H, group, pd, slope)
                plain = c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope, heads=H)
                alpha, drop = c.plan.incidence_attention_dropout(c.ptr, c.ind, sv, se, group, slope, pd, c.rng, heads=H)
                torch.cuda.synchronize()
                assert alpha.shape == plain.shape == drop.shape
                assert torch.equal(_bits(alpha), _bits(plain)), "alpha differs from the plain softmax: " + what
                assert torch.equal(_bits(drop), _bits(_masked(keep, plain, pd))), "dropped coefficients: " + what
                assert bool((_bits(drop)[~keep] == 0).all()), "a dropped entry is not +0.0: " + what
                assert bool((drop[keep] > 0).all()), what
                zero_patterns.append(drop == 0)
        for z in zero_patterns[1:]:
            assert torch.equal(z, zero_patterns[0]), "the mask depends on the group: %s H %d p %g" % (shape, H, pd)
        assert torch.equal(zero_patterns[0], ~keep)


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_backward_bits(case, shape, H):
    """d."""
    c = case(shape)
    sv, se, dout = c.hsv[H], c.hse[H], c.hdout[H]
    for pd in PDS:
        keep = c.keep(pd, H)
        dalpha = _masked(keep, dout, pd)
        for group in ar.GROUPS:
            for slope in ar.SLOPES:
                what = "%s H %d %s p %g slope %g" % (shape, H, group, pd, slope)
                alpha = c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope, heads=H)
                want = c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, dalpha, sv, se, group, slope, heads=H)
                got = c.plan.incidence_attention_dropout_backward(c.ptr, c.ind, alpha, dout, sv, se, group, slope, pd, c.rng,
                                                                  heads=H)
                torch.cuda.synchronize()
                for name, g, w in zip(("ds", "dsv", "dse"), got, want):
                    assert g.shape == w.shape and torch.equal(_bits(g), _bits(w)), name + ": " + what
        # ds alone: neither sum asked for
        alpha = c.plan.incidence_attention(c.ptr, c.ind, sv, se, "vertex", 1.0, heads=H)
        full = c.plan.incidence_attention_dropout_backward(c.ptr, c.ind, alpha, dout, sv, se, "vertex", 1.0, pd, c.rng, heads=H)
        only = c.plan.incidence_attention_dropout_backward(c.ptr, c.ind, alpha, dout, sv, se, "vertex", 1.0, pd, c.rng,
                                                           need_sv=False, need_se=False, heads=H)
        assert only[1] is None and only[2] is None and torch.equal(_bits(only[0]), _bits(full[0]))


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_autograd_against_float64(hg, case, shape, H):
    """e."""
    c = case(shape)
    D = {"dsv": c.L["vertex"], "dse": c.L["hyperedge"]}
    for pd in PDS:
        scale = _scale(pd)
        keep = c.keep(pd, H).cpu().reshape(-1, H)
        dout64 = gr.f64(c.hdout[H]).reshape(-1, H)
        for group in ar.GROUPS:
            for slope in ar.SLOPES:
                what = "%s H %d %s p %g slope %g" % (shape, H, group, pd, slope)
                alpha64, smax = c.ref64(H, group, slope)
                assert smax <= 8.0
                cc = (c.L[group] + 16 + 16 * smax) * U
                leaves = [t.clone().requires_grad_(True) for t in (c.hsv[H], c.hse[H])]
                out = hg.ops.incidence_softmax(c.ptr, c.ind, leaves[0], leaves[1], group=group, negative_slope=slope,
                                               num_nodes=c.inc.N, heads=H, dropout=pd, rng_state=c.rng)
                got = dict(zip(("dsv", "dse"), torch.autograd.grad(out, leaves, c.hdout[H])))
                torch.cuda.synchronize()
                want_out = torch.where(keep, alpha64 / (1.0 - pd), torch.zeros_like(alpha64))
                err = (gr.f64(out).reshape(-1, H) - want_out).abs()
                print("%s: out max |err| / (scale alpha) %.3g (bound %.3g)" % (
                    what, float((err / (scale * alpha64)).max()) if err.numel() else 0.0, cc))
                assert bool(torch.isfinite(out).all()) and bool((err <= scale * cc * alpha64).all()), what
                for h in range(H):
                    sv, se = gr.f64(c.hsv[H]).reshape(-1, H)[:, h], gr.f64(c.hse[H]).reshape(-1, H)[:, h]
                    masked = torch.where(keep[:, h], dout64[:, h], torch.zeros_like(dout64[:, h]))
                    _, dsv, dse = ar.closed_form_backward(c.graph, sv, se, group, slope, alpha64[:, h], masked / (1.0 - pd))
                    _, mv, me = ar.backward_masses(c.graph, group, slope, alpha64[:, h], masked)
                    for name, ref, mass in (("dsv", dsv, mv), ("dse", dse, me)):
                        bound = scale * (2 * cc + (c.L[group] + D[name] + 8) * U)
                        g = gr.f64(got[name]).reshape(-1, H)[:, h]
                        e = float(((g - ref).abs() / mass.clamp(min=gr.TINY)).max()) if ref.numel() else 0.0
                        print("%s head %d %s: max |err| / mass %.3g (bound %.3g)" % (what, h, name, e, bound))
                        gr.assert_within(g, ref, mass, bound, "%s head %d %s" % (what, h, name))


@pytest.mark.parametrize("H", HEADS)
def test_no_dropout_is_todays_call(hg, case, H):
    """f."""
    c = case("ragged")
    sv, se = c.hsv[H], c.hse[H]
    kw = dict(group="vertex", negative_slope=0.2, num_nodes=c.inc.N, heads=H)
    today = hg.ops.incidence_softmax(c.ptr, c.ind, sv, se, **kw)
    torch.cuda.synchronize()
    state = torch.cuda.get_rng_state()
    for extra in (dict(dropout=0.0), dict(dropout=0.5, training=False), dict(dropout=0.0, training=False, rng_state=c.rng)):
        got, used = hg.ops.incidence_softmax(c.ptr, c.ind, sv, se, return_rng_state=True, **kw, **extra)
        leaves = [t.clone().requires_grad_(True) for t in (sv, se)]
        tracked = hg.ops.incidence_softmax(c.ptr, c.ind, leaves[0], leaves[1], **kw, **extra)
        torch.cuda.synchronize()
        assert used is None and torch.equal(_bits(got), _bits(today)) and torch.equal(_bits(tracked.detach()), _bits(today))
        assert type(tracked.grad_fn).__name__.startswith("_IncidenceSoftmaxBackward"), type(tracked.grad_fn)
    assert torch.equal(torch.cuda.get_rng_state(), state), "torch's generator moved without dropout"


def test_drawn_state(hg, case):
    """g."""
    c = case("ragged")
    kw = dict(group="hyperedge", num_nodes=c.inc.N, heads=3, dropout=0.5, return_rng_state=True)

    def call():
        return hg.ops.incidence_softmax(c.ptr, c.ind, c.hsv[3], c.hse[3], **kw)
    (a, ra), (b, rb) = call(), call()
    assert ra.dtype == torch.int64 and ra.numel() == 2 and ra.device == a.device
    assert not torch.equal(ra, rb) and not torch.equal(_bits(a), _bits(b))
    torch.manual_seed(7)
    a, ra = call()
    torch.manual_seed(7)
    b, rb = call()
    assert torch.equal(ra, rb) and torch.equal(_bits(a), _bits(b))
    plain = c.plan.incidence_attention(c.ptr, c.ind, c.hsv[3], c.hse[3], "hyperedge", 0.2, heads=3)
    assert torch.equal(_bits(a), _bits(_masked(c.keep(0.5, 3, rng=ra), plain, 0.5)))


@pytest.mark.parametrize("H", HEADS)
def test_layer(hg, case, H):
    """h."""
    c = case("ragged")
    F_in, C = 12, 4
    torch.manual_seed(5)
    X = torch.rand(c.inc.N, F_in, device=DEV)
    layer = hg.HypergraphAttnConv(c.h, F_in, C, group="hyperedge", heads=H, dropout=0.5).to(DEV)
    plain = hg.HypergraphAttnConv(c.h, F_in, C, group="hyperedge", heads=H, dropout=0.0).to(DEV)
    assert set(layer.state_dict()) == set(plain.state_dict()) == {"lin.weight", "a_v", "a_e", "bias"}
    plain.load_state_dict(layer.state_dict())
    layer.eval()
    assert torch.equal(_bits(layer(X).detach()), _bits(plain.train()(X).detach()))
    assert torch.equal(_bits(layer(X).detach()), _bits(plain.eval()(X).detach()))
    layer.train()
    torch.manual_seed(11)
    y1 = layer(X)
    y2 = layer(X)
    torch.manual_seed(11)
    y3 = layer(X)
    assert torch.equal(_bits(y1.detach()), _bits(y3.detach())), "not reproducible under torch.manual_seed"
    assert not torch.equal(_bits(y1.detach()), _bits(y2.detach())), "two consecutive calls drew the same mask"
    y1.square().sum().backward()
    for name, p in layer.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), name


def test_captured_step_draws_a_new_mask_per_replay(hg, case):
    """i: forward and backward in one graph; the state is drawn inside it, so every replay draws again."""
    c = case("ragged")
    H, pd = 3, 0.5
    sv, se = (t.clone().requires_grad_(True) for t in (c.hsv[H], c.hse[H]))
    dout = c.hdout[H]
    res = {}

    def step():
        out, rng = hg.ops.incidence_softmax(c.ptr, c.ind, sv, se, group="vertex", num_nodes=c.inc.N, heads=H, dropout=pd,
                                            return_rng_state=True)
        res["out"], res["rng"] = out, rng
        res["dsv"], res["dse"] = torch.autograd.grad(out, (sv, se), dout)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up: the first call builds and uploads the permutation and the long-row lists
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    plain = c.plan.incidence_attention(c.ptr, c.ind, c.hsv[H], c.hse[H], "vertex", 0.2, heads=H)
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        rng = res["rng"].clone()
        keep = c.keep(pd, H, rng=rng)
        assert torch.equal(_bits(res["out"].detach()), _bits(_masked(keep, plain, pd)))
        want = c.plan.incidence_attention_backward(c.ptr, c.ind, plain, _masked(keep, dout, pd), c.hsv[H], c.hse[H], "vertex",
                                                   0.2, heads=H)
        assert torch.equal(_bits(res["dsv"]), _bits(want[1])) and torch.equal(_bits(res["dse"]), _bits(want[2]))
        seen.append((rng, res["out"].detach().clone()))
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(_bits(seen[0][1]), _bits(seen[1][1]))


def test_refused_inputs(hg, case):
    c = case("toy")
    from hypergef_amd import _lib
    args = (c.ptr, c.ind, c.sv, c.se, "hyperedge", 0.2)
    for pd in (-0.1, 1.0, float("nan")):
        with pytest.raises(_lib.HgError) as e:
            c.plan.incidence_attention_dropout(*args, pd, c.rng)
        assert e.value.status == _lib.HG_ERR_INVALID and "p_drop" in str(e.value)
    with pytest.raises(TypeError):
        c.plan.incidence_attention_dropout(*args, 0.5, c.rng.to(torch.float32))
    with pytest.raises(ValueError):
        c.plan.incidence_attention_dropout(*args, 0.5, torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        c.plan.incidence_attention_dropout(*args, 0.5, c.rng.cpu())
    with pytest.raises(RuntimeError):
        hg.ops.incidence_softmax(c.ptr, c.ind, c.sv, c.se, dropout=0.5, rng_state=c.rng.cpu())
    L = _lib.lib()
    import ctypes
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    out = torch.empty(c.inc.nnz, device=DEV)
    null = ctypes.c_void_p(0)
    for rng, a, b in ((null, p(out), p(out)), (p(c.rng), null, p(out)), (p(c.rng), p(out), null),
                      (ctypes.c_void_p(c.rng.data_ptr() + 4), p(out), p(out))):
        rc = L.hg_incidence_attention_dropout_heads_f32(c.plan._h, 0, 1, p(c.ptr), p(c.ind), p(c.sv), p(c.se), 0.2, 0.5, rng, a, b,
                                                        null)
        assert rc == _lib.HG_ERR_INVALID
    rc = L.hg_incidence_attention_dropout_heads_bwd_f32(c.plan._h, 0, 1, p(c.ptr), p(c.ind), p(c.sv), p(c.se), 0.2, 0.5, p(c.rng),
                                                        p(out), p(out), null, null, null, null)
    assert rc == _lib.HG_ERR_INVALID
    rc = L.hg_incidence_attention_dropout_heads_f32(c.plan._h, 0, 0, p(c.ptr), p(c.ind), p(c.sv), p(c.se), 0.2, 0.5, p(c.rng),
                                                    p(out), p(out), null)
    assert rc == _lib.HG_ERR_INVALID
