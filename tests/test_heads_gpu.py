"""The multi-head incidence path on the GPU (the *_heads_f32 entries, heads=H of Plan / ops, HypergraphAttnConv(heads)).

Shapes: the toy graph; `ragged` (10 % empty hyperedges); `boundaries` and its transpose (a group of every length 0 .. 70,
around 128 / 256 / 1024, 5000, so both sides cross every threshold of the segment kernels); `widths_4 / 8 / 16` (the hyperedge
side at each lane-group width); `powerlaw(50_000, 200_000)` (wave tasks, two fixup levels, long segments on both sides).
(H, C): (1, 32); (2, 6), (4, 3), (8, 5) -- C % 4 != 0, the first two with F % 4 == 0, where a 16-byte lane would mix heads;
(4, 8), (8, 16); (3, 4); (8, 40) -- F = 320, two column tiles, head 6 straddles column 256; (16, 4).

Exact checks.  heads = 1 through every new entry has the bits of the existing entry.  Column h of the softmax, its backward
and the sum has the bits of the single-head call on the contiguous column h.  Head h's columns of Y and xe_out have the bits of
the single-head call of the same F weighted by column h.  Weights that are powers of two scale the unweighted pull exactly.
Integer-valued operands give the dot's float64 answer.  Two calls agree; guard words (SENTINEL) around outputs stay.
Float64 checks, bounds of the single-head tests per head (U = 2^-24): alpha (L + 16 + 16 Smax) U relative; ds / dsv / dse
2 c + (L + D + 8) U of the mass; the sum (D + 2) U of sum |val|; Y, dX FP32_C of the mass; the dot and the weight gradients
FP32_C + (C + 1) U of the mass; the layer test_attention_gpu.test_layer_against_float64's composed bound.
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

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV, U, SENTINEL, SLOPES = ar.DEV, ar.U, ar.SENTINEL, ar.SLOPES
GUARD = 64  # floats: 256 bytes, so a guarded output keeps its 16-byte alignment
_bits = ar.bits

SHAPES = {
    "toy": ar.toy,
    "ragged": lambda: synth.random_incidence(3000, 2000, 6.0, seed=4, empty_frac=0.1),
    "boundaries": ar.boundaries,
    "boundaries_T": lambda: ar.transpose(ar.boundaries()),
    "widths_4": lambda: ar.width_shape(4),
    "widths_8": lambda: ar.width_shape(8),
    "widths_16": lambda: ar.width_shape(16),
    "powerlaw": lambda: synth.powerlaw(50_000, 200_000),
}
PAIRS = [(1, 32), (2, 6), (4, 3), (8, 5), (4, 8), (8, 16), (3, 4), (8, 40), (16, 4)]
HEADS = sorted({h for h, _ in PAIRS})

_CASES = {}


@pytest.fixture
def case(hg):
    def get(name):
        if name not in _CASES:
            _CASES.clear()  # one shape at a time on the device
            torch.cuda.empty_cache()
            _CASES[name] = ar.Case(hg, SHAPES[name](), name)
        return _CASES[name]
    return get


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(*shape, seed):
    return torch.randn(*shape, device=DEV, generator=_gen(seed))


def _guarded(*shape):
    """(buffer, view): a SENTINEL-filled buffer and the output inside it, GUARD words on either side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _scores(c, H, seed=31):
    """sv [N, H], se [M, H] with max |.| = 4 per array (max |raw| <= 8)."""
    sv, se = _randn(c.inc.N, H, seed=seed), _randn(c.inc.M, H, seed=seed + 1)
    return sv * (4.0 / float(sv.abs().max())), se * (4.0 / float(se.abs().max()))


def _col(t, h):
    return None if t is None else t[:, h].contiguous()


def test_shapes_reach_every_path(case):
    c = case("powerlaw")
    assert (np.diff(c.inc.csrptr) > 512).sum() > 0 and (np.bincount(c.inc.colind, minlength=c.inc.N) > 512).sum() > 0
    for side in ar.GROUPS:
        assert len(c.plan.segment_info(side)["long_rows"]) > 0, side
    for name, side in (("boundaries", "hyperedge"), ("boundaries_T", "vertex")):
        c = case(name)
        assert ar.reaches_every_path(c.plan.segment_info(side), ar.side_lengths(c.inc, side)) is None
    for w in (4, 8, 16):
        assert case("widths_%d" % w).plan.segment_info("hyperedge")["width"] == w


def test_one_head_through_the_new_entries_is_the_existing_entry(hg, case):
    from hypergef_amd import _lib
    from hypergef_amd.plan import _ptr, _stream_handle
    L = _lib.lib()
    c = case("ragged")
    N, M, nnz, F = c.inc.N, c.inc.M, c.inc.nnz, 32
    st = _stream_handle(torch.device(DEV))
    for group in (0, 1):
        for slope in SLOPES:
            want = c.plan.incidence_attention(c.ptr, c.ind, c.sv, c.se, group, slope)
            got = torch.empty(nnz, device=DEV)
            _lib.check(L.hg_incidence_attention_heads_f32(c.plan._h, group, 1, _ptr(c.ptr), _ptr(c.ind), _ptr(c.sv), _ptr(c.se),
                                                          slope, _ptr(got), st))
            assert torch.equal(_bits(got), _bits(want))
            wds, wdv, wde = c.plan.incidence_attention_backward(c.ptr, c.ind, want, c.dalpha, c.sv, c.se, group, slope)
            ds, dv, de = torch.empty(nnz, device=DEV), torch.empty(N, device=DEV), torch.empty(M, device=DEV)
            _lib.check(L.hg_incidence_attention_heads_bwd_f32(c.plan._h, group, 1, _ptr(c.ptr), _ptr(c.ind), _ptr(c.sv),
                                                              _ptr(c.se), slope, _ptr(want), _ptr(c.dalpha), _ptr(ds), _ptr(dv),
                                                              _ptr(de), st))
            for a, b in ((ds, wds), (dv, wdv), (de, wde)):
                assert torch.equal(_bits(a), _bits(b))
        want = c.plan.incidence_sum(c.ptr, c.ind, c.val, group)
        got = torch.empty_like(want)
        _lib.check(L.hg_incidence_sum_heads_f32(c.plan._h, group, 1, _ptr(c.ptr), _ptr(c.ind), _ptr(c.val), _ptr(got), st))
        assert torch.equal(_bits(got), _bits(want))
    X, A, B = _randn(N, F, seed=1), _randn(N, F, seed=2), _randn(M, F, seed=3)
    alpha = c.plan.incidence_attention(c.ptr, c.ind, c.sv, c.se, 0, 0.2)
    wxe = torch.empty(M, F, device=DEV)
    want = c.plan.aggregate_incidence(c.ptr, c.ind, X, alpha, alpha, c.h.degE.reshape(-1), c.h.degV.reshape(-1), None, xe_out=wxe)
    got, xe = torch.empty(N, F, device=DEV), torch.empty(M, F, device=DEV)
    nbytes = c.plan.incidence_workspace_bytes(F)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
    _lib.check(L.hg_aggr_incidence_heads_f32(c.plan._h, F, 1, _ptr(c.ptr), _ptr(c.ind), _ptr(X), _ptr(alpha), _ptr(alpha),
                                             _ptr(c.h.degE), _ptr(c.h.degV), None, _ptr(xe), _ptr(got), _ptr(ws), nbytes, st))
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(xe), _bits(wxe))
    want = c.plan.incidence_dot(c.ptr, c.ind, A, B)
    got = torch.empty(nnz, device=DEV)
    _lib.check(L.hg_incidence_dot_heads_f32(c.plan._h, F, 1, _ptr(c.ptr), _ptr(c.ind), _ptr(A), _ptr(B), _ptr(got), st))
    assert torch.equal(_bits(got), _bits(want))
    # Plan and ops with heads=1: today's shapes
    assert c.plan.incidence_attention(c.ptr, c.ind, c.sv.view(N, 1), c.se, heads=1).shape == (nnz,)
    assert hg.ops.incidence_softmax(c.ptr, c.ind, c.sv.view(N, 1), c.se.view(M, 1), heads=1).shape == (nnz,)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_segment_columns_equal_the_single_head_calls(case, shape):
    c = case(shape)
    N, M, nnz = c.inc.N, c.inc.M, c.inc.nnz
    for H in HEADS[1:]:
        sv, se = _scores(c, H)
        dalpha, val = _randn(nnz, H, seed=41), _randn(nnz, H, seed=42)
        modes = ("both", "sv", "se") if H == 3 else ("both",)
        for group in ar.GROUPS:
            nout = M if group == "hyperedge" else N
            buf, out = _guarded(nout, H)
            c.plan.incidence_sum(c.ptr, c.ind, val, group, out=out, heads=H)
            again = c.plan.incidence_sum(c.ptr, c.ind, val, group, heads=H)
            assert torch.equal(_bits(out), _bits(again)) and _guards_intact(buf) and not bool((out == SENTINEL).any())
            for h in range(H):
                assert torch.equal(_bits(out[:, h]), _bits(c.plan.incidence_sum(c.ptr, c.ind, _col(val, h), group))), (H, h, group)
            for slope in SLOPES:
                for mode in modes:
                    a, b = (sv if mode != "se" else None), (se if mode != "sv" else None)
                    what = "%s H %d %s %s slope %g" % (shape, H, group, mode, slope)
                    buf, alpha = _guarded(nnz, H)
                    c.plan.incidence_attention(c.ptr, c.ind, a, b, group, slope, out=alpha, heads=H)
                    again = c.plan.incidence_attention(c.ptr, c.ind, a, b, group, slope, heads=H)
                    assert torch.equal(_bits(alpha), _bits(again)), "two calls differ: " + what
                    assert _guards_intact(buf) and not bool((alpha == SENTINEL).any()), what
                    combos = ((True, True), (True, False), (False, True), (False, False)) if mode == "both" else ((True, True),)
                    for need_sv, need_se in combos:
                        got = c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, dalpha, a, b, group, slope,
                                                                  need_sv=need_sv, need_se=need_se, heads=H)
                        assert got[0].shape == (nnz, H) and (got[1] is None) == (not need_sv) and (got[2] is None) == (not need_se)
                        for h in range(H):
                            one = c.plan.incidence_attention(c.ptr, c.ind, _col(a, h), _col(b, h), group, slope)
                            assert torch.equal(_bits(alpha[:, h]), _bits(one)), "alpha column %d: %s" % (h, what)
                            want = c.plan.incidence_attention_backward(c.ptr, c.ind, one, _col(dalpha, h), _col(a, h), _col(b, h),
                                                                       group, slope, need_sv=need_sv, need_se=need_se)
                            for name, g, w in zip(("ds", "dsv", "dse"), got, want):
                                assert (g is None) == (w is None)
                                if g is not None:
                                    assert torch.equal(_bits(g[:, h]), _bits(w)), "%s column %d: %s" % (name, h, what)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_constant_scores_and_counting_sums(case, shape):
    c = case(shape)
    H = 4
    N, M, nnz = c.inc.N, c.inc.M, c.inc.nnz
    sv, se = torch.full((N, H), 0.75, device=DEV), torch.full((M, H), -1.5, device=DEV)
    for group in ar.GROUPS:
        idx, sizes = c.sizes(group)
        alpha = c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, 0.2, heads=H).cpu()
        want = (torch.ones((), dtype=torch.float32) / sizes[idx].to(torch.float32))  # fl32(1 / L)
        assert torch.equal(alpha, want[:, None].expand(nnz, H)), (shape, group)
        ones = torch.ones(nnz, H, device=DEV) * torch.arange(1, H + 1, device=DEV, dtype=torch.float32)
        cnt = c.plan.incidence_sum(c.ptr, c.ind, ones, group, heads=H).cpu()
        assert torch.equal(cnt, sizes.to(torch.float32)[:, None] * torch.arange(1, H + 1, dtype=torch.float32)), (shape, group)


def _weights(c, H, seed):
    """Positive weights per incidence and head: a softmax's output, signed variety not needed for bit equality."""
    sv, se = _scores(c, H, seed)
    return (c.plan.incidence_attention(c.ptr, c.ind, sv, se, "hyperedge", 0.2, heads=H),
            c.plan.incidence_attention(c.ptr, c.ind, sv, se, "vertex", 0.2, heads=H))


@pytest.mark.parametrize("H,C", PAIRS[1:])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_aggregation_heads_equal_the_single_head_calls(case, shape, H, C):
    c = case(shape)
    N, M, nnz, F = c.inc.N, c.inc.M, c.inc.nnz, H * C
    X = _randn(N, F, seed=5)
    v2e, e2v = _weights(c, H, 51)
    degE, degV = c.h.degE.reshape(-1), c.h.degV.reshape(-1)
    W = torch.rand(M, device=DEV, generator=_gen(6)) + 0.5
    for wv, we, scales in ((v2e, e2v, (None, None, None)), (v2e, None, (degE, degV, W)), (None, e2v, (degE, degV, W)),
                           (v2e, e2v, (degE, degV, W))):
        what = "%s (%d, %d) v2e %s e2v %s scales %s" % (shape, H, C, wv is not None, we is not None, scales[0] is not None)
        ybuf, Y = _guarded(N, F)
        xbuf, Xe = _guarded(M, F)
        c.plan.aggregate_incidence(c.ptr, c.ind, X, wv, we, *scales, xe_out=Xe, out=Y, heads=H)
        again = c.plan.aggregate_incidence(c.ptr, c.ind, X, wv, we, *scales, heads=H)
        assert torch.equal(_bits(Y), _bits(again)), "two calls differ: " + what
        assert _guards_intact(ybuf) and _guards_intact(xbuf), what
        assert not bool((Y == SENTINEL).any()) and not bool((Xe == SENTINEL).any()), what
        for h in range(H):
            one_xe = torch.empty(M, F, device=DEV)
            one = c.plan.aggregate_incidence(c.ptr, c.ind, X, _col(wv, h), _col(we, h), *scales, xe_out=one_xe)
            cols = slice(h * C, (h + 1) * C)
            assert torch.equal(_bits(Y[:, cols]), _bits(one[:, cols])), "Y head %d: %s" % (h, what)
            assert torch.equal(_bits(Xe[:, cols]), _bits(one_xe[:, cols])), "xe_out head %d: %s" % (h, what)
    # powers of two, another per head: the unweighted pull, scaled exactly
    kv = torch.tensor([(h % 5) - 2 for h in range(H)], device=DEV, dtype=torch.float32)
    ke = torch.tensor([(h % 3) - 1 for h in range(H)], device=DEV, dtype=torch.float32)
    pv, pe = torch.ones(nnz, H, device=DEV) * torch.exp2(kv), torch.ones(nnz, H, device=DEV) * torch.exp2(ke)
    plain = c.plan.aggregate_incidence(c.ptr, c.ind, X, None, None, degE, degV, W)
    got = c.plan.aggregate_incidence(c.ptr, c.ind, X, pv, pe, degE, degV, W, heads=H)
    want = plain * torch.exp2(kv + ke).repeat_interleave(C)
    assert torch.equal(_bits(got), _bits(want)), "%s (%d, %d): power-of-two weights" % (shape, H, C)


@pytest.mark.parametrize("H,C", PAIRS[1:])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_dot_of_integers_is_exact(case, shape, H, C):
    c = case(shape)
    N, M, nnz, F = c.inc.N, c.inc.M, c.inc.nnz, H * C
    A = torch.randint(-4, 5, (N, F), device=DEV, generator=_gen(7)).float()
    B = torch.randint(-4, 5, (M, F), device=DEV, generator=_gen(8)).float()
    buf, out = _guarded(nnz, H)
    c.plan.incidence_dot(c.ptr, c.ind, A, B, out=out, heads=H)
    again = c.plan.incidence_dot(c.ptr, c.ind, A, B, heads=H)
    assert torch.equal(_bits(out), _bits(again)) and _guards_intact(buf) and again.shape == (nnz, H)
    V, E = c.graph.V.to(DEV), c.graph.E.to(DEV)
    want = (A[V].double() * B[E].double()).view(nnz, H, C).sum(2)  # |sum| <= 16 C: exact in fp32 and float64
    assert torch.equal(out.double(), want), "%s (%d, %d)" % (shape, H, C)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_coefficients_against_float64(case, shape):
    c = case(shape)
    H = 3
    sv, se = _scores(c, H)
    sv64, se64 = gr.f64(sv), gr.f64(se)
    dalpha, val = _randn(c.inc.nnz, H, seed=41), _randn(c.inc.nnz, H, seed=42)
    da = gr.f64(dalpha)
    for side in ar.GROUPS:
        got = c.plan.incidence_sum(c.ptr, c.ind, val, side, heads=H)
        gr.assert_within(got, hr.segment_sum(c.graph, gr.f64(val), side), hr.segment_sum(c.graph, gr.f64(val).abs(), side),
                         (c.L[side] + 2) * U, "%s incidence_sum %s" % (shape, side))
    for group in ar.GROUPS:
        idx, sizes = c.sizes(group)
        D = {"ds": 0, "dsv": c.L["vertex"], "dse": c.L["hyperedge"]}
        for slope in SLOPES:
            what = "%s %s slope %g" % (shape, group, slope)
            ref = hr.softmax(c.graph, sv64, se64, group, slope, H)
            smax = float(ar.raw_score(c.graph, sv64.abs().max(1).values, se64.abs().max(1).values).max()) if ref.numel() else 0.0
            assert smax <= 8.0
            cc = (c.L[group] + 16 + 16 * smax) * U
            alpha = c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope, heads=H)
            got = gr.f64(alpha)
            rel = float(((got - ref).abs() / ref).max()) if ref.numel() else 0.0
            print("%s: max |err| / alpha %.3g (bound %.3g)" % (what, rel, cc))
            assert bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= cc * ref).all()), what
            want = dict(zip(("ds", "dsv", "dse"), hr.closed_form_backward(c.graph, sv64, se64, group, slope, ref, da)))
            mass = dict(zip(("ds", "dsv", "dse"), hr.backward_masses(c.graph, group, slope, ref, da)))
            back = dict(zip(("ds", "dsv", "dse"), c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, dalpha, sv, se, group,
                                                                                      slope, heads=H)))
            for name in ("ds", "dsv", "dse"):
                gr.assert_within(back[name], want[name], mass[name], 2 * cc + (c.L[group] + D[name] + 8) * U, what + " " + name)
            # scores of magnitude 1e4: finite, every non-empty group sums to 1 in every head
            big = gr.f64(c.plan.incidence_attention(c.ptr, c.ind, sv * 2500.0, se * 2500.0, group, slope, heads=H))
            assert bool(torch.isfinite(big).all()), what
            sums = hr.segment_sum(c.graph, big, group)
            assert bool(((sums[sizes > 0] - 1.0).abs() <= (2 * c.L[group] + 16) * U).all()) and bool((sums[sizes == 0] == 0).all())


@pytest.mark.parametrize("shape,H,C", [("toy", 3, 4), ("ragged", 8, 40), ("ragged", 4, 3), ("boundaries", 2, 6),
                                       ("boundaries_T", 8, 5), ("powerlaw", 4, 3), ("powerlaw", 4, 8)])
def test_aggregation_and_gradients_against_float64(hg, case, shape, H, C):
    c = case(shape)
    N, M, nnz, F = c.inc.N, c.inc.M, c.inc.nnz, H * C
    X, dY = _randn(N, F, seed=5), _randn(N, F, seed=9)
    v2e, e2v = _weights(c, H, 51)
    degE, degV = c.h.degE.reshape(-1), c.h.degV.reshape(-1)
    leaves = [t.clone().requires_grad_(True) for t in (X, v2e, e2v)]
    Y = hg.ops.incidence_aggr(c.ptr, c.ind, leaves[0], leaves[1], leaves[2], degE, degV, None, heads=H)
    dX, dv, de = torch.autograd.grad(Y, leaves, dY)
    assert dv.shape == (nnz, H) and de.shape == (nnz, H)
    graph = gr.Graph(c.inc, degE, degV, None)
    out, grads, out_mass, grad_mass = gr.evaluate(hr.fn, graph, {"x": X, "v2e": v2e, "e2v": e2v, "heads": H}, dY,
                                                  ("x", "v2e", "e2v"))
    what = "%s (%d, %d)" % (shape, H, C)
    gr.assert_within(Y, out, out_mass, gr.FP32_C, what + " Y")
    gr.assert_within(dX, grads["x"], grad_mass["x"], gr.FP32_C, what + " dX")
    c_dot = gr.FP32_C + (C + 1) * U
    gr.assert_within(dv, grads["v2e"], grad_mass["v2e"], c_dot, what + " dv2e")
    gr.assert_within(de, grads["e2v"], grad_mass["e2v"], c_dot, what + " de2v")
    A, B = _randn(N, F, seed=2), _randn(M, F, seed=3)
    gr.assert_within(c.plan.incidence_dot(c.ptr, c.ind, A, B, heads=H), hr.dot(c.graph, A, B, H), hr.dot_mass(c.graph, A, B, H),
                     c_dot, what + " dot")


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("group", ar.GROUPS)
def test_layer_training_step_against_float64(hg, group, concat):
    """test_attention_gpu.test_layer_against_float64 with heads = 4 on the cora shape: non-negative X, parameters and dY,
    the masses from _heads_ref._MassSoftmax.  The bound is that test's, with F_out the linear's width H C (every score is a
    product over at most F_out terms), and for concat=False the mean's H - 1 additions and one product: (H + 1) U more."""
    inc = synth.cora_shape()
    h = hg.HyperGraph.from_incidence(inc, DEV, data_name="cora-heads", ngs=1 << 30)
    H, C, F_in, slope = 4, 8, 16, 0.2
    F_out, W_out = H * C, (H * C if concat else C)
    g = torch.Generator().manual_seed(9)
    X32, dY = torch.rand(inc.N, F_in, generator=g), torch.rand(inc.N, W_out, generator=g)
    params = {"lin.weight": torch.rand(F_out, F_in, generator=g) / F_in, "a_v": torch.rand(F_out, generator=g),
              "a_e": torch.rand(F_out, generator=g), "bias": torch.rand(W_out, generator=g)}
    layer = hg.HypergraphAttnConv(h, F_in, C, group=group, negative_slope=slope, heads=H, concat=concat).to(DEV)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            p.copy_(params[name])
    opt = torch.optim.SGD(layer.parameters(), lr=0.125)
    Y = layer(X32.to(DEV))
    assert Y.shape == (inc.N, W_out)
    Y.backward(dY.to(DEV))
    graph64 = gr.Graph(inc, h.degE.reshape(-1), h.degV.reshape(-1), None)

    def run64(mass):
        leaves = {k: v.double().requires_grad_(True) for k, v in params.items()}
        out = hr.attn_conv(graph64, X32.double(), leaves["lin.weight"], leaves["a_v"], leaves["a_e"], leaves["bias"], group,
                           slope, H, concat, mass=mass)
        return out.detach(), dict(zip(leaves, torch.autograd.grad(out, list(leaves.values()), dY.double())))
    Y64, ref = run64(False)
    _, mass = run64(True)
    zh = (X32.double() @ params["lin.weight"].double().t()).view(inc.N, H, C)
    smax = float(((zh * params["a_v"].double().view(H, C)).sum(-1).max(0).values
                  + (zh * params["a_e"].double().view(H, C)).sum(-1).max(0).values).max())
    Lh, Lv = ar.longest(inc, "hyperedge"), ar.longest(inc, "vertex")
    L = Lh if group == "hyperedge" else Lv
    c_alpha = (L + 16 + 16 * smax) * U
    cc = (3 * gr.FP32_C + (F_out + 1 + inc.nnz + F_in + 16) * U + 2 * smax * (F_in + F_out + Lh + 4) * U + 2 * c_alpha
          + 2 * c_alpha + (L + Lv + Lh + 8) * U + (0 if concat else (H + 1) * U))
    gr.assert_within(Y, Y64, Y64.abs(), cc, "layer out")
    before = {n: p.detach().clone() for n, p in layer.named_parameters()}
    opt.step()
    for name, p in layer.named_parameters():
        assert bool((mass[name] >= ref[name].abs() * (1 - 1e-12)).all())
        gr.assert_within(p.grad, ref[name], mass[name], cc, "layer d%s" % name)
        assert torch.equal(p.detach(), before[name] - 0.125 * p.grad), name  # the step itself: exact in fp32 (lr = 2^-3)


def test_refused_inputs_leave_outputs_untouched(hg, case):
    from hypergef_amd import _lib
    from hypergef_amd.plan import _ptr, _stream_handle
    L = _lib.lib()
    c = case("ragged")
    N, M, nnz, H, C = c.inc.N, c.inc.M, c.inc.nnz, 4, 3
    F = H * C
    st = _stream_handle(torch.device(DEV))
    X, w = _randn(N, F, seed=1), torch.rand(nnz, H, device=DEV, generator=_gen(2))
    sv, se = _scores(c, H)
    Y, Xe = torch.full((N, F), SENTINEL, device=DEV), torch.full((M, F), SENTINEL, device=DEV)
    out = torch.full((nnz, H), SENTINEL, device=DEV)
    seg = torch.full((M, H), SENTINEL, device=DEV)
    nbytes = c.plan.incidence_workspace_bytes(F)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
    for heads in (0, -1, 5, 8):  # 5 and 8 do not divide F = 12
        rc = L.hg_aggr_incidence_heads_f32(c.plan._h, F, heads, _ptr(c.ptr), _ptr(c.ind), _ptr(X), _ptr(w), _ptr(w), None, None,
                                           None, _ptr(Xe), _ptr(Y), _ptr(ws), nbytes, st)
        assert rc == _lib.HG_ERR_INVALID and b"heads" in L.hg_last_error(), heads
        rc = L.hg_incidence_dot_heads_f32(c.plan._h, F, heads, _ptr(c.ptr), _ptr(c.ind), _ptr(X), _ptr(Xe), _ptr(out), st)
        assert rc == _lib.HG_ERR_INVALID, heads
    for heads in (0, -1):
        assert L.hg_incidence_attention_heads_f32(c.plan._h, 0, heads, _ptr(c.ptr), _ptr(c.ind), _ptr(sv), _ptr(se), 0.2,
                                                  _ptr(out), st) == _lib.HG_ERR_INVALID
        assert L.hg_incidence_attention_heads_bwd_f32(c.plan._h, 0, heads, _ptr(c.ptr), _ptr(c.ind), _ptr(sv), _ptr(se), 0.2,
                                                      _ptr(w), _ptr(w), _ptr(out), None, _ptr(seg), st) == _lib.HG_ERR_INVALID
        assert L.hg_incidence_sum_heads_f32(c.plan._h, 0, heads, _ptr(c.ptr), _ptr(c.ind), _ptr(w), _ptr(seg), st) == _lib.HG_ERR_INVALID
    assert L.hg_incidence_attention_heads_f32(c.plan._h, 2, H, _ptr(c.ptr), _ptr(c.ind), _ptr(sv), _ptr(se), 0.2, _ptr(out),
                                              st) == _lib.HG_ERR_INVALID  # inherited: group not 0 / 1
    assert L.hg_incidence_attention_heads_f32(c.plan._h, 0, H, _ptr(c.ptr), _ptr(c.ind), _ptr(sv), _ptr(se), float("nan"),
                                              _ptr(out), st) == _lib.HG_ERR_INVALID  # inherited: non-finite slope
    assert L.hg_aggr_incidence_heads_f32(c.plan._h, F, H, _ptr(c.ptr), _ptr(c.ind), _ptr(X), _ptr(w), _ptr(w), None, None, None,
                                         _ptr(Xe), _ptr(Y), _ptr(ws), 0, st) == _lib.HG_ERR_WORKSPACE  # inherited
    with pytest.raises(ValueError, match="multiple of heads"):
        c.plan.aggregate_incidence(c.ptr, c.ind, X, w, w, xe_out=Xe, out=Y, heads=5)
    with pytest.raises(ValueError, match="elements"):
        c.plan.aggregate_incidence(c.ptr, c.ind, X, w[:, :2].contiguous(), None, xe_out=Xe, out=Y, heads=H)
    with pytest.raises(ValueError, match="elements"):
        c.plan.incidence_attention(c.ptr, c.ind, sv[:, :2].contiguous(), se, out=out, heads=H)
    with pytest.raises(ValueError, match="elements"):
        c.plan.incidence_sum(c.ptr, c.ind, w[:, :2].contiguous(), out=seg, heads=H)
    with pytest.raises(ValueError, match="multiple of heads"):
        c.plan.incidence_dot(c.ptr, c.ind, X, Xe, out=out, heads=5)
    with pytest.raises(ValueError):
        hg.ops.incidence_aggr(c.ptr, c.ind, X, w, w, heads=H, options=hg.ops.Options(variant="fused"))
    with pytest.raises(RuntimeError):
        hg.ops.incidence_softmax(c.ptr, c.ind, sv.cpu(), se, heads=H)
    torch.cuda.synchronize()
    for t in (Y, Xe, out, seg):
        assert bool((t == SENTINEL).all())
