"""The segment kernels of the attention coefficients (hg_incidence_attention_f32 / _bwd_f32, hg_incidence_sum_f32) with
every segment length at every lane-group width.  The launcher derives the width W of a side from the mean length of the
rows a lane group walks (seg_width), so a test reaches a width only through the shape it builds:

  widths_W (W = 4, 8, 16): the boundary rows of test_attention_gpu.py -- every length 0 .. 70, 255 .. 257, 1023 .. 1025,
  5000 and every threshold of the kernels +-1 -- then 3000 rows of 2, 6 or 12 members, which put the hyperedge side's mean
  at 2.85, 6.75 or 12.61; M = 3081 is no multiple of 256 / W.  widths_W_T, the transpose, puts the same lengths on the
  vertex side.  The side so designed is the point of each shape; the other side runs at W = 4 or 8 with short rows and
  must pass the same checks.
  Degenerate launches (exact checks only): `all_long`, whose every non-empty hyperedge is longer than a lane group takes
  (mean 0, W = 4, every lane group skips); M = 1 with one hyperedge of 1 and of 129 members; nnz = 0 with M > 0.
  `widths_4+dups`: widths_4 with 3 % of its incidences listed twice.

1. Exact checks, which a dropped or repeated entry cannot pass.  Constant scores (sv = 0.75, se = -1.25: every raw score
   of a segment is the same, every s - m is 0, every exponential is 1, and the sum is the length L <= 5000 < 2^24 in any
   order): alpha is fl32(1 / L) bit for bit.  Counting: the segment sum of ones is the length, and that of the H_T
   position mod 256 (integers, sums below 2^24) equals the int64 sum.  Two calls agree bit for bit; guard words around
   the outputs keep their sentinel and every real position loses it; one-entry groups are 1.0f.
2. Float64 comparison with random scores, the bounds derived in test_attention_gpu.py: alpha per element within
   c = (L + 16 + 16 Smax) U of itself; every non-empty group sums to 1 within (2 L + 16) U -- with L the longest group of
   the side and, since that derivation holds group by group and L = 5000 here would hide an error in a short row, again
   with L the entry's own group's length; ds, dsv, dse within
   (2 c + (L + D + 8) U) max(mass, TINY); incidence_sum within (D + 2) U of sum |val|.
3. The backward's paths.  The same alpha and dalpha at slope 1.0 (no score is gathered) and at slope 0.2: t, the
   segment's sum of alpha dalpha, does not depend on the slope, so ds(0.2) is ds(1.0) times leaky'(raw) = 1 or fl32(0.2),
   the sign of raw taken from the fp32 sum as the kernel forms it.  Both are products of the same three fp32 factors, each
   rounded at most twice: they agree within 4 U of the value whatever the order of the two multiplications.  And ds is
   bit-equal whether dsv / dse are requested or not (the segment's own sum must not perturb the entries), as are the sums
   that are requested.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402
import _grad_ref as gr  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = ar.DEV
U = ar.U
SENTINEL = ar.SENTINEL
SLOPES = ar.SLOPES
MODES = ar.MODES
GUARD = 64
WIDTHS = (4, 8, 16)


def _single(N, sizes, name):
    return synth._from_sizes(np.random.default_rng(5), N, sizes, name=name)


# name -> (builder, designed side or None, the width that side must run at)
WIDTH_SHAPES = {}
for _w in WIDTHS:
    WIDTH_SHAPES["widths_%d" % _w] = (lambda w=_w: ar.width_shape(w), "hyperedge", _w)
    WIDTH_SHAPES["widths_%d_T" % _w] = (lambda w=_w: ar.transpose(ar.width_shape(w)), "vertex", _w)
EXACT_ONLY = {
    "all_long": (lambda: _single(1100, [129, 0, 300, 1024], "all_long"), "hyperedge", 4),
    "one_of_1": (lambda: _single(3, [1], "one_of_1"), "hyperedge", 4),
    "one_of_129": (lambda: _single(200, [129], "one_of_129"), "hyperedge", 4),
    "no_entries": (lambda: synth.Incidence(7, 5, np.zeros(6, np.int32), np.zeros(0, np.int32), name="no_entries"),
                   "hyperedge", 4),
    "widths_4+dups": (lambda: ar.with_duplicates(ar.width_shape(4)), "hyperedge", 4),
}
SHAPES = dict(WIDTH_SHAPES, **EXACT_ONLY)

_CASES = {}


@pytest.fixture
def case(hg):
    def get(name):
        if name not in _CASES:
            _CASES.clear()  # one shape at a time on the device
            _CASES[name] = ar.Case(hg, SHAPES[name][0](), name)
        return _CASES[name]
    return get


EXACT_CELLS = [(s, g) for s in SHAPES for g in ar.GROUPS]
WIDTH_CELLS = [(s, g) for s in WIDTH_SHAPES for g in ar.GROUPS]


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_kept(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def test_shapes_reach_every_width(case):
    for name, (_, side, width) in SHAPES.items():
        c = case(name)
        info = c.plan.segment_info(side)
        lens = ar.side_lengths(c.inc, side)
        other = ar.GROUPS[1 - ar.GROUPS.index(side)]
        print("%s: %s side W %d, longest %d, %d long rows; %s side W %d, longest %d" % (
            name, side, info["width"], lens.max(), len(info["long_rows"]), other, c.plan.segment_info(other)["width"],
            c.L[other]))
        assert info["width"] == width, (name, side, info)
        if name in WIDTH_SHAPES:
            assert ar.reaches_every_path(info, lens) is None, (name, ar.reaches_every_path(info, lens))
            assert lens.size % (256 // width) != 0 and c.inc.nnz <= 48_000, name
    c = case("all_long")
    info = c.plan.segment_info("hyperedge")
    np.testing.assert_array_equal(info["long_rows"], [0, 2, 3])  # every non-empty row: the lane groups all skip
    dup = case("widths_4+dups")
    assert (np.diff(dup.inc.colind) == 0).sum() > 0.02 * ar.width_shape(4).nnz  # a repeated member follows its first listing


@pytest.mark.parametrize("shape,group", EXACT_CELLS)
def test_constant_scores_give_the_exact_reciprocal(case, shape, group):
    c = case(shape)
    idx, sizes = c.sizes(group)
    want = (torch.ones((), dtype=torch.float32) / sizes.to(torch.float32))[idx]  # fl32(1 / L) of every entry's group
    sv = torch.full((c.inc.N,), 0.75, device=DEV)
    se = torch.full((c.inc.M,), -1.25, device=DEV)
    for mode in MODES:
        for slope in SLOPES:
            got = c.plan.incidence_attention(c.ptr, c.ind, sv if mode != "se" else None, se if mode != "sv" else None,
                                             group, slope).cpu()
            bad = torch.nonzero(ar.bits(got) != ar.bits(want)).reshape(-1)
            assert bad.numel() == 0, "%s %s %s slope %g: %d entries are not fl32(1 / L), in groups of %s entries" % (
                shape, group, mode, slope, bad.numel(), sorted(set(sizes[idx][bad].tolist()))[:12])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_counting(case, shape):
    c = case(shape)
    nnz = c.inc.nnz
    ones = torch.ones(nnz, device=DEV)
    pos = torch.arange(nnz, dtype=torch.int64) % 256
    for side in ar.GROUPS:
        idx, sizes = c.sizes(side)
        n = sizes.numel()
        buf, out = _guarded(n)
        c.plan.incidence_sum(c.ptr, c.ind, ones, side, out=out)
        torch.cuda.synchronize()
        assert _guards_kept(buf, n) and not bool((out == SENTINEL).any()), (shape, side)
        got = out.cpu()
        bad = torch.nonzero(got != sizes.to(torch.float32)).reshape(-1)
        assert bad.numel() == 0, "%s %s: the sum of ones is not the length in %d rows, e.g. row %d: %g of %d" % (
            shape, side, bad.numel(), int(bad[0]), float(got[bad[0]]), int(sizes[bad[0]]))
        want = torch.zeros(n, dtype=torch.int64).index_add_(0, idx, pos)
        assert int(want.max()) < 1 << 24
        got = c.plan.incidence_sum(c.ptr, c.ind, pos.to(torch.float32).to(DEV), side)
        again = c.plan.incidence_sum(c.ptr, c.ind, pos.to(torch.float32).to(DEV), side)
        assert torch.equal(ar.bits(got), ar.bits(again)), (shape, side)
        bad = torch.nonzero(got.cpu().to(torch.float64) != want.to(torch.float64)).reshape(-1)
        assert bad.numel() == 0, "%s %s: %d rows sum other positions than their own, e.g. row %d of %d entries" % (
            shape, side, bad.numel(), int(bad[0]), int(sizes[bad[0]]))


@pytest.mark.parametrize("shape,group", EXACT_CELLS)
def test_determinism_and_exact_facts(case, shape, group):
    c = case(shape)
    nnz = c.inc.nnz
    idx, sizes = c.sizes(group)
    for mode in MODES:
        sv, se = c.scores(mode)
        for slope in SLOPES:
            buf, out = _guarded(nnz)
            c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope, out=out)
            again = c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope)
            torch.cuda.synchronize()
            what = "%s %s %s slope %g" % (shape, group, mode, slope)
            assert torch.equal(ar.bits(out), ar.bits(again)), "two calls differ: " + what
            assert _guards_kept(buf, nnz), what
            assert not bool((out == SENTINEL).any()), "a real position was not written: " + what
            ones = out.cpu()[sizes[idx] == 1]
            assert bool((ones == 1.0).all()), "one-entry groups are not exactly 1.0f: " + what
            first = c.plan.incidence_attention_backward(c.ptr, c.ind, out, c.dalpha, sv, se, group, slope)
            second = c.plan.incidence_attention_backward(c.ptr, c.ind, out, c.dalpha, sv, se, group, slope)
            for name, a, b in zip(("ds", "dsv", "dse"), first, second):
                assert torch.equal(ar.bits(a), ar.bits(b)), "two backward calls differ in %s: %s" % (name, what)


@pytest.mark.parametrize("shape,group", WIDTH_CELLS)
def test_alpha_against_float64(case, shape, group):
    c = case(shape)
    idx, sizes = c.sizes(group)
    L = c.L[group]
    worst = worst_own = 0.0
    for mode in MODES:
        sv, se = c.scores(mode)
        for slope in SLOPES:
            ref, smax = c.ref(mode, group, slope)
            cc = c.c(mode, group, slope)
            assert smax <= 8.0
            got = gr.f64(c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope))
            rel = (got - ref).abs() / ref
            own = (sizes[idx] + 16 + 16 * smax).to(torch.float64) * U  # the same bound with the entry's own group's length
            dev = (ar.segment_sum(c.graph, got, group) - 1.0).abs()
            worst = max(worst, float(rel.max()) / cc)
            worst_own = max(worst_own, float((rel / own).max()))
            print("%s %s %s slope %g: max |err| / alpha %.3g (bound %.3g, L %d, Smax %.2f); max |sum - 1| %.3g (bound %.3g)"
                  % (shape, group, mode, slope, float(rel.max()), cc, L, smax, float(dev[sizes > 0].max()), (2 * L + 16) * U))
            what = (shape, group, mode, slope)
            assert bool(torch.isfinite(got).all()) and bool((rel <= cc).all()), what
            assert bool((rel <= own).all()), what
            assert bool((dev[sizes > 0] <= (2 * L + 16) * U).all()), what
            assert bool((dev[sizes > 0] <= (2 * sizes[sizes > 0] + 16).to(torch.float64) * U).all()), what
    print("%s %s: worst alpha error / bound %.3g, / the bound with the group's own length %.3g" % (
        shape, group, worst, worst_own))


@pytest.mark.parametrize("shape,group", WIDTH_CELLS)
def test_gradients_against_float64(case, shape, group):
    c = case(shape)
    names = ("ds", "dsv", "dse")
    D = {"ds": 0, "dsv": c.L["vertex"], "dse": c.L["hyperedge"]}
    da = gr.f64(c.dalpha)
    worst = dict.fromkeys(names, 0.0)
    for mode in MODES:
        sv, se = c.scores(mode)
        for slope in SLOPES:
            ref_alpha, _ = c.ref(mode, group, slope)
            cc = c.c(mode, group, slope)
            want = dict(zip(names, ar.closed_form_backward(c.graph, gr.f64(sv), gr.f64(se), group, slope, ref_alpha, da)))
            mass = dict(zip(names, ar.backward_masses(c.graph, group, slope, ref_alpha, da)))
            alpha = c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope)
            got = dict(zip(names, c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, c.dalpha, sv, se, group, slope)))
            what = "%s %s %s slope %g" % (shape, group, mode, slope)
            for name in names:
                bound = 2 * cc + (c.L[group] + D[name] + 8) * U
                err = float(((gr.f64(got[name]) - want[name]).abs() / mass[name].clamp(min=gr.TINY)).max())
                worst[name] = max(worst[name], err / bound)
                print("%s %s: max |err| / mass %.3g (bound %.3g)" % (what, name, err, bound))
                gr.assert_within(got[name], want[name], mass[name], bound, what + " " + name)
    print("%s %s: worst gradient error / bound %s" % (shape, group, ", ".join("%s %.3g" % kv for kv in worst.items())))


@pytest.mark.parametrize("shape", list(WIDTH_SHAPES))
def test_incidence_sum_against_float64(case, shape):
    c = case(shape)
    for side in ar.GROUPS:
        got = c.plan.incidence_sum(c.ptr, c.ind, c.val, side)
        want = ar.segment_sum(c.graph, gr.f64(c.val), side)
        mass = ar.segment_sum(c.graph, gr.f64(c.val).abs(), side)
        bound = (c.L[side] + 2) * U
        err = float(((gr.f64(got) - want).abs() / mass.clamp(min=gr.TINY)).max())
        print("%s incidence_sum %s: max |err| / sum|val| %.3g (bound %.3g), error / bound %.3g" % (
            shape, side, err, bound, err / bound))
        gr.assert_within(got, want, mass, bound, "%s incidence_sum %s" % (shape, side))


@pytest.mark.parametrize("shape,group", WIDTH_CELLS)
def test_backward_with_and_without_the_raw_score(case, shape, group):
    c = case(shape)
    slope32 = torch.tensor(0.2, dtype=torch.float32)
    for mode in MODES:  # the group's own score is absent in one mode and present in two
        sv, se = c.scores(mode)
        raw32 = torch.zeros(c.inc.nnz, dtype=torch.float32)  # the fp32 sum, as the kernel forms it
        if sv is not None:
            raw32 = raw32 + sv.cpu()[c.graph.V]
        if se is not None:
            raw32 = raw32 + se.cpu()[c.graph.E]
        alpha = c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, 0.2)
        plain = c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, c.dalpha, sv, se, group, 1.0)[0].cpu()
        leaky = c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, c.dalpha, sv, se, group, 0.2)[0].cpu()
        want = torch.where(raw32 > 0, plain, plain * slope32)
        err = (gr.f64(leaky) - gr.f64(want)).abs()
        tol = 4 * U * gr.f64(want).abs().clamp(min=gr.TINY)
        print("%s %s %s: ds(0.2) against ds(1.0) leaky'(raw): max err / tol %.3g, %d of %d entries bit-equal" % (
            shape, group, mode, float((err / tol).max()), int((ar.bits(leaky) == ar.bits(want)).sum()), c.inc.nnz))
        assert bool((err <= tol).all()), (shape, group, mode)
        assert int((raw32 > 0).sum()) > 100 and int((raw32 <= 0).sum()) > 100


@pytest.mark.parametrize("shape,group", WIDTH_CELLS)
def test_entries_do_not_depend_on_the_requested_sums(case, shape, group):
    c = case(shape)
    for mode in MODES:
        sv, se = c.scores(mode)
        for slope in SLOPES:
            alpha = c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, slope)
            full = c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, c.dalpha, sv, se, group, slope)
            for need_sv, need_se in ((False, False), (True, False), (False, True)):
                part = c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, c.dalpha, sv, se, group, slope,
                                                           need_sv=need_sv, need_se=need_se)
                what = (shape, group, mode, slope, need_sv, need_se)
                assert (part[1] is not None) == need_sv and (part[2] is not None) == need_se, what
                for a, b in zip(part, full):
                    assert a is None or torch.equal(ar.bits(a), ar.bits(b)), what
