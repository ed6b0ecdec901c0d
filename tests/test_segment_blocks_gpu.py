"""The one work split of the segment kernels (hg_attention.hip, segment_kernel) under each of its five argument blocks.
tests/test_attention_widths.py crosses segment lengths and lane-group widths for the plain single-head bodies (SegArgs);
here the same cut is reached through the other four blocks -- heads (SegHeadsArgs), dropout (SegDropArgs,
SegDropHeadsArgs) and entry logits (SegEntryArgs, with heads = 1 and 3, with and without dropout) -- and tied back to the
plain entries by properties the kernels document.  Every comparison is torch.equal on bits: there is no tolerance.

Shapes: `blocks_W` for W = 4, 8, 16 -- hyperedges of 0, 1, 128 and 129 members (128 is the longest row a lane group takes,
129 gets a workgroup of its own), then FILL[W] hyperedges of 2 members, which put the mean of the rows a lane group
walks at 3.98, 4.98 or 10.9 and so the side's width at W, then one more empty hyperedge; 160 vertices, 282 to 380
incidences, and more segments than one workgroup has lane groups.  `blocks_W_T`, the transpose, puts the same lengths on
the vertex side.  Both groups run on every shape, with heads 1 and 3.

1. Column h of a heads = 3 call has the bits of the single-head call on column h of the inputs: the softmax, its backward
   (ds, dsv, dse), the statistics and the segment sum.
2. Each further block gives the plain entries' bits where what it adds is the identity: dropout at p_drop = 0 (every entry
   kept, scale 1.0f) gives alpha, ds, dsv and dse, and alpha_drop equals alpha; entry_score = 0 gives them with and without
   heads; so do the entry-logit dropout entries at p_drop = 0 and entry_score = 0.
3. Every output of 2 is written into a buffer filled with a sentinel beforehand, guard words on either side.  The last
   segment of the designed side is empty and begins where the per-entry arrays end: its positions are the first guard
   words, and they keep the sentinel, as do all the others, while every real position loses it.  In the per-segment
   outputs an empty segment's word is the documented 0.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = ar.DEV
SENTINEL = ar.SENTINEL
GUARD = 64
HEADS = (1, 3)
FILL = {4: 61, 8: 40, 16: 12}  # hyperedges of 2 members beside those of 1 and 128: means 251 / 63, 209 / 42, 153 / 14
STATE = (0x0123456789ABCDEF, -0x0EDCBA9876543210)  # {key, sid} as int64
_bits = ar.bits


def _shape(width):
    return synth._from_sizes(np.random.default_rng(9), 160, [0, 1, 128, 129] + [2] * FILL[width] + [0],
                             name="blocks_%d" % width)


# name -> (builder, designed side, the width that side must run at)
SHAPES = {}
for _w in (4, 8, 16):
    SHAPES["blocks_%d" % _w] = (lambda w=_w: _shape(w), "hyperedge", _w)
    SHAPES["blocks_%d_T" % _w] = (lambda w=_w: ar.transpose(_shape(w)), "vertex", _w)


class Case(ar.Case):
    """ar.Case with scores and gradients for every head count, and the plain entries' results: computed once, shared by
    the tests, never modified."""

    def __init__(self, hg, inc, name):
        super().__init__(hg, inc, name)
        g = torch.Generator().manual_seed(57)
        H = HEADS[1]
        sv, se = torch.randn(inc.N, H, generator=g), torch.randn(inc.M, H, generator=g)
        self.hsv = {1: self.sv, H: (sv * (4.0 / float(sv.abs().max()))).to(DEV)}
        self.hse = {1: self.se, H: (se * (4.0 / float(se.abs().max()))).to(DEV)}
        self.hgrad = {1: self.dalpha, H: torch.randn(inc.nnz, H, generator=g).to(DEV)}
        self.hval = {1: self.val, H: torch.randn(inc.nnz, H, generator=g).to(DEV)}
        self.rng = torch.tensor(STATE, dtype=torch.int64, device=DEV)
        self._plain = {}

    def plain(self, H, group, slope):
        """(alpha, ds, dsv, dse) of incidence_attention / _backward: SegArgs at H = 1, SegHeadsArgs at H = 3."""
        key = (H, group, slope)
        if key not in self._plain:
            sv, se = self.hsv[H], self.hse[H]
            alpha = self.plan.incidence_attention(self.ptr, self.ind, sv, se, group, slope, heads=H)
            self._plain[key] = (alpha,) + self.plan.incidence_attention_backward(self.ptr, self.ind, alpha, self.hgrad[H], sv, se,
                                                                                 group, slope, heads=H)
        return self._plain[key]


_CASES = {}


@pytest.fixture
def case(hg):
    def get(name):
        if name not in _CASES:
            _CASES[name] = Case(hg, SHAPES[name][0](), name)  # all six are tiny: they stay
        return _CASES[name]
    return get


def _guarded(*shape):
    """(buffer, view): a SENTINEL-filled buffer and the output inside it, GUARD words on either side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_kept(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _col(t, h):
    return t[:, h].contiguous()


def test_shapes_reach_every_width_and_both_sides_of_the_long_rule(case):
    for name, (_, side, width) in SHAPES.items():
        c = case(name)
        info = c.plan.segment_info(side)
        lens = ar.side_lengths(c.inc, side)
        print("%s: %s side W %d, %d segments, %d incidences, long rows %s" % (
            name, side, info["width"], lens.size, c.inc.nnz, list(info["long_rows"])))
        assert info["width"] == width and info["long"] == 128, (name, info)
        assert {0, 1, 128, 129} <= set(int(x) for x in lens), name
        np.testing.assert_array_equal(info["long_rows"], np.nonzero(lens > 128)[0])
        assert len(info["long_rows"]) == 1 and lens[0] == 0 and lens[-1] == 0, name
        assert lens.size > 256 // width and lens.size % (256 // width) != 0, name  # two workgroups, the last one partly idle
        assert 200 <= c.inc.nnz <= 400, name


@pytest.mark.parametrize("shape", list(SHAPES))
def test_head_columns_equal_the_single_head_calls(case, shape):
    c = case(shape)
    H = HEADS[1]
    sv, se, grad, val = c.hsv[H], c.hse[H], c.hgrad[H], c.hval[H]
    for group in ar.GROUPS:
        total = c.plan.incidence_sum(c.ptr, c.ind, val, group, heads=H)
        for h in range(H):
            assert torch.equal(_bits(_col(total, h)), _bits(c.plan.incidence_sum(c.ptr, c.ind, _col(val, h), group))), (group, h)
        for slope in ar.SLOPES:
            got = c.plain(H, group, slope)
            stats = c.plan.incidence_attention_stats(c.ptr, c.ind, sv, se, group, slope, heads=H)
            for h in range(H):
                what = "%s %s slope %g column %d" % (shape, group, slope, h)
                a, b = _col(sv, h), _col(se, h)
                alpha = c.plan.incidence_attention(c.ptr, c.ind, a, b, group, slope)
                want = (alpha,) + c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, _col(grad, h), a, b, group, slope)
                for name, g, w in zip(("alpha", "ds", "dsv", "dse"), got, want):
                    assert torch.equal(_bits(_col(g, h)), _bits(w)), "%s: %s" % (name, what)
                one = c.plan.incidence_attention_stats(c.ptr, c.ind, a, b, group, slope)
                for name, g, w in zip(("seg_max", "seg_inv"), stats, one):
                    assert torch.equal(_bits(_col(g, h)), _bits(w)), "%s: %s" % (name, what)


# what a block adds to the plain call: (entry logits?, p_drop or None)
FORMS = {"plain": (False, None), "dropout": (False, 0.0), "entry": (True, None), "entry+dropout": (True, 0.0)}


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_block_gives_the_plain_bits_and_writes_its_own_positions_only(case, shape, H):
    from hypergef_amd import _lib
    from hypergef_amd.plan import _ptr, _stream_handle
    c = case(shape)
    N, M, nnz = c.inc.N, c.inc.M, c.inc.nnz
    st = _stream_handle(torch.device(DEV))
    sv, se, grad = c.hsv[H], c.hse[H], c.hgrad[H]
    zeros = torch.zeros(nnz, H, device=DEV)
    empty = {"vertex": torch.from_numpy(ar.side_lengths(c.inc, "vertex") == 0),
             "hyperedge": torch.from_numpy(ar.side_lengths(c.inc, "hyperedge") == 0)}
    assert bool(empty[SHAPES[shape][1]][-1])  # its positions begin at nnz: the first guard words

    def run(bwd, group, slope, form, arrays):
        has_entry, pd = FORMS[form]
        fn, args = c.plan._softmax_entry(bwd, ar.GROUPS.index(group), H, c.ptr, c.ind, sv, se, zeros if has_entry else None,
                                         slope, pd, None if pd is None else _ptr(c.rng))
        _lib.check(fn(*args, *[_ptr(t) for t in arrays], st))
        torch.cuda.synchronize()

    for group in ar.GROUPS:
        for slope in ar.SLOPES:
            alpha, ds, dsv, dse = c.plain(H, group, slope)
            for form, (_, pd) in FORMS.items():
                what = "%s H %d %s slope %g %s" % (shape, H, group, slope, form)
                outs = [_guarded(nnz, H) for _ in range(1 if pd is None else 2)]
                run(False, group, slope, form, [o for _, o in outs])
                for name, (buf, o) in zip(("alpha", "alpha_drop"), outs):
                    assert _guards_kept(buf), "%s guard words: %s" % (name, what)
                    assert not bool((o == SENTINEL).any()), "a real position of %s was not written: %s" % (name, what)
                    assert torch.equal(_bits(o.reshape(alpha.shape)), _bits(alpha)), "%s: %s" % (name, what)
                outs = [_guarded(nnz, H), _guarded(N, H), _guarded(M, H)]
                run(True, group, slope, form, [alpha, grad] + [o for _, o in outs])
                for name, (buf, o), w in zip(("ds", "dsv", "dse"), outs, (ds, dsv, dse)):
                    assert _guards_kept(buf), "%s guard words: %s" % (name, what)
                    assert not bool((o == SENTINEL).any()), "a real position of %s was not written: %s" % (name, what)
                    assert torch.equal(_bits(o.reshape(w.shape)), _bits(w)), "%s: %s" % (name, what)
                for side, (_, o) in (("vertex", outs[1]), ("hyperedge", outs[2])):
                    assert bool((_bits(o.cpu()[empty[side]]) == 0).all()), "an empty %s's sum is not +0.0: %s" % (side, what)
