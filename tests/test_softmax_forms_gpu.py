"""ops.incidence_softmax is one autograd node over the four public softmax methods of Plan, whatever the form of the call:
with or without incidence_score, with or without dropout.  For every form, both groups and heads in {1, 3}:

a. the tracked call (a score requires a gradient) and the untracked one return the same bits;
b. the tracked result's grad_fn is _IncidenceSoftmaxBackward;
c. the gradients of node_score, edge_score and -- where given -- incidence_score under a fixed dout are, bit for bit,
   what the matching public Plan forward and backward methods return when they are called directly with the same
   arguments, without autograd.

Bit equality, no tolerance: both sides run the same kernels on the same inputs.  Shapes: the toy graph of the host tests
and `ragged` (700 / 450, 10 % empty, rows of several lane-group widths) -- the smallest on which a wrong choice among the
eight C entries, or a wrong saved tensor (the dropped coefficients for the undropped ones), changes a bit."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402

from hypergef_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = ar.DEV
SLOPE, PD = 0.2, 0.5
SHAPES = {
    "toy": ar.toy,
    "ragged": lambda: synth.random_incidence(700, 450, 7.0, seed=3, empty_frac=0.1),
}
FORMS = [(entry, drop) for entry in (False, True) for drop in (False, True)]
_bits = ar.bits
_CASES = {}


def _case(name, H):
    """The graph on the device with scores, a logit per incidence and a dout for H heads: drawn once, never modified."""
    if (name, H) not in _CASES:
        from hypergef_amd.plan import Plan
        inc = SHAPES[name]()
        g = torch.Generator().manual_seed(60 + H)
        shape = (lambda n: (n,)) if H == 1 else (lambda n: (n, H))
        c = {"inc": inc, "ptr": torch.from_numpy(inc.csrptr).to(DEV), "ind": torch.from_numpy(inc.colind).to(DEV)}
        for key, n in (("sv", inc.N), ("se", inc.M), ("t", inc.nnz), ("dout", inc.nnz)):
            c[key] = torch.randn(shape(n), generator=g).to(DEV)
        c["plan"] = Plan.from_tensors(inc.N, c["ptr"], c["ind"])
        c["rng"] = torch.tensor([0x0123456789ABCDEF, -0x0EDCBA9876543210], dtype=torch.int64, device=DEV)
        _CASES[(name, H)] = c
    return _CASES[(name, H)]


@pytest.mark.parametrize("H", (1, 3))
@pytest.mark.parametrize("group", ar.GROUPS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_form_is_one_node_over_the_plan_methods(hg, shape, group, H):
    c = _case(shape, H)
    plan, ptr, ind, sv, se, dout = c["plan"], c["ptr"], c["ind"], c["sv"], c["se"], c["dout"]
    seen = {}
    for entry, drop in FORMS:
        what = "%s %s H=%d entry=%s dropout=%s" % (shape, group, H, entry, drop)
        t = c["t"] if entry else None
        kw = dict(group=group, negative_slope=SLOPE, num_nodes=c["inc"].N, heads=H)
        if drop:
            kw.update(dropout=PD, rng_state=c["rng"])
        untracked = hg.ops.incidence_softmax(ptr, ind, sv, se, incidence_score=t, **kw)
        assert untracked.grad_fn is None and not untracked.requires_grad, what
        leaves = [x.clone().requires_grad_(True) if x is not None else None for x in (sv, se, t)]
        tracked = hg.ops.incidence_softmax(ptr, ind, leaves[0], leaves[1], incidence_score=leaves[2], **kw)
        assert torch.equal(_bits(tracked.detach()), _bits(untracked)), "a: " + what
        assert type(tracked.grad_fn).__name__.startswith("_IncidenceSoftmaxBackward"), (what, type(tracked.grad_fn))
        grads = torch.autograd.grad(tracked, [x for x in leaves if x is not None], dout)
        # the same computation on the Plan's public methods, no autograd
        if drop:
            alpha, direct = plan.incidence_attention_dropout(ptr, ind, sv, se, group, SLOPE, PD, c["rng"], heads=H, entry=t)
            want = plan.incidence_attention_dropout_backward(ptr, ind, alpha, dout, sv, se, group, SLOPE, PD, c["rng"],
                                                             heads=H, entry=t)
        else:
            alpha = direct = plan.incidence_attention(ptr, ind, sv, se, group, SLOPE, heads=H, entry=t)
            want = plan.incidence_attention_backward(ptr, ind, alpha, dout, sv, se, group, SLOPE, heads=H, entry=t)
        torch.cuda.synchronize()
        assert torch.equal(_bits(untracked), _bits(direct)), "the operator is not the Plan method: " + what
        ds, dsv, dse = want
        for name, got, ref in zip(("node_score", "edge_score", "incidence_score"), grads, (dsv, dse, ds)):
            assert got.shape == ref.shape and torch.equal(_bits(got), _bits(ref)), "c: d %s: %s" % (name, what)
        assert len(grads) == (3 if entry else 2)
        seen[(entry, drop)] = untracked
    # the four forms are four different results: none of them fell through to another's entry
    if c["inc"].nnz >= 8:
        keys = list(seen)
        for i, a in enumerate(keys):
            for b in keys[i + 1:]:
                assert not torch.equal(_bits(seen[a]), _bits(seen[b])), (shape, group, H, a, b)
