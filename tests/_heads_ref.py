"""Float64 reference of the multi-head incidence path (heads=H of ops.incidence_softmax / incidence_sum / incidence_aggr,
Plan.incidence_dot, models.HypergraphAttnConv): CPU, plain torch, test infrastructure only.

Layout as in include/hg_aggr.h: the head is the fastest index.  Scores are [N, H] / [M, H], everything per incidence is
[nnz, H], features are [N, H * C] and head h owns columns h C .. (h + 1) C - 1.  Every function here is the single-head
reference of _attention_ref.py / _incidence_ref.py applied to each head's column (or column block) and stacked, so the
bounds of the single-head tests hold per head unchanged.
"""
import torch

import _attention_ref as ar
import _incidence_ref as ir
from _grad_ref import f64  # noqa: F401

F64 = torch.float64


def _col(t, h):
    return None if t is None else t[:, h]


def softmax(graph, sv=None, se=None, group="hyperedge", slope=0.2, heads=1):
    """alpha [nnz, H] from sv [N, H] / se [M, H] (either may be None); differentiable."""
    return torch.stack([ar.softmax(graph, _col(sv, h), _col(se, h), group, slope) for h in range(heads)], 1)


def closed_form_backward(graph, sv, se, group, slope, alpha, dalpha):
    """(ds [nnz, H], dsv [N, H], dse [M, H]): _attention_ref.closed_form_backward per head."""
    parts = [ar.closed_form_backward(graph, _col(sv, h), _col(se, h), group, slope, alpha[:, h], dalpha[:, h])
             for h in range(alpha.shape[1])]
    return tuple(torch.stack([p[i] for p in parts], 1) for i in range(3))


def backward_masses(graph, group, slope, alpha, dalpha):
    parts = [ar.backward_masses(graph, group, slope, alpha[:, h], dalpha[:, h]) for h in range(alpha.shape[1])]
    return tuple(torch.stack([p[i] for p in parts], 1) for i in range(3))


def segment_sum(graph, val, side):
    """[groups, H] from val [nnz, H]."""
    return torch.stack([ar.segment_sum(graph, val[:, h], side) for h in range(val.shape[1])], 1)


def incidence_aggr(graph, x, v2e=None, e2v=None, heads=1):
    """Y [N, H * C]: head h's columns weighted by column h of v2e / e2v ([nnz, H] or None)."""
    C = x.shape[1] // heads
    assert C * heads == x.shape[1]
    return torch.cat([ir.incidence_aggr(graph, x[:, h * C:(h + 1) * C], _col(v2e, h), _col(e2v, h)) for h in range(heads)], 1)


def fn(graph, x, v2e=None, e2v=None, heads=1):
    """incidence_aggr in the keyword form _grad_ref.evaluate calls (heads travels as a plain number)."""
    return incidence_aggr(graph, x, v2e, e2v, heads)


def dot(graph, a, b, heads=1):
    """out[p, h] = <a[u, head h], b[e, head h]> for p = (e, u), [nnz, H]."""
    prod = f64(a)[graph.V] * f64(b)[graph.E]
    return prod.view(prod.shape[0], heads, -1).sum(2)


def dot_mass(graph, a, b, heads=1):
    return dot(graph, f64(a).abs(), f64(b).abs(), heads)


class _MassSoftmax(torch.autograd.Function):
    """_attention_ref._MassSoftmax per head: the value of the softmax, the masses of dsv / dse in the backward."""

    @staticmethod
    def forward(ctx, sv, se, graph, group, slope):
        alpha = softmax(graph, sv.detach(), se.detach(), group, slope, sv.shape[1])
        ctx.save_for_backward(alpha)
        ctx.args = (graph, group, slope)
        return alpha

    @staticmethod
    def backward(ctx, dalpha):
        (alpha,) = ctx.saved_tensors
        _, mv, me = backward_masses(*ctx.args, alpha, dalpha)
        return mv, me, None, None, None


def attn_conv(graph, x, weight, a_v, a_e, bias, group="hyperedge", slope=0.2, heads=1, concat=True, mass=False):
    """models.HypergraphAttnConv(heads, concat) in float64; graph carries degE / degV.  mass=True (non-negative inputs
    only): the same value, but backward yields every gradient's mass."""
    N = x.shape[0]
    C = weight.shape[0] // heads
    z = x @ weight.t()
    zh = z.view(N, heads, C)
    sv = (zh * a_v.view(heads, C)).sum(-1)
    sizes = ar.segment_sum(graph, torch.ones(graph.V.numel(), dtype=F64), "hyperedge")
    inv = torch.where(sizes > 0, 1.0 / sizes.clamp(min=1.0), torch.zeros_like(sizes))
    ze = (zh * a_e.view(heads, C)).sum(-1)[graph.V]
    se = segment_sum(graph, ze, "hyperedge") * inv.reshape(-1, 1)
    alpha = _MassSoftmax.apply(sv, se, graph, group, slope) if mass else softmax(graph, sv, se, group, slope, heads)
    y = incidence_aggr(graph, z, alpha, alpha, heads)
    if not concat:
        y = y.view(N, heads, C).mean(1)
    return y + bias
