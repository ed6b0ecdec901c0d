"""Float64 reference of the softmax over per-incidence logits (ops.incidence_softmax(incidence_score=...)), of the one-hop
weighted gather (ops.incidence_gather), the differentiable dot product (ops.incidence_dot) and the dot-product layer
(models.HypergraphAttnConv(score="dot")): CPU, plain torch, test infrastructure only.

Everything per incidence is [nnz, H] (H = 1 included), head fastest, as in include/hg_aggr.h; `graph` is a
_grad_ref.Graph.  For the H_T entries p = (e, u):
    raw[p, h]   = (sv[u, h] + se[e, h]) + t[p, h]       the bracket rounded to fp32 first, as the kernel forms it
    alpha[p, h] = softmax over p's group of leaky_relu(raw[p, h], slope)
"""
import torch

import _attention_ref as ar
import _heads_ref as hr
from _grad_ref import f64

F64 = torch.float64
U = ar.U


def seg_sum(graph, val, side):
    """[groups, H] from val [nnz, H]."""
    idx, n = ar.index_of(graph, side)
    return torch.zeros(n, val.shape[1], dtype=val.dtype).index_add_(0, idx, val)


def raw32(graph, sv, se, heads):
    """fp32 [nnz, H]: (sv[u] + se[e]) as fp32 forms it, +0 for a missing one.  sv / se: fp32 CPU tensors or None."""
    raw = torch.zeros(graph.V.numel(), heads, dtype=torch.float32)
    if sv is not None:
        raw = raw + sv.reshape(-1, heads)[graph.V]
    if se is not None:
        raw = raw + se.reshape(-1, heads)[graph.E]
    return raw


def raw64(graph, sv, se, t, heads):
    """The three-term logit in float64: the fp32 bracket, then t added in float64."""
    return raw32(graph, sv, se, heads).double() + t.reshape(-1, heads).double()


def draw_entry(graph, sv, se, heads, seed, scale=4.0, floor=1e-3):
    """fp32 t [nnz, H], normal, max |t| about `scale`, such that no |raw| < floor: the entries that miss are drawn again
    from the same seeded generator until none is left (the sign of raw must be the same in fp32 and float64)."""
    g = torch.Generator().manual_seed(seed)
    nnz = graph.V.numel()
    t = torch.randn(nnz, heads, generator=g)
    if nnz:
        t = t * (scale / float(t.abs().max()))
    base = raw32(graph, sv, se, heads).double()
    for _ in range(64):
        bad = (base + t.double()).abs() < floor
        if not bool(bad.any()):
            break
        t[bad] = torch.randn(int(bad.sum()), generator=g).clamp(-scale, scale)
    assert not bool(((base + t.double()).abs() < floor).any())
    return t


def softmax_raw(graph, raw, group, slope):
    """alpha [nnz, H] in the dtype of raw; differentiable in raw."""
    idx, n = ar.index_of(graph, group)
    s = torch.nn.functional.leaky_relu(raw, slope)
    ix = idx.reshape(-1, 1).expand_as(s)
    m = torch.full((n, raw.shape[1]), -float("inf"), dtype=raw.dtype).scatter_reduce(0, ix, s.detach(), "amax")
    e = torch.exp(s - m[idx])
    return e / seg_sum(graph, e, group)[idx]


def closed_form_backward(graph, raw, group, slope, alpha, dalpha):
    """_attention_ref.closed_form_backward on the three-term raw, extended by dt = ds: (ds, dsv, dse, dt)."""
    idx, _ = ar.index_of(graph, group)
    tt = seg_sum(graph, alpha * dalpha, group)[idx]
    ds = alpha * (dalpha - tt) * torch.where(raw > 0, torch.ones_like(raw), torch.full_like(raw, slope))
    return ds, seg_sum(graph, ds, "vertex"), seg_sum(graph, ds, "hyperedge"), ds


def backward_masses(graph, group, slope, alpha, dalpha):
    """_attention_ref.backward_masses for [nnz, H] arrays: (mass_ds, mass_dsv, mass_dse)."""
    idx, _ = ar.index_of(graph, group)
    mass = alpha * (dalpha.abs() + seg_sum(graph, alpha * dalpha.abs(), group)[idx]) * max(1.0, abs(slope))
    return mass, seg_sum(graph, mass, "vertex"), seg_sum(graph, mass, "hyperedge")


def bound_c(L, smax):
    """|alpha - ref| <= c ref: test_attention_gpu.py's (L + 16 + 16 Smax) U with one more fp32 addition in the logit,
    counted as that file counts each operation -- 2 Smax U in an exponent of the numerator and of every term of the
    denominator: 4 Smax U more."""
    return (L + 16 + 20 * smax) * U


# ---- the one-hop gather and the dot product --------------------------------------------------------------------------------

def gather(graph, src, w=None, sa=None, sb=None, to="hyperedge", heads=1):
    """ops.incidence_gather in the dtype of src, in the keyword form _grad_ref.evaluate calls (graph, **inputs)."""
    rows, out_idx, n = (graph.V, graph.E, graph.M) if to == "hyperedge" else (graph.E, graph.V, graph.N)
    xs = src[rows]
    if w is not None:
        C = src.shape[1] // heads
        xs = (xs.view(-1, heads, C) * w.reshape(-1, heads, 1)).reshape(-1, heads * C)
    out = torch.zeros(n, src.shape[1], dtype=src.dtype).index_add_(0, out_idx, xs)
    for s in (sa, sb):
        if s is not None:
            out = out * s.reshape(-1, 1)
    return out


def dot(graph, a, b, heads=1):
    """ops.incidence_dot, differentiable (hr.dot detaches): out[p, h] = <a[u, head h], b[e, head h]>, [nnz, H]."""
    prod = a[graph.V] * b[graph.E]
    return prod.view(prod.shape[0], heads, -1).sum(2)


# ---- the layer --------------------------------------------------------------------------------------------------------------

class _MassSoftmax(torch.autograd.Function):
    """The softmax of the logits whose backward returns the MASS of d logits (backward_masses' mass_ds) instead of its
    value: with every other factor of the layer non-negative, autograd then accumulates the mass of every parameter
    gradient, as _attention_ref._MassSoftmax does for the additive layer."""

    @staticmethod
    def forward(ctx, logits, graph, group, slope):
        alpha = softmax_raw(graph, logits.detach(), group, slope)
        ctx.save_for_backward(alpha)
        ctx.args = (graph, group, slope)
        return alpha

    @staticmethod
    def backward(ctx, dalpha):
        (alpha,) = ctx.saved_tensors
        return backward_masses(*ctx.args, alpha, dalpha)[0], None, None, None


def dot_conv(graph, x, weight, weight_k, bias, group="hyperedge", slope=0.2, heads=1, concat=True, mass=False):
    """models.HypergraphAttnConv(score="dot") in float64; graph carries degE / degV.  Returns (Y, logits)."""
    N = x.shape[0]
    C = weight.shape[0] // heads
    z = x @ weight.t()
    kv = x @ weight_k.t()
    sizes = ar.segment_sum(graph, torch.ones(graph.V.numel(), dtype=F64), "hyperedge")
    inv = torch.where(sizes > 0, 1.0 / sizes.clamp(min=1.0), torch.zeros_like(sizes))
    ke = gather(graph, kv, None, inv, None, "hyperedge")
    logits = dot(graph, z, ke, heads) * C ** -0.5
    alpha = _MassSoftmax.apply(logits, graph, group, slope) if mass else softmax_raw(graph, logits, group, slope)
    y = hr.incidence_aggr(graph, z, alpha, alpha, heads)
    if not concat:
        y = y.view(N, heads, C).mean(1)
    return y + bias, logits.detach()


__all__ = ["f64"]
