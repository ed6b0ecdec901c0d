"""Float64 reference of the hypergraph attention coefficients (ops.incidence_softmax), the segment sum (ops.incidence_sum) and
the layer built from them (models.HypergraphAttnConv): CPU, plain torch indexing, test infrastructure only.

For the H_T entries p = (e, u) (graph.E[p] = e, graph.V[p] = u, a _grad_ref.Graph):
    raw[p]   = sv[u] + se[e]                 (either may be None: 0)
    s[p]     = leaky_relu(raw[p], slope)     (torch's convention: slope * raw for raw <= 0)
    alpha[p] = exp(s[p] - m_g) / sum_{q in g} exp(s[q] - m_g),   g = p's hyperedge (group "hyperedge") or vertex ("vertex")
"""
import numpy as np
import torch

from _grad_ref import f64  # noqa: F401
import _incidence_ref as ir

from hypergef_amd import synth

F64 = torch.float64
GROUPS = ("hyperedge", "vertex")
U = 2.0 ** -24


def toy():
    """A hand-made H_T: vertex 2 twice in hyperedge 1, hyperedge 2 empty, vertex 4 in no hyperedge, hyperedge 4 with the
    one member 3; vertex 1 is in one hyperedge only (a one-entry vertex group)."""
    ptr = np.array([0, 3, 7, 7, 9, 10], np.int32)
    ind = np.array([0, 2, 3, 1, 2, 2, 5, 0, 5, 3], np.int32)
    return synth.Incidence(6, 5, ptr, ind, name="toy")


def transpose(inc):
    """The incidence with the roles of vertices and hyperedges swapped (H as an H_T), entries in stable order."""
    order = np.argsort(inc.colind, kind="stable")
    rows = np.repeat(np.arange(inc.M, dtype=np.int32), np.diff(inc.csrptr))
    ptr = np.zeros(inc.N + 1, np.int64)
    np.add.at(ptr, inc.colind.astype(np.int64) + 1, 1)
    return synth.Incidence(inc.M, inc.N, np.cumsum(ptr).astype(np.int32), rows[order], name=inc.name + "-T")


def index_of(graph, group):
    """(segment id of every H_T entry, number of segments) of a group / side."""
    assert group in GROUPS, group
    return (graph.E, graph.M) if group == "hyperedge" else (graph.V, graph.N)


def raw_score(graph, sv, se):
    raw = torch.zeros(graph.V.numel(), dtype=F64)
    if sv is not None:
        raw = raw + sv.reshape(-1)[graph.V]
    if se is not None:
        raw = raw + se.reshape(-1)[graph.E]
    return raw


def segment_sum(graph, val, side):
    idx, n = index_of(graph, side)
    return torch.zeros(n, dtype=val.dtype).index_add_(0, idx, val)


def softmax(graph, sv=None, se=None, group="hyperedge", slope=0.2):
    """alpha [nnz], differentiable in sv / se.  The subtracted maximum is a constant of the formula (it cancels)."""
    idx, n = index_of(graph, group)
    s = torch.nn.functional.leaky_relu(raw_score(graph, sv, se), slope)
    m = torch.full((n,), -float("inf"), dtype=F64).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
    e = torch.exp(s - m[idx])
    return e / segment_sum(graph, e, group)[idx]


def closed_form_backward(graph, sv, se, group, slope, alpha, dalpha):
    """What hg_incidence_attention_bwd_f32 computes, in float64: (ds, dsv, dse)."""
    idx, _ = index_of(graph, group)
    t = segment_sum(graph, alpha * dalpha, group)[idx]
    raw = raw_score(graph, sv, se)
    ds = alpha * (dalpha - t) * torch.where(raw > 0, torch.ones_like(raw), torch.full_like(raw, slope))
    return ds, segment_sum(graph, ds, "vertex"), segment_sum(graph, ds, "hyperedge")


def backward_masses(graph, group, slope, alpha, dalpha):
    """The magnitudes the backward's sums are made of: mass_ds[p] = alpha[p] (|dalpha[p]| + sum_g alpha |dalpha|)
    max(1, slope), and its segment sums over vertices / hyperedges."""
    idx, _ = index_of(graph, group)
    mass = alpha * (dalpha.abs() + segment_sum(graph, alpha * dalpha.abs(), group)[idx]) * max(1.0, abs(slope))
    return mass, segment_sum(graph, mass, "vertex"), segment_sum(graph, mass, "hyperedge")


def longest(inc, side):
    """The longest group of a side."""
    sizes = np.diff(inc.csrptr) if side == "hyperedge" else np.bincount(inc.colind, minlength=inc.N)
    return int(sizes.max()) if sizes.size else 0


class _MassSoftmax(torch.autograd.Function):
    """softmax whose backward returns the MASSES of dsv / dse (backward_masses) instead of their values.  In a layer whose
    every other factor is non-negative, autograd then accumulates the mass of every parameter gradient: the softmax
    backward's difference dalpha - t is the only place where terms cancel."""

    @staticmethod
    def forward(ctx, sv, se, graph, group, slope):
        alpha = softmax(graph, sv.detach(), se.detach(), group, slope)
        ctx.save_for_backward(alpha)
        ctx.args = (graph, group, slope)
        return alpha

    @staticmethod
    def backward(ctx, dalpha):
        (alpha,) = ctx.saved_tensors
        _, mv, me = backward_masses(*ctx.args, alpha, dalpha)
        return mv, me, None, None, None


def attn_conv(graph, x, weight, a_v, a_e, bias, group="hyperedge", slope=0.2, mass=False):
    """models.HypergraphAttnConv in float64: graph carries degE / degV (a _grad_ref.Graph built without W).  mass=True
    (non-negative inputs only): the same value, but backward yields every gradient's mass (_MassSoftmax)."""
    z = x @ weight.t()
    sv = z @ a_v
    sizes = segment_sum(graph, torch.ones(graph.V.numel(), dtype=F64), "hyperedge")
    inv = torch.where(sizes > 0, 1.0 / sizes.clamp(min=1.0), torch.zeros_like(sizes))
    se = segment_sum(graph, (z @ a_e)[graph.V], "hyperedge") * inv
    alpha = _MassSoftmax.apply(sv, se, graph, group, slope) if mass else softmax(graph, sv, se, group, slope)
    return ir.incidence_aggr(graph, z, alpha, alpha) + bias
