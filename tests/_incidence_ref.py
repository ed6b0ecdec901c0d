"""Float64 reference of the incidence-weighted aggregation (ops.incidence_aggr) and its gradients: CPU, plain torch, test
infrastructure only.

For the H_T entries p = (e, u) (graph.E[p] = e, graph.V[p] = u):
    Xe[e] = degE[e] * W[e] * sum_{p=(e,u)} v2e[p] * X[u]
    Y[v]  = degV[v]        * sum_{p=(e,v)} e2v[p] * Xe[e]
v2e / e2v None means unit weights.  Written with index_add_, so torch.autograd differentiates it for X and both weight
arrays.  The mass of a quantity is the same expression on |X|, |v2e|, |e2v|, |degE|, |degV|, |W| and |dY|
(_grad_ref.evaluate does that); the checks are |got - ref| <= c * max(mass, TINY), c as the issue of the operator sets it.
"""
import torch

from _grad_ref import FP32_C, TINY, f64  # noqa: F401  (re-exported for the tests)

F64 = torch.float64


def incidence_aggr(graph, x, v2e=None, e2v=None):
    """Y for a _grad_ref.Graph (its V / E index arrays and float64 se = degE * W, degV)."""
    xs = x[graph.V]
    if v2e is not None:
        xs = xs * v2e.reshape(-1, 1)
    xe = torch.zeros(graph.M, x.shape[1], dtype=x.dtype).index_add_(0, graph.E, xs)
    if graph.se is not None:
        xe = xe * graph.se.reshape(-1, 1)
    ys = xe[graph.E]
    if e2v is not None:
        ys = ys * e2v.reshape(-1, 1)
    y = torch.zeros(graph.N, x.shape[1], dtype=x.dtype).index_add_(0, graph.V, ys)
    return y if graph.degV is None else y * graph.degV.reshape(-1, 1)


def hop1(graph, x, v2e=None):
    """Xe = De W H_v2e^T x: hop 1 of incidence_aggr alone."""
    xs = x[graph.V] if v2e is None else x[graph.V] * v2e.reshape(-1, 1)
    xe = torch.zeros(graph.M, x.shape[1], dtype=x.dtype).index_add_(0, graph.E, xs)
    return xe if graph.se is None else xe * graph.se.reshape(-1, 1)


def closed_form_grads(graph, x, v2e, e2v, g):
    """The backward the library implements (ops._IncidenceAggr), in float64: with P = degV * g,
    G = De W H_e2v^T P, dX = H_v2e G, dv2e[p=(e,u)] = <x[u], G[e]>, de2v[p=(e,v)] = <P[v], Xe[e]>."""
    P = g if graph.degV is None else g * graph.degV.reshape(-1, 1)
    G = hop1(graph, P, e2v)
    dxs = G[graph.E] if v2e is None else G[graph.E] * v2e.reshape(-1, 1)
    dx = torch.zeros(graph.N, x.shape[1], dtype=x.dtype).index_add_(0, graph.V, dxs)
    dv2e = (x[graph.V] * G[graph.E]).sum(1)
    Xe = hop1(graph, x, v2e)
    de2v = (P[graph.V] * Xe[graph.E]).sum(1)
    return dx, dv2e, de2v


def dot(graph, a, b):
    """incidence_dot in float64: out[p = (e, u)] = <a[u], b[e]>."""
    return (f64(a)[graph.V] * f64(b)[graph.E]).sum(1)


def dot_mass(graph, a, b):
    return (f64(a).abs()[graph.V] * f64(b).abs()[graph.E]).sum(1)


def fn(graph, x, v2e=None, e2v=None):
    """incidence_aggr in the keyword form _grad_ref.evaluate calls."""
    return incidence_aggr(graph, x, v2e, e2v)
