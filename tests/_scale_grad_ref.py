"""Float64 reference of the scale gradients (CPU, plain torch): test infrastructure only.

_grad_ref.Graph holds degE / degV / W as constants of the graph.  Here they are inputs:

    Y = degV . H_e2v (degE . W . (H_v2e^T X))          H_v2e / H_e2v: H with a weight per incidence (None: plain H)

written once as `fn` in the gather / index_add form, usable with _grad_ref.evaluate (the expression is multilinear in
(X, degE, degV, W, dY, v2e, e2v), so its mass is the same expression on absolute values), and once in closed form,
`scale_grads`:

    S[e] = sum_{p=(e,u)} v2e[p] X[u],  P[v] = degV[v] dY[v],  Ge[e] = sum_{p=(e,v)} e2v[p] P[v],  q[e] = <S[e], Ge[e]>
    dW[e] = q[e] degE[e],   ddegE[e] = q[e] W[e],   ddegV[v] = <dY[v], Z[v]>,  Z = the aggregation without degV

An empty hyperedge takes no part whatever its degE (1 / 0 = inf): its factor is selected away, not multiplied by zero,
so its gradients are exactly 0.  With heads = H the weights are [nnz, H] and column h weighs columns h C .. (h+1) C - 1.
`graph` is an Index: the incidence's two index vectors on the device the float64 tensors live on (the CPU for
_grad_ref.evaluate; a GPU test may keep everything on its device, where float64 sums of a million-entry shape take
milliseconds).
"""
import numpy as np
import torch

F64 = torch.float64


class Index:
    """V[p], E[p]: the vertex and the hyperedge of every H_T entry p, as int64 tensors on `device`."""

    def __init__(self, inc, device="cpu"):
        self.N, self.M = inc.N, inc.M
        self.V = torch.from_numpy(inc.colind.astype(np.int64)).to(device)
        self.E = torch.from_numpy(np.repeat(np.arange(inc.M, dtype=np.int64), np.diff(inc.csrptr))).to(device)
        self.live = torch.bincount(self.E, minlength=inc.M) > 0 if inc.M else torch.zeros(0, dtype=torch.bool, device=device)

    def abs(self):  # no scales inside: the mass is evaluated on the same index vectors
        return self


def _per_column(w, F, heads):
    """An incidence weight [nnz] / [nnz, H] as a factor per gathered element [nnz, F] (or 1.0 for None)."""
    if w is None:
        return 1.0
    return w.reshape(-1, heads).repeat_interleave(F // heads, dim=1)


def _live(graph):
    return graph.live


def v2e_sum(graph, x, w=None, heads=1):
    """S[e] = sum_{p=(e,u)} w[p] x[u]."""
    return torch.zeros(graph.M, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, graph.E, x[graph.V] * _per_column(w, x.shape[1], heads))


def e2v_sum(graph, xe, w=None, heads=1):
    return torch.zeros(graph.N, xe.shape[1], dtype=xe.dtype, device=xe.device).index_add_(0, graph.V, xe[graph.E] * _per_column(w, xe.shape[1], heads))


def edge_factor(graph, degE, W):
    """degE[e] W[e] per hyperedge [M, 1], an absent one being 1; 0 on an empty hyperedge (selected, not multiplied)."""
    s = torch.ones(graph.M, dtype=F64, device=graph.E.device)
    for t in (degE, W):
        if t is not None:
            s = s * torch.where(_live(graph), t.reshape(-1), torch.zeros((), dtype=F64, device=t.device))
    return s.reshape(-1, 1)


def fn(graph, x, degE=None, degV=None, W=None, v2e=None, e2v=None, heads=1):
    """The aggregation with the three scales as inputs."""
    y = e2v_sum(graph, v2e_sum(graph, x, v2e, heads) * edge_factor(graph, degE, W), e2v, heads)
    return y if degV is None else y * degV.reshape(-1, 1)


def fn_linear(graph, x, weight, degE=None, degV=None, W=None):
    """ops.hgnnaggr_linear: Aggr(X . Wlin^T)."""
    return fn(graph, x @ weight.t(), degE, degV, W)


def edge_dot(graph, A, wa, B, wb, heads=1):
    """Plan.hyperedge_dot: out[e] = sum_c (sum_p wa[p, c/C] A[u, c]) (sum_p wb[p, c/C] B[u, c])."""
    return (v2e_sum(graph, A, wa, heads) * v2e_sum(graph, B, wb, heads)).sum(1)


def scale_grads(graph, x, dy, degE=None, degV=None, W=None, v2e=None, e2v=None, heads=1):
    """The closed form: {"degE": ddegE, "degV": ddegV, "W": dW} (None where the scale is absent), each float64."""
    P = dy if degV is None else dy * degV.reshape(-1, 1)
    q = edge_dot(graph, x, v2e, P, e2v, heads)
    live = _live(graph)
    zero = torch.zeros((), dtype=F64, device=q.device)
    partner = lambda t: 1.0 if t is None else torch.where(live, t.reshape(-1), zero)  # noqa: E731
    out = {"degE": None, "degV": None, "W": None}
    if degE is not None:
        out["degE"] = q * partner(W)
    if W is not None:
        out["W"] = q * partner(degE)
    if degV is not None:
        out["degV"] = (dy * fn(graph, x, degE, None, W, v2e, e2v, heads)).sum(1)
    return out


def scale_grad_masses(graph, x, dy, degE=None, degV=None, W=None, v2e=None, e2v=None, heads=1):
    """The same on absolute values: the mass of each gradient."""
    a = lambda t: None if t is None else t.abs()  # noqa: E731
    return scale_grads(graph.abs(), a(x), a(dy), a(degE), a(degV), a(W), a(v2e), a(e2v), heads)
