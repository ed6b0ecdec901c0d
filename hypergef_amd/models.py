"""The reference's hgsys-backend models on this backend.

Mirrors HyperGsys/model/ugsys/{hgnn,unigin,unigcnii}.py and the wrappers
HGsysHGNN / UniGCNII of HyperGsys/model/gnn.py:110-208 (same constructor
arguments, same forward).  Reference defect D5 is fixed where it would crash:
`HyperGsysUniGCNII.forward` uses its `alpha` / `beta` arguments (the reference
reads unset attributes), and `UniGCNII` builds its hgsys layers for
backend 'hgsys' as well as 'ugsys'.

`backend="torch"` builds the same networks on plain `index_add_` (the PyG
formulation, HyperGsys/model/pygnn/hgnn.py:25-38) -- the stand-in for the
PyG / DGL baselines, which cannot be installed offline.  It runs on CPU or GPU.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .ops import HGNNAggr, HGNNAggrLinear, UniGNNConv, UniGNNConvdeg


# ---- hgsys convolutions (model/ugsys/*.py) -----------------------------------

def _variant_of(options):
    return (options or ops.current_options()).variant


def _hyperedge_weight(hyperg, learn):
    """A layer's diagonal hyperedge weight: ones [M] on the hypergraph's device, an nn.Parameter where it is learned."""
    w = torch.ones(hyperg.degE.shape[0]).to(hyperg.device)
    return nn.Parameter(w) if learn else w


class HyperGsysHGNN(nn.Module):
    # `options` (an ops.Options, or None = the caller's current options at every forward) is this backend's
    # addition to the reference's constructor arguments: per-model kernel family / backward rule / linear folding
    # learn_hyperedge_weight=True makes HGNN's diagonal hyperedge weight `Wdiag` an nn.Parameter of ones (in state_dict,
    # moved by the optimizer; its gradient is ops' dW); False is the reference's constant vector of ones.  The gradient
    # reaches Wdiag whatever `first_aggr` says: both branches of forward() run the sum operator (HGNNAggr accepts
    # first_aggr and ignores it, as the reference does), never ops.hgnnaggr_mean / hgnnaggr_max, which give W none
    def __init__(self, hyperg, in_channels, out_channels, first_aggr, heads=1, options=None, learn_hyperedge_weight=False):
        super().__init__()
        self.options = options
        self.W = ops.Linear(in_channels, heads * out_channels, bias=False, options=options)
        self.Wdiag = _hyperedge_weight(hyperg, learn_hyperedge_weight)
        self.heads, self.in_channels, self.out_channels = heads, in_channels, out_channels
        self.hyperg, self.degE, self.degV = hyperg, hyperg.degE, hyperg.degV
        self.first_aggr = first_aggr

    def forward(self, X):
        if _variant_of(self.options) in ("auto", "pull", "fused"):
            # same operator, one pass where that is faster (Options.fuse_linear; two-step otherwise)
            return HGNNAggrLinear(self.hyperg, X, self.W.weight, self.degE, self.degV, self.Wdiag, options=self.options)
        X = self.W(X)
        return HGNNAggr(self.hyperg, X, self.degE, self.degV, self.Wdiag, self.first_aggr, options=self.options)


class HyperGsysUinGINConv(nn.Module):
    def __init__(self, hyperg, in_channels, out_channels, first_aggr, heads=1, options=None):
        super().__init__()
        self.options = options
        self.W = ops.Linear(in_channels, heads * out_channels, bias=False, options=options)
        self.heads, self.in_channels, self.out_channels = heads, in_channels, out_channels
        self.hyperg, self.degE, self.degV = hyperg, hyperg.degE, hyperg.degV
        self.eps = nn.parameter.Parameter(torch.FloatTensor([0]))

    def forward(self, X):
        if _variant_of(self.options) in ("auto", "pull", "fused") and ops.linear_fusion_pays(X.shape[1], self.W.weight.shape[0]):
            # (1 + eps) W(X) + Aggr(W(X)) = ((1 + eps) X + Aggr(X)) . W^T: the whole layer in one pass
            # training: cb stays a device tensor (eps is learned: its gradient flows through cb) and the kernel reads
            # it from device memory -- no read-back, so the whole training step can be captured in a hipGraph;
            # without grad the value is read once per eps update and handed over as a Python float (no extra kernel)
            if torch.is_grad_enabled() and self.eps.requires_grad:
                cb = 1 + self.eps.reshape(())
            else:
                key = (self.eps.data_ptr(), self.eps._version)
                if getattr(self, "_eps_host", (None, 0.0))[0] != key:
                    self._eps_host = (key, float(self.eps.detach()))
                cb = 1.0 + self._eps_host[1]
            return ops.aggr_res_linear(self.hyperg.H_T_csrptr, self.hyperg.H_T_colind, X, self.W.weight,
                                       residual=X, ca=1.0, cb=cb, options=self.options)
        X = self.W(X)
        Xv = UniGNNConv(self.hyperg, X, options=self.options)
        return (1 + self.eps) * X + Xv


class HyperGsysUniGCNII(nn.Module):
    def __init__(self, hyperg, in_channels, out_channels, heads=1, options=None):
        super().__init__()
        self.options = options
        self.W = ops.Linear(in_channels, out_channels, bias=False, options=options)
        self.heads, self.in_channels, self.out_channels = heads, in_channels, out_channels
        self.hyperg, self.degE, self.degV = hyperg, hyperg.degE, hyperg.degV

    def forward(self, X, X0, alpha, beta, relu=False):
        F = X.shape[1]
        if _variant_of(self.options) in ("auto", "pull", "fused") and ops.linear_fusion_pays(F, self.W.weight.shape[0]) \
                and self.W.weight.shape[0] == F:
            # Xi = (1 - alpha) Xv + alpha X0;  (1 - beta) Xi + beta W(Xi) = Xi . ((1 - beta) I + beta W)^T:
            # aggregation, both mixes, the projection and the model's relu in one pass
            if getattr(self, "_eye", None) is None or self._eye.device != X.device:
                self._eye = torch.eye(F, device=X.device, dtype=X.dtype)
            M = torch.lerp(self._eye, self.W.weight, float(beta))  # (1 - beta) I + beta W, one kernel
            return ops.aggr_res_linear(self.hyperg.H_T_csrptr, self.hyperg.H_T_colind, X, M, residual=X0,
                                       ca=1 - alpha, cb=alpha, degE=self.degE, degV=self.degV, relu=relu,
                                       options=self.options)
        Xv = UniGNNConvdeg(self.hyperg, X, self.degE, self.degV, options=self.options)
        Xi = (1 - alpha) * Xv + alpha * X0
        out = (1 - beta) * Xi + beta * self.W(Xi)
        return torch.relu(out) if relu else out


class HyperGsysUniSAGE(nn.Module):
    """UniSAGE, the UniGNN family's member with a choice of aggregator in either hop, next to UniGIN and UniGCNII above:
        Z = lin(X),   Y = Z + reduce_aggr(Z, first_aggr, second_aggr)
    first_aggr reduces the members of every hyperedge, second_aggr the hyperedges of every vertex, each 'sum', 'mean',
    'max' or 'min' (ops.reduce_aggr; no degree scales).  The one parameter is the bias-free linear's weight."""

    def __init__(self, hyperg, in_channels, out_channels, first_aggr="mean", second_aggr="sum", options=None):
        super().__init__()
        for name, r in (("first_aggr", first_aggr), ("second_aggr", second_aggr)):
            if r not in ("sum", "mean", "max", "min"):
                raise ValueError("%s must be 'sum', 'mean', 'max' or 'min', got %r" % (name, r))
        self.options = options
        self.W = ops.Linear(in_channels, out_channels, bias=False, options=options)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.hyperg, self.first_aggr, self.second_aggr = hyperg, first_aggr, second_aggr

    def forward(self, X):
        Z = self.W(X)
        return Z + ops.reduce_aggr(self.hyperg.H_T_csrptr, self.hyperg.H_T_colind, Z, self.first_aggr, self.second_aggr,
                                   options=self.options)


class DynamicHypergraphConv(nn.Module):
    """A layer that rebuilds its hypergraph from its own input, as DHGNN's layers do: hyperedge i = vertex i and its k - 1
    nearest neighbours among the rows of X (detached: the search has no gradient),
        Z = lin(X),   Y = degV . H (degE . (H^T Z))          (HGNNAggr on HyperGraph.from_knn(X, k)),
    or, with probabilistic=True, the same sums weighted by HGNN's exp(-d2 / mean^2) entries on both hops
    (HGNNAggrIncidence with hyperg.knn_weights(m_prob)).  segments: ops.knn's host offsets -- a batch of point sets in
    one tensor, every set its own hypergraph.  The hypergraph of the last forward stays in `hyperg`.
    device_graph=True: the hypergraph never leaves the device -- knn_graph.KnnHypergraph (table, transpose and degrees
    built on the device) and ops.knn_aggr (two gathers over the table, no plan) in place of HyperGraph.from_knn and the
    planned operators; `hyperg` is then the KnnHypergraph.  The same layer, parameter for parameter, and the same sums in
    another order.  With segments=None a forward and backward then waits for the device nowhere and allocates only through
    torch, so the layer can be recorded into a hipGraph (torch.cuda.graph) and the neighbours are searched again on every
    replay.  With segments, ops.knn still waits once for its offsets: such a layer runs eagerly only.  False (the default)
    is the layer above, untouched.  knn_form: ops.knn's `form` -- "dot" searches the same neighbours through the
    matrix-unit prefilter (no segments); with probabilistic=True the weights then use the dot form's mean.
    learn_distances=True (needs probabilistic=True and device_graph=True): the weights exp(-d2 / (m_prob mean)^2) are
    differentiated through d2 = ops.knn_dist(idx, X), so the gradient of X gains the path through the weights of both hops
    -- what a learnable metric needs.  The output keeps its bits; the table is still searched on detached rows (the
    selection has no gradient) and `mean` is a constant of the construction.  No parameter is added, the layer still
    waits nowhere with segments=None and is still recorded into a hipGraph.  False (the default) is the layer above, bit for
    bit, with the same saved tensors.
    After .to(torch.bfloat16), with knn_form="dot" and device_graph=False, the layer runs on bfloat16 rows: the neighbours are
    searched on the bfloat16 input itself (ops.knn's bfloat16 rows: the hypergraph of X.float(), float32 distances), the
    unweighted sums run on the bfloat16 HGNNAggr, and probabilistic=True turns Options.incidence_bf16 = 'rows' on for the
    layer's own HGNNAggrIncidence call, the weights staying float32.  device_graph=True on bfloat16 input still raises
    ops.knn_aggr's TypeError (the table gathers are float32 only), and under knn_form="difference" the search refuses
    bfloat16.  float32 layers are untouched."""

    def __init__(self, in_channels, out_channels, k, probabilistic=False, segments=None, m_prob=1.0, options=None,
                 device_graph=False, knn_form="difference", learn_distances=False):
        super().__init__()
        if not isinstance(k, int) or not 1 <= k <= 64:
            raise ValueError("k must be an integer in 1 .. 64, got %r" % (k,))
        if learn_distances and not (probabilistic and device_graph):
            raise ValueError("learn_distances=True needs probabilistic=True (the distances only enter the weights) and "
                             "device_graph=True (ops.knn_dist and the weight gradient run over the device table)")
        self.learn_distances = bool(learn_distances)
        self.options = options
        self.lin = ops.Linear(in_channels, out_channels, bias=False, options=options)
        self.in_channels, self.out_channels, self.k = in_channels, out_channels, k
        self.probabilistic, self.segments, self.m_prob = probabilistic, segments, m_prob
        self.device_graph = bool(device_graph)
        self.knn_form = knn_form
        self.hyperg = None

    def forward(self, X):
        if self.device_graph:
            from .knn_graph import KnnHypergraph
            hyperg = self.hyperg = KnnHypergraph.build(X, self.k, segments=self.segments, form=self.knn_form)
            if self.learn_distances:
                return hyperg.aggregate(self.lin(X), True, self.m_prob, X=X)
            return hyperg.aggregate(self.lin(X), probabilistic=self.probabilistic, m_prob=self.m_prob)
        from .hypergraph import HyperGraph
        hyperg = self.hyperg = HyperGraph.from_knn(X.detach(), self.k, X.device, segments=self.segments, form=self.knn_form)
        Z = self.lin(X)
        Wdiag = torch.ones(hyperg.num_edges, device=X.device)
        if self.probabilistic:
            w = hyperg.knn_weights(self.m_prob)
            options = self.options
            if Z.dtype == torch.bfloat16:  # bfloat16 rows for this call, as HypergraphAttnConv does; w stays float32
                options = (options if options is not None else ops.current_options()).replace(incidence_bf16="rows")
            return ops.HGNNAggrIncidence(hyperg, Z, w, w, hyperg.degE, hyperg.degV, Wdiag, options=options)
        return HGNNAggr(hyperg, Z, hyperg.degE, hyperg.degV, Wdiag, "sum", options=self.options)


class HypergraphAttnConv(nn.Module):
    """A hypergraph attention layer whose coefficient path runs on this backend's segment kernels.  Single head:
        Z = X W^T,   sv = Z a_v,   se[e] = mean_{u in e} (Z a_e)[u]   (0 for an empty hyperedge),
        alpha = softmax over each group of leaky_relu(sv[u] + se[e], negative_slope)      (ops.incidence_softmax),
        Y = degV . H_alpha (degE . (H_alpha^T Z)) + bias                                  (ops.incidence_aggr).
    group: 'hyperedge' normalises over each hyperedge's members, 'vertex' over each vertex's hyperedges.  Parameters: the
    linear's weight, a_v, a_e [out_channels] and bias [out_channels].
    heads = H > 1: the linear maps to H * out_channels, head h owns columns h C .. (h + 1) C - 1 of Z (C = out_channels),
    a_v / a_e are flat [H * C], sv[u, h] = <Z[u, head h], a_v[head h]>, se the per-head hyperedge mean, alpha [nnz, H], and
    every operator runs once for all heads (heads=H).  The output is [N, H * C] (concat=True) or the mean over the heads
    [N, C]; the bias has the output's width.  heads = 1 is the single-head layer, parameter for parameter.
    dropout = p in (0, 1): in training mode the coefficients are dropped with probability p and the kept ones scaled by
    1 / (1 - p), inside the softmax kernels (ops.incidence_softmax(dropout=p)); the mask follows torch.manual_seed.  No
    parameter and no buffer is added; eval() and dropout = 0.0 are the layer without it.
    score = 'additive' is the layer above.  score = 'dot' is transformer-style attention of every vertex to the hyperedges'
    own embeddings: no a_v / a_e but a second bias-free linear lin_k (in_channels -> H * C), and
        Kv = lin_k(X),   Ke[e] = mean_{u in e} Kv[u]   (0 for an empty hyperedge)                 (ops.incidence_gather),
        logit[p = (e, u), h] = <Z[u, head h], Ke[e, head h]> * C ** -0.5                           (ops.incidence_dot),
        alpha = softmax over each group of leaky_relu(logit, negative_slope)   (ops.incidence_softmax(incidence_score=)),
    and Y as above; negative_slope = 1.0 is the plain softmax of the logits.  Parameters: lin.weight, lin_k.weight, bias.
    learn_hyperedge_weight=True: the aggregation's diagonal hyperedge weight `Wdiag` (ones [M]) is one more nn.Parameter,
    Y = degV . H_alpha (degE . Wdiag . (H_alpha^T Z)); False is the layer above, parameter for parameter.
    fuse_attention=True: softmax and aggregation run as ops.incidence_attention_aggr -- the same output and gradient bits,
    with no alpha [nnz, heads] written, read or kept for the backward -- where that operator applies: score = 'additive' and
    no dropout active (dropout = 0.0, or eval()).  Elsewhere the layer takes the path above without a word.  No parameter
    or buffer is added; False (the default) is the layer above.
    After .to(torch.bfloat16) the layer runs on bfloat16 rows: it turns Options.incidence_bf16 = 'rows' on for its own calls,
    so Z, the hyperedge keys and Y are bfloat16 rows on the library's bf16-row kernels (fp32 sums, one rounding), while
    sv, se, the dot logits and alpha are formed in float32 from the widened Z; a learned Wdiag is widened too.
    fuse_attention=True then takes the composed path (ops.incidence_attention_aggr is float32 only).  float32 layers are
    untouched."""

    def __init__(self, hyperg, in_channels, out_channels, group="hyperedge", negative_slope=0.2, options=None, heads=1,
                 concat=True, dropout=0.0, score="additive", learn_hyperedge_weight=False, fuse_attention=False):
        super().__init__()
        self.fuse_attention = bool(fuse_attention)
        if score not in ("additive", "dot"):
            raise ValueError("score must be 'additive' or 'dot', got %r" % (score,))
        self.score = score
        self.dropout = ops._dropout_p(dropout)
        if group not in ("hyperedge", "vertex"):
            raise ValueError("group must be 'hyperedge' or 'vertex', got %r" % (group,))
        if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
            raise ValueError("heads must be an integer >= 1, got %r" % (heads,))
        self.options, self.group, self.negative_slope = options, group, float(negative_slope)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.heads, self.concat = heads, bool(concat)
        self.lin = ops.Linear(in_channels, heads * out_channels, bias=False, options=options)
        if score == "dot":
            self.lin_k = ops.Linear(in_channels, heads * out_channels, bias=False, options=options)
        else:
            bound = math.sqrt(6.0 / (out_channels + 1))
            self.a_v = nn.Parameter(torch.empty(heads * out_channels).uniform_(-bound, bound))
            self.a_e = nn.Parameter(torch.empty(heads * out_channels).uniform_(-bound, bound))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels if self.concat else out_channels))
        self.hyperg, self.degE, self.degV = hyperg, hyperg.degE, hyperg.degV
        self.Wdiag = _hyperedge_weight(hyperg, learn_hyperedge_weight)
        self._members = hyperg.H_T_colind.long()                                 # vertex of every incidence
        self._inv_size = torch.nan_to_num(hyperg.degE.reshape(-1), posinf=0.0)   # 1 / |e|, 0 for an empty hyperedge

    def _options(self, rows):
        """The layer's options for one call: its own (or the caller's), with bfloat16 feature rows let through where `rows`
        (Z, or the keys' input) is bfloat16."""
        if rows.dtype != torch.bfloat16:
            return self.options
        return (self.options if self.options is not None else ops.current_options()).replace(incidence_bf16="rows")

    def hyperedge_keys(self, X):
        """score = 'dot': the hyperedges' own embeddings Ke [M, H * C], the mean of lin_k(X) over each hyperedge's members."""
        Kv = self.lin_k(X)
        return ops.incidence_gather(self.hyperg.H_T_csrptr, self.hyperg.H_T_colind, Kv, None, to="hyperedge",
                                    scale_a=self._inv_size, options=self._options(Kv))

    def coefficients(self, Z, X=None):
        """alpha for the projected features Z: [nnz], or [nnz, heads]; after dropout where the layer trains with one.
        score = 'dot' needs the layer's input X as well (the keys are projected from it)."""
        ptr, ind = self.hyperg.H_T_csrptr, self.hyperg.H_T_colind
        if self.score == "dot":
            if X is None:
                raise ValueError("score='dot': coefficients(Z, X) needs the layer's input X for the hyperedge keys")
            if Z.dtype == torch.bfloat16:  # both operands bfloat16 rows, the logits float32
                logits = ops.incidence_dot(ptr, ind, Z, self.hyperedge_keys(X), heads=self.heads,
                                           options=self._options(Z)) * self.out_channels ** -0.5
            else:
                logits = ops.incidence_dot(ptr, ind, Z, self.hyperedge_keys(X), heads=self.heads) * self.out_channels ** -0.5
            return ops.incidence_softmax(ptr, ind, None, None, group=self.group, negative_slope=self.negative_slope,
                                         options=self.options, num_nodes=Z.shape[0], heads=self.heads, dropout=self.dropout,
                                         training=self.training, incidence_score=logits)
        sv, se = self.scores(Z)
        if self.heads == 1:
            return ops.incidence_softmax(ptr, ind, sv, se, group=self.group, negative_slope=self.negative_slope,
                                         options=self.options, num_nodes=Z.shape[0], dropout=self.dropout,
                                         training=self.training)
        return ops.incidence_softmax(ptr, ind, sv, se, group=self.group, negative_slope=self.negative_slope,
                                     options=self.options, num_nodes=Z.shape[0], heads=self.heads, dropout=self.dropout,
                                     training=self.training)

    def scores(self, Z):
        """score = 'additive': (sv [N] / [N, heads], se [M] / [M, heads]) for the projected features Z."""
        ptr, ind = self.hyperg.H_T_csrptr, self.hyperg.H_T_colind
        if Z.dtype == torch.bfloat16:  # the scores are float32, from the widened rows and vectors
            return self._scores(Z.float(), self.a_v.float(), self.a_e.float())
        return self._scores(Z, self.a_v, self.a_e)

    def _scores(self, Z, a_v, a_e):
        ptr, ind = self.hyperg.H_T_csrptr, self.hyperg.H_T_colind
        if self.heads == 1:
            sv = Z @ a_v
            ze = (Z @ a_e)[self._members]
            se = ops.incidence_sum(ptr, ind, ze, side="hyperedge", num_nodes=Z.shape[0]) * self._inv_size
            return sv, se
        H, C = self.heads, self.out_channels
        Zh = Z.view(Z.shape[0], H, C)
        sv = (Zh * a_v.view(H, C)).sum(-1)
        ze = (Zh * a_e.view(H, C)).sum(-1)[self._members]
        se = ops.incidence_sum(ptr, ind, ze, side="hyperedge", num_nodes=Z.shape[0], heads=H) * self._inv_size.reshape(-1, 1)
        return sv, se

    def forward(self, X):
        Z = self.lin(X)
        if self.fuse_attention and self.score == "additive" and not (self.dropout > 0.0 and self.training) \
                and Z.dtype == torch.float32:
            sv, se = self.scores(Z)
            Y = ops.incidence_attention_aggr(self.hyperg.H_T_csrptr, self.hyperg.H_T_colind, Z, sv, se, group=self.group,
                                             negative_slope=self.negative_slope, degE=self.degE, degV=self.degV,
                                             W=self.Wdiag, heads=self.heads, options=self.options)
            if self.heads > 1 and not self.concat:
                Y = Y.view(Y.shape[0], self.heads, self.out_channels).mean(1)
            return Y + self.bias
        alpha = self.coefficients(Z, X)
        Wdiag = self.Wdiag.float() if Z.dtype == torch.bfloat16 else self.Wdiag  # the scales stay float32
        Y = ops.incidence_aggr(self.hyperg.H_T_csrptr, self.hyperg.H_T_colind, Z, alpha, alpha, self.degE, self.degV,
                               Wdiag, options=self._options(Z), heads=self.heads)
        if self.heads > 1 and not self.concat:
            Y = Y.view(Y.shape[0], self.heads, self.out_channels).mean(1)
        return Y + self.bias


# ---- torch index_add baseline (model/pygnn/*.py formulas) ---------------------

class _TorchGraph:
    """Gather/scatter form of the incidence: V, E index vectors (hypergraph.py:30-32)."""

    def __init__(self, hyperg, device):
        inc = hyperg._host
        import numpy as np
        E = np.repeat(np.arange(inc.M, dtype=np.int64), np.diff(inc.csrptr))
        self.V = torch.from_numpy(inc.colind.astype(np.int64)).to(device)
        self.E = torch.from_numpy(E).to(device)
        self.N, self.M = inc.N, inc.M
        self.degE = hyperg.degE.to(device)
        self.degV = hyperg.degV.to(device)

    def v2e(self, X):
        return torch.zeros(self.M, X.shape[1], dtype=X.dtype, device=X.device).index_add_(0, self.E, X[self.V])

    def e2v(self, Xe):
        return torch.zeros(self.N, Xe.shape[1], dtype=Xe.dtype, device=Xe.device).index_add_(0, self.V, Xe[self.E])


class TorchHGNNConv(nn.Module):
    def __init__(self, tg, in_channels, out_channels, first_aggr, heads=1):
        super().__init__()
        self.linear = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.tg = tg

    def forward(self, X):
        X = self.linear(X)
        Xe = self.tg.v2e(X) * torch.nan_to_num(self.tg.degE, posinf=0.0)
        return self.tg.e2v(Xe) * self.tg.degV


class TorchGINConv(nn.Module):
    def __init__(self, tg, in_channels, out_channels, first_aggr, heads=1):
        super().__init__()
        self.W = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.eps = nn.parameter.Parameter(torch.FloatTensor([0]))
        self.tg = tg

    def forward(self, X):
        X = self.W(X)
        return (1 + self.eps) * X + self.tg.e2v(self.tg.v2e(X))


class TorchGCNIIConv(nn.Module):
    def __init__(self, tg, in_channels, out_channels, heads=1):
        super().__init__()
        self.W = nn.Linear(in_channels, out_channels, bias=False)
        self.tg = tg

    def forward(self, X, X0, alpha, beta):
        Xe = self.tg.v2e(X) * torch.nan_to_num(self.tg.degE, posinf=0.0)
        Xv = self.tg.e2v(Xe) * self.tg.degV
        Xi = (1 - alpha) * Xv + alpha * X0
        return (1 - beta) * Xi + beta * self.W(Xi)


__hgsys_convs__ = {"UniGIN": HyperGsysUinGINConv, "HGNN": HyperGsysHGNN}
__torch_convs__ = {"UniGIN": TorchGINConv, "HGNN": TorchHGNNConv}


# ---- networks (model/gnn.py) -----------------------------------------------------

class HGsysHGNN(nn.Module):
    """model/gnn.py:110-134; `args` needs .model, .activation, .input_drop, .dropout
    (and .backend: 'hgsys' or 'torch')."""

    def __init__(self, args, hyperg, nfeat, nhid, nclass, nlayer, first_aggr, nhead):
        super().__init__()
        if getattr(args, "backend", "hgsys") == "torch":
            Conv, g = __torch_convs__[args.model], _TorchGraph(hyperg, getattr(args, "device", hyperg.device))
        else:
            import functools
            # args.options (an ops.Options) pins this model's kernel family / backward rule / linear folding
            Conv, g = functools.partial(__hgsys_convs__[args.model], options=getattr(args, "options", None)), hyperg
            if args.model == "HGNN" and getattr(args, "learn_hyperedge_weight", False):  # HGNN's own diagonal W, trained
                Conv = functools.partial(Conv, learn_hyperedge_weight=True)
        self.conv_out = Conv(g, nhid * nhead, nclass, first_aggr, nhead)
        self.convs = nn.ModuleList([Conv(g, nfeat, nhid, first_aggr, nhead)] +
                                   [Conv(g, nhid * nhead, nhid, first_aggr, nhead) for _ in range(nlayer - 2)])
        self.act = {"relu": nn.ReLU(), "leaky_relu": nn.LeakyReLU()}[args.activation]
        self.input_drop = nn.Dropout(args.input_drop)
        self.dropout = nn.Dropout(args.dropout)

    def forward(self, X):
        X = self.input_drop(X)
        for conv in self.convs:
            X = self.dropout(self.act(conv(X)))
        return F.log_softmax(self.conv_out(X), dim=1)


class UniGCNII(nn.Module):
    """model/gnn.py:137-208."""

    def __init__(self, args, hyperg, nfeat, nhid, nclass, nlayer, nhead):
        super().__init__()
        nhid = nhid * nhead
        self.act = {"relu": nn.ReLU(), "prelu": nn.PReLU()}[args.activation]
        self.input_drop = nn.Dropout(args.input_drop)
        self.dropout = nn.Dropout(args.dropout)
        if getattr(args, "backend", "hgsys") == "torch":
            lin = nn.Linear
        else:  # same module, own wgrad kernel, under the model's options like its conv layers
            lin = lambda i, o: ops.Linear(i, o, options=getattr(args, "options", None))
        self.convs = nn.ModuleList([lin(nfeat, nhid)])
        if getattr(args, "backend", "hgsys") == "torch":
            tg = _TorchGraph(hyperg, getattr(args, "device", hyperg.device))
            self.convs.extend(TorchGCNIIConv(tg, nhid, nhid) for _ in range(nlayer))
        else:
            self.convs.extend(HyperGsysUniGCNII(hyperg, nhid, nhid, options=getattr(args, "options", None))
                              for _ in range(nlayer))
        self.convs.append(lin(nhid, nclass))
        self.reg_params = list(self.convs[1:-1].parameters())
        self.non_reg_params = list(self.convs[0:1].parameters()) + list(self.convs[-1:].parameters())

    def forward(self, x):
        lamda, alpha = 0.5, 0.1
        x = self.dropout(x)
        x = F.relu(self.convs[0](x))
        x0 = x
        for i, con in enumerate(self.convs[1:-1]):
            x = self.dropout(x)
            beta = math.log(lamda / (i + 1) + 1)
            if isinstance(con, HyperGsysUniGCNII):
                x = con(x, x0, alpha, beta, relu=True)  # the relu rides in the layer's epilogue
            else:
                x = F.relu(con(x, x0, alpha, beta))
        x = self.dropout(x)
        return F.log_softmax(self.convs[-1](x), dim=1)
