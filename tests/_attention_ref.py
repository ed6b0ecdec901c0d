"""Float64 reference of the hypergraph attention coefficients (ops.incidence_softmax), the segment sum (ops.incidence_sum) and
the layer built from them (models.HypergraphAttnConv): CPU, plain torch indexing, test infrastructure only.

For the H_T entries p = (e, u) (graph.E[p] = e, graph.V[p] = u, a _grad_ref.Graph):
    raw[p]   = sv[u] + se[e]                 (either may be None: 0)
    s[p]     = leaky_relu(raw[p], slope)     (torch's convention: slope * raw for raw <= 0)
    alpha[p] = exp(s[p] - m_g) / sum_{q in g} exp(s[q] - m_g),   g = p's hyperedge (group "hyperedge") or vertex ("vertex")
"""
import numpy as np
import torch

from _grad_ref import Graph, f64  # noqa: F401
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


def thresholds():
    """The lengths at which the segment kernels change path, from the library's own constants: lane-group width x entries
    kept in registers for each width, the longest row a lane group takes, 256 lanes x entries kept."""
    from hypergef_amd.plan import Plan, make_opts
    inc = toy()
    info = Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True)).segment_info(0)
    return [w * info["keep"] for w in (4, 8, 16)] + [info["long"], 256 * info["keep"]]


def boundary_sizes():
    """Every length 0 .. 70, 255 .. 257, 1023 .. 1025, 5000 and every threshold +-1, ascending."""
    return sorted(set(list(range(0, 71)) + [255, 256, 257, 1023, 1024, 1025, 5000]
                      + [t + d for t in thresholds() for d in (-1, 0, 1)]))


def boundaries():
    return synth._from_sizes(np.random.default_rng(7), 6000, boundary_sizes(), name="boundaries")


# Lane-group width -> the length of the 3000 rows that steer the mean of the rows a lane group walks into that width's
# band (seg_width: mean <= 4 -> 4, <= 8 -> 8, else 16): with the boundary rows the means are 2.85, 6.75 and 12.61.
WIDTH_FILL = {4: 2, 8: 6, 16: 12}


def width_shape(width):
    """The boundary rows, then 3000 rows of WIDTH_FILL[width] members: the hyperedge side runs at `width`; M = 3081 is no
    multiple of 256 / width, so the last workgroup has lane groups without a segment."""
    return synth._from_sizes(np.random.default_rng(7), 6000, boundary_sizes() + [WIDTH_FILL[width]] * 3000,
                             name="widths_%d" % width)


def with_duplicates(inc, frac=0.03, seed=11):
    """`frac` of the incidences listed twice (a vertex listed twice in a hyperedge counts twice)."""
    reps = np.where(np.random.default_rng(seed).random(inc.nnz) < frac, 2, 1)
    eid = np.repeat(np.arange(inc.M), np.diff(inc.csrptr))
    cnt = np.zeros(inc.M + 1, np.int64)
    np.add.at(cnt, eid + 1, reps)
    return synth.Incidence(inc.N, inc.M, np.cumsum(cnt).astype(np.int32), np.repeat(inc.colind, reps).astype(np.int32),
                           name=inc.name + "+dups")


def side_lengths(inc, side):
    """The length of every group of a side."""
    assert side in GROUPS, side
    return np.diff(inc.csrptr) if side == "hyperedge" else np.bincount(inc.colind, minlength=inc.N)


def reaches_every_path(info, lens):
    """None if `lens` holds every threshold of a side cut as `info` (Plan.segment_info) with t - 1 and t + 1, and 0, 1 and
    5000; else what is missing."""
    have = set(int(x) for x in lens)
    want = {0, 1, 5000}
    for t in (info["width"] * info["keep"], info["long"], 256 * info["keep"]):
        want |= {t - 1, t, t + 1}
    return sorted(want - have) or None


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
    sizes = side_lengths(inc, side)
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


# ---- what the GPU tests of the coefficients share -----------------------------------------------------------------------

DEV = "cuda:0"
SENTINEL = -12345.0
SLOPES = (0.2, 1.0)
MODES = ("both", "sv", "se")


class Case:
    """One incidence on the device with its plan, random scores scaled to max |sv| = max |se| = 4 (max |raw| <= 8), a
    signed dalpha and val, and the float64 references the tests share."""

    def __init__(self, hg, inc, name):
        from hypergef_amd.plan import Plan
        self._hg = hg
        self.name = name
        self.inc = inc
        self.ptr, self.ind = torch.from_numpy(inc.csrptr).to(DEV), torch.from_numpy(inc.colind).to(DEV)
        self.plan = Plan.from_tensors(inc.N, self.ptr, self.ind)
        self.graph = Graph(inc)
        g = torch.Generator().manual_seed(21)
        sv, se = torch.randn(inc.N, generator=g), torch.randn(inc.M, generator=g)
        self.sv = (sv * (4.0 / float(sv.abs().max()))).to(DEV)
        self.se = (se * (4.0 / float(se.abs().max()))).to(DEV)
        self.dalpha = torch.randn(inc.nnz, generator=g).to(DEV)
        self.val = torch.randn(inc.nnz, generator=g).to(DEV)
        self.L = {grp: longest(inc, grp) for grp in GROUPS}
        self._ref = {}

    @property
    def h(self):
        """The HyperGraph of the incidence, built when a test first asks for it."""
        if "_h" not in self.__dict__:
            self._h = self._hg.HyperGraph.from_incidence(self.inc, DEV, data_name=self.name, ngs=1 << 30)
        return self._h

    def scores(self, mode):
        return (self.sv if mode != "se" else None), (self.se if mode != "sv" else None)

    def ref(self, mode, group, slope):
        """(alpha, Smax) in float64 from the fp32 scores: computed once, shared by the tests, never modified."""
        key = (mode, group, slope)
        if key not in self._ref:
            sv, se = (f64(t) for t in self.scores(mode))
            raw = raw_score(self.graph, sv, se)
            self._ref[key] = (softmax(self.graph, sv, se, group, slope), float(raw.abs().max()) if raw.numel() else 0.0)
        return self._ref[key]

    def c(self, mode, group, slope):
        """The per-element bound of alpha relative to alpha: (L + 16 + 16 Smax) U (derived in test_attention_gpu.py)."""
        return (self.L[group] + 16 + 16 * self.ref(mode, group, slope)[1]) * U

    def sizes(self, group):
        """(segment id of every H_T entry, length of every segment) of a group."""
        idx, n = index_of(self.graph, group)
        return idx, torch.bincount(idx, minlength=n)


def bits(t):
    return t.contiguous().view(torch.int32)
