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
    xe = torch.zeros(graph.M, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, graph.E, xs)
    if graph.se is not None:
        xe = xe * graph.se.reshape(-1, 1)
    ys = xe[graph.E]
    if e2v is not None:
        ys = ys * e2v.reshape(-1, 1)
    y = torch.zeros(graph.N, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, graph.V, ys)
    return y if graph.degV is None else y * graph.degV.reshape(-1, 1)


def hop1(graph, x, v2e=None):
    """Xe = De W H_v2e^T x: hop 1 of incidence_aggr alone."""
    xs = x[graph.V] if v2e is None else x[graph.V] * v2e.reshape(-1, 1)
    xe = torch.zeros(graph.M, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, graph.E, xs)
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


# ---- what the schedule tests share (test_incidence_schedules_host.py, test_incidence_schedules.py) ----------------------
# The weighted row gathers on every plan schedule: the plan-option sets, the graphs, the widths and the inputs whose every
# partial sum is an integer below 2^24 (exact in fp32 in any order).

LDS_BYTES = 160 * 1024  # what aggr_incidence (hg_api.hip) allows a workgroup: gfx950's LDS per CU
PANEL_NNZ_MAX = 16384   # resolve_opts' limit of panel_nnz
WIDTHS = (1, 3, 4, 33, 64)                 # single head
PAIRS = ((2, 6), (4, 3), (4, 8), (8, 40))  # (H, C): F % 4 == 0 but C % 4 != 0 twice; 16-byte lanes; two column tiles
EXACT_PAIRS = ((4, 3), (8, 40))


def lat_short_max():
    """kLatShortMax, the latency schedule's cut (hg_plan::sched_lat), from the library's own source: no entry of the C ABI
    reports it, so it is read where it is defined, hypergef_amd/csrc/hg_internal.h."""
    import os
    import re
    import hypergef_amd
    header = os.path.join(os.path.dirname(os.path.abspath(hypergef_amd.__file__)), "csrc", "hg_internal.h")
    found = re.findall(r"constexpr\s+int\s+kLatShortMax\s*=\s*(\d+)\s*;", open(header).read())
    assert len(found) == 1, "kLatShortMax is not defined once in %s" % header
    return int(found[0])


def weighted_lds_bytes(panel_rows, panel_nnz):
    """The LDS a weighted panel workgroup needs: the formula of aggr_incidence's refusal and of launch_gather_t."""
    return (4 * panel_rows + 1 + 2 * panel_nnz) * 4


def wide_panel_rows(panel_nnz=PANEL_NNZ_MAX):
    """The largest panel_rows the weighted entry accepts beside panel_nnz; the next one up is refused."""
    rows = (LDS_BYTES // 4 - 1 - 2 * panel_nnz) // 4
    assert weighted_lds_bytes(rows, panel_nnz) <= LDS_BYTES < weighted_lds_bytes(rows + 1, panel_nnz)
    return rows


def option_sets():
    """name -> keyword arguments of make_opts (the tests add row_stream=False, the host test host_only=True)."""
    small = dict(short_max=6, split_len=8, panel_rows=16, panel_nnz=32)
    return {
        "default": dict(),
        "lat": dict(short_max=lat_short_max()),
        "small": small,
        "unit": dict(short_max=1, split_len=1, panel_rows=1, panel_nnz=1),
        "odd": dict(short_max=4, split_len=7, panel_rows=3, panel_nnz=9, xcd_remap=False),
        "dfs": dict(dfs_order=True, **small),
        "wide": dict(panel_rows=wide_panel_rows(), panel_nnz=PANEL_NNZ_MAX),
    }


OPTION_SETS = ("default", "lat", "small", "unit", "odd", "dfs", "wide")


def _schedule_graphs():
    import _attention_ref as ar  # imports this module: not at the top
    from hypergef_amd import synth
    ragged = lambda: synth.random_incidence(3000, 2000, 6.0, seed=4, empty_frac=0.1)  # noqa: E731
    return {
        "toy": ar.toy,
        "ragged": ragged,
        "boundaries": ar.boundaries,
        "boundaries_T": lambda: ar.transpose(ar.boundaries()),
        "ragged+dups": lambda: ar.with_duplicates(ragged()),
        "powerlaw": lambda: synth.powerlaw(5000, 20000),
    }


GRAPHS = ("toy", "ragged", "boundaries", "boundaries_T", "ragged+dups", "powerlaw")


def schedule_graph(name):
    return _schedule_graphs()[name]()


def graph_on(graph, device):
    """A copy of a _grad_ref.Graph with its index and scale vectors on `device`: incidence_aggr and hop1 (and through them
    _heads_ref.incidence_aggr) then run there on float64 tensors of that device -- the same formulas; index_add_ adds in
    an arbitrary order on a GPU, which float64 makes immaterial at fp32 bounds (2^-53 against 2^-24 of the mass)."""
    g = graph.__class__.__new__(graph.__class__)
    g.__dict__.update(graph.__dict__)
    for k in ("V", "E", "degE", "degV", "W", "se"):
        if getattr(g, k) is not None:
            setattr(g, k, getattr(g, k).to(device))
    g._abs = None
    return g


def integer_inputs(inc, F, heads=1, seed=17):
    """(X [N, F], v2e, e2v [nnz] or [nnz, heads]) as float32 numpy arrays with X in {-1, 0, 1} and weights in {-2 .. 2}:
    every product and, while the mass stays below 2^24 (exact_mass), every partial sum in any order is an integer fp32
    holds exactly."""
    import numpy as np
    rng = np.random.default_rng(seed)
    shape = (inc.nnz,) if heads == 1 else (inc.nnz, heads)
    X = rng.integers(-1, 2, (inc.N, F)).astype(np.float32)
    return X, rng.integers(-2, 3, shape).astype(np.float32), rng.integers(-2, 3, shape).astype(np.float32)


def exact_mass(graph, X, v2e, e2v, heads=1):
    """(max over hop 1's table, max over Y) of the sums of absolute values, in float64: max_e sum_{u in e} |v2e| |X| and
    max_v sum_{e with v} |e2v| sum_{u in e} |v2e| |X|.  `graph`: a _grad_ref.Graph without scales."""
    x, a, b = (f64(t).abs() for t in (X, v2e, e2v))
    C = x.shape[1] // heads
    top = [0.0, 0.0]
    for h in range(heads):
        wa, wb = (a, b) if heads == 1 else (a[:, h], b[:, h])
        xe = hop1(graph, x[:, h * C:(h + 1) * C], wa)
        y = torch.zeros(graph.N, C, dtype=F64).index_add_(0, graph.V, xe[graph.E] * wb.reshape(-1, 1))
        top = [max(top[0], float(xe.max()) if xe.numel() else 0.0), max(top[1], float(y.max()) if y.numel() else 0.0)]
    return tuple(top)


# ---- what the hop-kernel tests share (test_hop_kernels_host.py, test_hop_kernels_gpu.py) ---------------------------------
# The pull variant's three kernels per hop, named by Plan.pin: k = 0 streaming row gather, 1 row panels + wave tasks on the
# plan's schedule, 2 the same kernel on the latency schedule; a mask is k0 + 3 * k1 (hg_tune_info).

HOP_OPTION_SETS = ("default", "wide", "dfs", "small", "odd")
# what each set's short_max means for graphs of at most 2^18 incidences: `dfs` carries `small`'s short_max = 6
HOP_SETS_WITH_LAT = {"default": True, "wide": True, "dfs": False, "small": False, "odd": False}
HOP_WIDTHS = (1, 3, 4, 8, 12, 20, 33, 64, 128, 260)
LAT_NNZ_MAX = 1 << 18  # plan_build (hg_api.hip): larger graphs get no latency schedule


def hop_masks(has_lat):
    """The masks Plan.pin accepts on a plan with / without a latency schedule: all nine, or the four of kinds 0 and 1."""
    kinds = (0, 1, 2) if has_lat else (0, 1)
    return tuple(k0 + 3 * k1 for k1 in kinds for k0 in kinds)


def expect_latency_schedule(nnz, short_max):
    """The rule as plan_build states it, on the resolved short_max (Plan.info)."""
    return nnz <= LAT_NNZ_MAX and short_max > lat_short_max()


def power_of_two_scales(inc, seed=23):
    """(degE [M], degV [N], W [M]) float32 numpy: degE, degV in {0.25, 0.5, 1}, W in {0.5, 1, 2}.  Multiplying by them is
    exact, so integer sums stay exact: hop 1's table is a multiple of 2^-3 of magnitude at most 2 * mass, Y a multiple of
    2^-5 of magnitude at most 2 * mass."""
    import numpy as np
    rng = np.random.default_rng(seed)
    pick = lambda n, vals: np.asarray(vals, np.float32)[rng.integers(0, len(vals), n)]  # noqa: E731
    return pick(inc.M, (0.25, 0.5, 1.0)), pick(inc.N, (0.25, 0.5, 1.0)), pick(inc.M, (0.5, 1.0, 2.0))


SCALE_PRODUCT_MAX = 2.0    # degE * W at most 1 * 2 (degV at most 1)
SCALE_GRANULE = 2.0 ** -3  # degE * W at least 0.25 * 0.5: every term of hop 2's sums is a multiple of it


def unweighted_mass_bound(inc):
    """exact_mass for unit incidence weights and |X| = 1 everywhere: (max hyperedge size, max over vertices of the summed
    sizes of their hyperedges).  It bounds the mass of any X in {-1, 0, 1} at any width."""
    import numpy as np
    import _grad_ref as gr
    one = np.ones(inc.nnz, np.float32)
    return exact_mass(gr.Graph(inc), np.ones((inc.N, 1), np.float32), one, one)


def within_on_device(got, ref, mass, c, what=""):
    """_grad_ref.assert_within's bound, |got - ref| <= c * max(mass, TINY) per element with non-finite values outside,
    decided on the tensors' device; only a failure goes through assert_within (on the host) for its message.  Returns the
    largest |got - ref| / max(mass, TINY)."""
    import _grad_ref as gr
    assert tuple(got.shape) == tuple(ref.shape), "%s: shape %s, want %s" % (what, tuple(got.shape), tuple(ref.shape))
    if got.numel() == 0:
        return 0.0
    err, floor = (got.double() - ref).abs(), mass.clamp(min=TINY)
    if not (bool(torch.isfinite(got).all()) and bool((err <= c * floor).all())):  # bad_elements' expression
        gr.assert_within(got, ref, mass, c, what)
        raise AssertionError("%s: outside %g of the mass on the device, inside on the host" % (what, c))
    return float((err / floor).max())
