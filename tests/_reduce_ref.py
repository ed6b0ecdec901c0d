"""Exact reference of the max / min row gathers and of their gradient (plain torch, any device): test infrastructure only.

A hop reduces, for every row of one side of the incidence and every column, the source rows of the row's entries:
hop 0 the members of a hyperedge (the rows of H_T, positions p in indices_t order), hop 1 the hyperedges of a vertex.
The winner is the entry with the greatest (smallest) value under > (<) -- so -0.0 ties +0.0 -- and among ties the one with
the smallest position in indices_t; an empty row has none (arg = -1, value +0.0).  The gradient goes to the winner only:
not torch's amax rule, which shares it among ties.
"""
import numpy as np
import torch


def entries(inc, device="cpu"):
    """(row_e, row_v): for every position p of indices_t its hyperedge and its vertex, int64 [nnz]."""
    E = torch.from_numpy(np.repeat(np.arange(inc.M, dtype=np.int64), np.diff(inc.csrptr))).to(device)
    V = torch.from_numpy(inc.colind.astype(np.int64)).to(device)
    return E, V


def reduce_hop(inc, hop, src, op, E=None, V=None):
    """(value, arg) of one hop on src ([N, F] for hop 0, [M, F] for hop 1; any float dtype, compared as it is).
    value [rows, F] is src[ind[arg]] itself (+0.0 for an empty row), arg int64 [rows, F] (-1 for an empty row)."""
    if E is None:
        E, V = entries(inc, src.device)
    rows, other, nrows = (E, V, inc.M) if hop == 0 else (V, E, inc.N)
    F = src.shape[1]
    nnz = rows.numel()
    vals = src[other]  # [nnz, F]: the value every position offers
    if nnz == 0:
        return torch.zeros(nrows, F, dtype=src.dtype, device=src.device), torch.full((nrows, F), -1, dtype=torch.int64, device=src.device)
    idx = rows.reshape(-1, 1).expand(nnz, F)
    start = float("-inf") if op == "max" else float("inf")
    best = torch.full((nrows, F), start, dtype=src.dtype, device=src.device)
    best = best.scatter_reduce(0, idx, vals, "amax" if op == "max" else "amin", include_self=True)
    # the smallest position whose value equals the row's best (== : -0.0 equals +0.0)
    pos = torch.arange(nnz, dtype=torch.int64, device=src.device).reshape(-1, 1).expand(nnz, F)
    cand = torch.where(vals == best[rows], pos, torch.full_like(pos, nnz))
    arg = torch.full((nrows, F), nnz, dtype=torch.int64, device=src.device).scatter_reduce(0, idx, cand, "amin", include_self=True)
    empty = arg == nnz
    safe = arg.clamp(max=nnz - 1)
    value = torch.gather(vals, 0, safe)
    value = torch.where(empty, torch.zeros_like(value), value)
    return value, torch.where(empty, torch.full_like(arg, -1), arg)


def select_grad(inc, hop, gs, arg, E=None, V=None):
    """dsrc of reduce_hop(hop): gs [rows, F] (float64 for an exact answer) lands on the source row of the winner, once."""
    if E is None:
        E, V = entries(inc, gs.device)
    other, nsrc = (V, inc.N) if hop == 0 else (E, inc.M)
    F = gs.shape[1]
    out = torch.zeros(nsrc, F, dtype=gs.dtype, device=gs.device)
    won = arg >= 0
    if not bool(won.any()):
        return out
    src_row = other[arg.clamp(min=0)]  # [rows, F]
    cols = torch.arange(F, device=gs.device).reshape(1, -1).expand_as(arg)
    out.index_put_((src_row[won], cols[won]), gs[won], accumulate=True)
    return out


class Reduce64(torch.autograd.Function):
    """One max / min hop in float64 with the winner-only gradient above.  g: a graph object with inc, E, V (entries(), on
    src's device).  winners: a list; empty, it receives this hop's arg; holding one, that arg is used instead of a
    comparison -- the mass pass, on absolute values, must follow the winners of the real pass."""

    @staticmethod
    def forward(ctx, src, g, hop, op, winners):
        if winners:
            arg = winners[0]
            cols = torch.arange(src.shape[1], device=src.device).reshape(1, -1).expand_as(arg)
            val = src[(g.V if hop == 0 else g.E)[arg.clamp(min=0)], cols]
            val = torch.where(arg < 0, torch.zeros_like(val), val)
        else:
            val, arg = reduce_hop(g.inc, hop, src, op, g.E, g.V)
            winners.append(arg)
        ctx.g, ctx.hop, ctx.arg = g, hop, arg
        return val

    @staticmethod
    def backward(ctx, grad):
        return select_grad(ctx.g.inc, ctx.hop, grad, ctx.arg, ctx.g.E, ctx.g.V), None, None, None, None


def hop64(g, hop, src, op, winners):
    """One hop in float64: max / min as Reduce64, or the plain sum / mean (g.len[hop]: the rows' lengths)."""
    if op in ("max", "min"):
        return Reduce64.apply(src, g, hop, op, winners)
    rows, other = (g.E, g.V) if hop == 0 else (g.V, g.E)
    ndst = g.inc.M if hop == 0 else g.inc.N
    out = torch.zeros(ndst, src.shape[1], dtype=src.dtype, device=src.device).index_add(0, rows, src[other])
    return out / g.len[hop].clamp(min=1).reshape(-1, 1).to(src.dtype) if op == "mean" else out


def reduce_aggr64(g, x, first, second, degE=None, degV=None, W=None, winners=None):
    """ops.reduce_aggr in float64: Xe = ((first over members) * degE) * W, Y = (second over hyperedges) * degV; the scales
    float64 vectors on x's device or None; winners = (list, list) as hop64 takes them for hop 0 and hop 1."""
    win = winners if winners is not None else ([], [])
    xe = hop64(g, 0, x, first, win[0])
    for s in (degE, W):
        if s is not None:
            xe = xe * s.reshape(-1, 1)
    y = hop64(g, 1, xe, second, win[1])
    return y if degV is None else y * degV.reshape(-1, 1)


# ---- what the schedule tests share (test_reduce_schedules_host.py, test_reduce_schedules.py) ----------------------------
# The max / min row gather and its select-gather on every plan schedule: the cells (graph x plan-option set of
# _incidence_ref), the widths, and the inputs, drawn on the host so that the CPU file sees what the GPU file runs.

CORE_WIDTHS = (1, 3, 4, 33, 64, 65, 260)  # on every cell; 65: the first 4-byte-lane width with two column tiles
# On SWEEP_CELLS only.  2, 6, 13, 21 complete the 4-byte lanes' LPR = 2, 8, 16, 32; 16 and 256 are 16-byte lanes of LPR 4 and
# 64; 8, 32, 128 are the 16-byte lanes' LPR = 2, 8, 32, which no other width instantiates (lane_shape;
# test_reduce_schedules_host.test_widths_instantiate_every_lane_shape).
SWEEP_WIDTHS = (2, 6, 13, 21, 16, 256, 8, 32, 128)
FMAX = max(CORE_WIDTHS + SWEEP_WIDTHS)
OPS = ("max", "min")
KINDS = ("randn", "ties", "inf", "const")
SWEEP_KINDS = ("randn", "ties")
SELECT_WINNERS = (("max", "ties"), ("min", "randn"), ("max", "inf"))  # whose reference arg the select-gather is given
REDUCE_SETS = ("default", "lat", "small", "unit", "odd", "dfs")
WIDE_GRAPHS = ("ragged", "boundaries")
SWEEP_CELLS = (("ragged", "wide"), ("boundaries", "small"), ("boundaries_T", "small"))
PIN_GRAPHS = ("toy", "ragged", "boundaries")
PIN_MASKS = (0, 4, 8, 5, 7)  # k0 + 3 * k1: kinds (0, 0), (1, 1), (2, 2), (2, 1), (1, 2)
PIN_WIDTHS = (4, 33)
PAIR_GRAPHS = ("ragged", "boundaries_T")
PAIR_WIDTHS = (4, 33)
PAIR_REDUCES = ("sum", "mean", "max", "min")
MISALIGNED_F = 8          # once per cell, rows offset by 4 bytes: 4-byte lanes of LPR 8
MISALIGNED_TILES_F = 128  # once on MISALIGNED_TILES_CELL: 4-byte lanes, two column tiles
MISALIGNED_TILES_CELL = ("ragged", "small")


def cells():
    """Every (graph, option set) the forward and select checks run on: `wide` only on WIDE_GRAPHS."""
    import _incidence_ref as ir
    return [(g, s) for g in ir.GRAPHS for s in REDUCE_SETS] + [(g, "wide") for g in WIDE_GRAPHS]


def widths_on(graph, opts):
    """The widths a cell is run at (aligned rows)."""
    return CORE_WIDTHS + (SWEEP_WIDTHS if (graph, opts) in SWEEP_CELLS else ())


def lane_shape(F, aligned=True):
    """(VEC, LPR, column tiles) of a call of width F, by reduce_hop's and launch_gather_reduce's rule (hg_api.hip,
    hg_kernels.hip): 16-byte lanes where F % 4 == 0 and the rows are 16-byte aligned, else 4-byte lanes."""
    vec = 4 if (F % 4 == 0 and aligned) else 1
    lanes = F // vec
    lpr = 1
    while lpr < min(lanes, 64):
        lpr *= 2
    return vec, lpr, -(-lanes // lpr)


def row_lengths(inc):
    """(hyperedge sizes [M], vertex degrees [N]), int64 numpy: the rows of hop 0 and of hop 1."""
    return np.diff(inc.csrptr).astype(np.int64), np.bincount(inc.colind, minlength=inc.N).astype(np.int64)


def all_inf_row(inc, hop):
    """The first destination row of at least two entries: the 'inf' input makes all its entries -inf."""
    return int(np.nonzero(row_lengths(inc)[hop] >= 2)[0][0])


def draw(inc, hop, kind):
    """The source rows of one hop ([N, FMAX] for hop 0, [M, FMAX] for hop 1; a call takes the first F columns), float32
    numpy.  randn; ties: -0.0 or +0.0, and in column j each of -1 and 1 with probability 4^-(1 + j % 6); inf: randn with 5 % +inf, 5 % -inf and every entry of
    all_inf_row -inf; const: 1.0 everywhere."""
    nsrc = inc.N if hop == 0 else inc.M
    rng = np.random.default_rng(100 + 10 * hop + KINDS.index(kind))
    if kind == "const":
        return np.ones((nsrc, FMAX), np.float32)
    if kind == "ties":  # the extremes grow rarer from column to column, so that in long rows too the best value is met late
        x = rng.choice(np.array([-0.0, 0.0], np.float32), size=(nsrc, FMAX))
        u = rng.random(x.shape)
        p = 0.25 ** (1 + np.arange(FMAX) % 6)
        x[u < p] = 1.0
        x[u > 1 - p] = -1.0
        return x
    x = rng.standard_normal((nsrc, FMAX)).astype(np.float32)
    if kind == "inf":
        u = rng.random(x.shape)
        x[u < 0.05] = np.inf
        x[u > 0.95] = -np.inf
        E = np.repeat(np.arange(inc.M), np.diff(inc.csrptr))
        rows, other = (E, inc.colind) if hop == 0 else (inc.colind, E)
        x[other[rows == all_inf_row(inc, hop)]] = -np.inf
    return x


def first_positions(inc, hop):
    """The smallest indices_t position of every row of a hop (-1: empty row), int64 numpy: the winner of a constant input."""
    lens = row_lengths(inc)[hop]
    if hop == 0:
        first = inc.csrptr[:-1].astype(np.int64)
    else:
        first = np.full(inc.N, inc.nnz, np.int64)
        np.minimum.at(first, inc.colind, np.arange(inc.nnz, dtype=np.int64))
    return np.where(lens > 0, first, -1)


def pair_inputs(inc, F, seed=31):
    """(X [N, F] integers in -3 .. 3, dY [N, F] integers in -2 .. 2), float32 numpy: with _incidence_ref.power_of_two_scales no
    sum of reduce_aggr without a mean rounds (test_reduce_schedules_host.test_pair_inputs_stay_exact_in_fp32)."""
    rng = np.random.default_rng(seed + F)
    return rng.integers(-3, 4, (inc.N, F)).astype(np.float32), rng.integers(-2, 3, (inc.N, F)).astype(np.float32)


def brute_force(inc, hop, src, op):
    """The definition as two Python loops (numpy): tiny graphs only."""
    src = np.asarray(src)
    rows = np.repeat(np.arange(inc.M), np.diff(inc.csrptr))
    cols = inc.colind
    own, other, nrows = (rows, cols, inc.M) if hop == 0 else (cols, rows, inc.N)
    F = src.shape[1]
    value = np.zeros((nrows, F), src.dtype)
    arg = np.full((nrows, F), -1, np.int64)
    for r in range(nrows):
        for c in range(F):
            for p in range(len(own)):  # ascending positions: a strict comparison keeps the smallest among ties
                if own[p] != r:
                    continue
                x = src[other[p], c]
                if arg[r, c] < 0 or (x > value[r, c] if op == "max" else x < value[r, c]):
                    value[r, c], arg[r, c] = x, p
    return value, arg
