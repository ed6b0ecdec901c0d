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
