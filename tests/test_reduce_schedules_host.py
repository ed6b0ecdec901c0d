"""CPU-only: what the matrix of test_reduce_schedules.py (graphs x plan-option sets x widths x inputs) reaches inside
gather_rows_reduce_kernel and fixup_rows_reduce_kernel, read from host-only plans and the host-drawn inputs of _reduce_ref.

a. For every lane-group width LPR in {1 .. 64} a tested (cell, hop) has a panel of more than 256 / LPR rows -- the only
   case in which a lane group walks more than one row -- holding two adjacent non-empty rows inside one group's range
   (rpg = ceil(nrows / (256 / LPR)) rows per group) and an empty row that is not the panel's first or last; the hop-0
   supplier also has a group that ends with an empty row and a run of empty rows inside a group.  SUPPLIERS names the
   cells, and widths of that LPR with 4-byte and with 16-byte lanes are run on them.
b. The `ties` input puts equal best values across every cut the (value, position) order is applied over: two partial slots
   of a split row, a winner outside the row's first slot, two first-level fixup groups, and two lane groups of a wave task
   at every lane width that has more than one (G = 64 / LPR >= 2: the entries of group g are those at beg + g (mod G)).
c. The width lists instantiate every (VEC, LPR) pair and a 4-byte-lane launch with two column tiles.
d. The integer inputs of the reduce_aggr pairs cannot round: the sums of absolute values behind Xe, Y and dX, with the
   scales' largest product and smallest granule, stay below 2^24.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _incidence_ref as ir  # noqa: E402
import _reduce_ref as rr  # noqa: E402

LPRS = (1, 2, 4, 8, 16, 32, 64)
# LPR -> ((graph, option set) whose hop 0 supplies the multi-row lane groups, the same for hop 1)
SUPPLIERS = {
    1: (("ragged", "wide"), ("ragged", "wide")),
    2: (("ragged", "wide"), ("ragged", "wide")),
    4: (("ragged", "wide"), ("ragged", "wide")),
    8: (("ragged", "wide"), ("ragged", "wide")),
    16: (("ragged", "wide"), ("ragged", "wide")),
    32: (("ragged", "wide"), ("boundaries", "small")),
    64: (("boundaries_T", "small"), ("boundaries", "small")),
}
TIE_CELLS = (("boundaries", 0), ("boundaries_T", 1))  # (graph, hop): the hop whose rows have every length
TIE_SETS = ("small", "unit", "default")
TIE_COLUMNS = 12  # the columns looked at: the first ones, which every width from 33 up runs; two of each rarity of draw()

_PLANS = {}


def _plan(graph, name):
    """(incidence, host-only plan) of a cell of the matrix, built once."""
    from hypergef_amd.plan import Plan, make_opts
    if (graph, name) not in _PLANS:
        inc = ir.schedule_graph(graph)
        opts = make_opts(host_only=True, row_stream=False, **ir.option_sets()[name])
        _PLANS[graph, name] = (inc, Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=opts))
    return _PLANS[graph, name]


def _walked(inc, plan, hop):
    """(ptr, ind, pos) of the CSR hop walks: pos[q] is entry q's position in indices_t (q itself on H_T, perm[q] on H)."""
    if hop == 0:
        return inc.csrptr.astype(np.int64), inc.colind.astype(np.int64), np.arange(inc.nnz, dtype=np.int64)
    ptr, ind = plan.vertex_csr()
    return ptr.astype(np.int64), ind.astype(np.int64), plan.incidence_perm().astype(np.int64)


# ---- a: several rows per lane group ----------------------------------------------------------------------------------------

def _group_features(lens, panels, lpr):
    """What the panels of more than 256 / lpr rows hold, as the kernel cuts them into lane groups."""
    ng = 256 // lpr
    have = set()
    for row0, n, _, _ in panels:
        if n <= ng:
            continue
        have.add("multi_row_panel")
        filled = lens[row0:row0 + n] > 0
        if (~filled[1:-1]).any():
            have.add("interior_empty")
        rpg = -(-n // ng)
        for g in range(ng):
            f = filled[min(g * rpg, n):min((g + 1) * rpg, n)]
            if len(f) < 2:
                continue
            if (f[:-1] & f[1:]).any():
                have.add("adjacent_rows")
            if f.any() and not f[-1]:
                have.add("group_ends_empty")
            if len(f) >= 3 and (~f[:-2] & ~f[1:-1] & f[2:]).any():
                have.add("empty_run")
    return have


def test_suppliers_are_tested_cells_at_widths_of_their_lane_shape():
    assert tuple(sorted(SUPPLIERS)) == LPRS
    for lpr, cells in SUPPLIERS.items():
        for cell in cells:
            assert cell in rr.cells(), cell
            shapes = {rr.lane_shape(F)[:2] for F in rr.widths_on(*cell)}
            assert {(1, lpr), (4, lpr)} <= shapes, "no width of LPR %d with both lane sizes runs on %s/%s" % ((lpr,) + cell)


@pytest.mark.parametrize("lpr", LPRS)
def test_some_cell_walks_several_rows_per_lane_group(hg, lpr):
    for hop, (graph, name) in enumerate(SUPPLIERS[lpr]):
        inc, plan = _plan(graph, name)
        lens = np.diff(_walked(inc, plan, hop)[0])
        have = _group_features(lens, plan.schedule(hop)["panels"], lpr)
        print("LPR %d hop %d %s/%s: %s" % (lpr, hop, graph, name, sorted(have)))
        want = {"multi_row_panel", "adjacent_rows", "interior_empty"} | ({"group_ends_empty", "empty_run"} if hop == 0 else set())
        assert want <= have, "LPR %d hop %d: %s/%s lacks %s" % (lpr, hop, graph, name, sorted(want - have))


def test_default_plans_alone_reach_one_row_per_group_below_lpr_64(hg):
    """Why `wide` and `small` are in the matrix: default plans of these graphs have panels of 8 to 20 rows."""
    for graph in ir.GRAPHS:
        inc, plan = _plan(graph, "default")
        for hop in (0, 1):
            panels = plan.schedule(hop)["panels"]
            assert len(panels) == 0 or int(panels[:, 1].max()) <= 32, (graph, hop)


# ---- b: ties across the cuts -----------------------------------------------------------------------------------------------

def _tie_facts(graph, hop, name):
    """The cuts the `ties` input's equal best values lie across, for op = max, on the first TIE_COLUMNS columns."""
    inc, plan = _plan(graph, name)
    ptr, ind, pos = _walked(inc, plan, hop)
    src = torch.from_numpy(rr.draw(inc, hop, "ties")[:, :TIE_COLUMNS].copy())
    best, arg = (t.numpy() for t in rr.reduce_hop(inc, hop, src, "max"))
    vals = src.numpy()[ind]                       # [nnz, C] in the walked order
    where = np.empty(inc.nnz, np.int64)
    where[pos] = np.arange(inc.nnz)               # position in indices_t -> walked entry
    sched = plan.schedule(hop)
    tasks, fixups = sched["tasks"], sched["fixups"]
    facts = set()
    slot_has = {}                                 # slot -> [C] bool: the slot holds the row's best value
    first_end = {}                                # split row -> end of its first slot
    for row, beg, end, slot in tasks:
        hit = vals[beg:end] == best[row]          # [len, C]
        if slot >= 0:
            slot_has[slot] = hit.any(0)
            if beg == ptr[row]:
                first_end[row] = end
        for G in (2, 4, 8, 16, 32, 64):           # lane groups of a wave task at LPR = 64 / G
            groups = np.zeros((G, hit.shape[1]), bool)
            np.logical_or.at(groups, np.arange(end - beg) % G, hit)
            if (groups.sum(0) >= 2).any():
                facts.add("lane_groups_%d" % G)
    for row, first, count, pad in fixups:
        if pad > 0:
            continue
        level1 = [(f, n) for r, f, n, p in fixups if r == row and p > 0]
        slots = list(range(first, first + count)) if not level1 else [s for f, n in level1 for s in range(f, f + n)]
        if (np.sum([slot_has[s] for s in slots], 0) >= 2).any():
            facts.add("two_slots")
        if (where[arg[row]] >= first_end[row]).any():
            facts.add("winner_outside_first_slot")
        if level1:
            per_group = [np.any([slot_has[s] for s in range(f, f + n)], 0) for f, n in level1]
            if (np.sum(per_group, 0) >= 2).any():
                facts.add("two_level1_groups")
    return facts


@pytest.mark.parametrize("name", TIE_SETS)
@pytest.mark.parametrize("graph,hop", TIE_CELLS)
def test_ties_span_the_cuts(hg, graph, hop, name):
    facts = _tie_facts(graph, hop, name)
    print("%s hop %d %s: %s" % (graph, hop, name, sorted(facts)))
    want = {"two_slots", "winner_outside_first_slot"}
    if name == "small":
        want |= {"two_level1_groups"} | {"lane_groups_%d" % G for G in (2, 4, 8, 16, 32, 64)}
    assert want <= facts, "%s hop %d %s: the ties input lacks %s" % (graph, hop, name, sorted(want - facts))


# ---- c: lane shapes --------------------------------------------------------------------------------------------------------

def test_widths_instantiate_every_lane_shape():
    """The issue's sweep list (2, 6, 13, 21, 16, 256) leaves the 16-byte lanes without LPR 2, 8 and 32 (F / 4 = 2, 5 .. 8,
    17 .. 32): 8, 32 and 128 were added to SWEEP_WIDTHS for them."""
    assert set(rr.CORE_WIDTHS) == {1, 3, 4, 33, 64, 65, 260} and {2, 6, 13, 21, 16, 256} <= set(rr.SWEEP_WIDTHS)
    shapes = {F: rr.lane_shape(F) for F in rr.CORE_WIDTHS + rr.SWEEP_WIDTHS}
    for F, s in sorted(shapes.items()):
        print("F %3d: VEC %d LPR %2d tiles %d" % ((F,) + s))
    assert {s[:2] for s in shapes.values()} == {(v, l) for v in (1, 4) for l in LPRS}
    assert not {(v, l) for v in (1, 4) for l in LPRS} <= {rr.lane_shape(F)[:2] for F in rr.CORE_WIDTHS + (2, 6, 13, 21, 16, 256)}
    assert shapes[65] == (1, 64, 2) and shapes[33] == (1, 64, 1) and shapes[260] == (4, 64, 2)
    assert min(F for F in range(1, 300) if rr.lane_shape(F)[0] == 1 and rr.lane_shape(F)[2] == 2) == 65
    # the offset calls: 4-byte lanes at widths that are 16-byte lanes when aligned
    assert rr.lane_shape(rr.MISALIGNED_F, aligned=False) == (1, 8, 1)
    assert rr.lane_shape(rr.MISALIGNED_TILES_F, aligned=False) == (1, 64, 2)
    assert rr.MISALIGNED_TILES_CELL in rr.cells()
    assert rr.FMAX == max(shapes) and all((g, s) in rr.cells() for g, s in rr.SWEEP_CELLS)


# ---- d: the reduce_aggr pairs' inputs cannot round -------------------------------------------------------------------------

@pytest.mark.parametrize("graph", rr.PAIR_GRAPHS)
def test_pair_inputs_stay_exact_in_fp32(graph):
    """|X| <= 3, |dY| <= 2, degE * W in [SCALE_GRANULE, SCALE_PRODUCT_MAX], degV in [1/4, 1].  A max / min hop copies one term
    of what a sum hop would add, so (sum, sum) bounds every pair without a mean.  Every partial sum of Xe is an integer of
    magnitude at most 3 |e|; of Y a multiple of SCALE_GRANULE, at most 3 SCALE_PRODUCT_MAX sum_{e with v} |e|; of dXe a
    multiple of 1/4, at most 2 |e|; of dX a multiple of SCALE_GRANULE / 4, at most 2 SCALE_PRODUCT_MAX sum_{e with u} |e|.
    Each is exact in fp32 while magnitude / granule < 2^24."""
    inc = ir.schedule_graph(graph)
    for F in rr.PAIR_WIDTHS:
        X, dY = rr.pair_inputs(inc, F)
        assert np.array_equal(X, np.round(X)) and np.abs(X).max() <= 3 and np.abs(dY).max() <= 2 and np.array_equal(dY, np.round(dY))
    degE, degV, W = ir.power_of_two_scales(inc)
    assert float((degE * W).max()) <= ir.SCALE_PRODUCT_MAX and float((degE * W).min()) >= ir.SCALE_GRANULE
    assert float(degV.max()) <= 1.0 and float(degV.min()) >= 0.25
    top_e, top_v = ir.unweighted_mass_bound(inc)  # max |e|, max_v sum_{e with v} |e|
    bounds = {"Xe": 3 * top_e, "Y": 3 * ir.SCALE_PRODUCT_MAX * top_v / ir.SCALE_GRANULE, "dXe": 2 * top_e * 4,
              "dX": 2 * ir.SCALE_PRODUCT_MAX * top_v / (ir.SCALE_GRANULE / 4)}
    print("%s: magnitude / granule at most %s (2^24 = %d)" % (graph, bounds, 1 << 24))
    assert max(bounds.values()) < 2 ** 24, (graph, bounds)
