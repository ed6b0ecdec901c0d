"""CPU-only: what the schedule matrix of test_incidence_schedules.py (graphs x plan-option sets) reaches, read from
host-only plans, and that the integer inputs of its exact check cannot round.

1. Over the matrix, every feature of the row schedule the weighted kernels index by occurs on both hops, and SUPPLIERS
   names a (graph, option set) that has it: a panel filled to panel_nnz, a panel of panel_rows rows, a panel that begins /
   ends with an empty row, a row of exactly short_max entries inside a panel and one of short_max + 1 as a wave task, a
   task that writes a partial slot, a first-level fixup, and (remap on) a panel count that is no multiple of 8.
2. The `wide` set is the largest panel the weighted entry's LDS formula lets through, the next panel_rows up is the first
   it refuses, and hg_plan_create itself accepts both.
3. For the inputs of the exact check (X in {-1, 0, 1}, weights in {-2 .. 2}) the sums of absolute values behind every element
   of hop 1's table and of Y stay below 2^24 on every graph: every partial sum in any order is exact in fp32.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _grad_ref as gr  # noqa: E402
import _incidence_ref as ir  # noqa: E402

FEATURES = ("panel_nnz_full", "panel_rows_full", "panel_begins_empty", "panel_ends_empty", "cut_row_in_panel",
            "cut_plus_one_is_task", "partial_slot", "level1_fixup", "remap_remainder")

# feature -> ((graph, option set) for hop 0 (rows = hyperedges), the same for hop 1 (rows = vertices))
SUPPLIERS = {
    "panel_nnz_full": (("ragged", "small"), ("ragged", "small")),
    "panel_rows_full": (("boundaries_T", "small"), ("boundaries", "small")),
    "panel_begins_empty": (("ragged", "odd"), ("ragged", "odd")),
    "panel_ends_empty": (("ragged", "odd"), ("ragged", "odd")),
    "cut_row_in_panel": (("boundaries", "lat"), ("boundaries_T", "lat")),
    "cut_plus_one_is_task": (("boundaries", "lat"), ("boundaries_T", "lat")),
    "partial_slot": (("boundaries", "default"), ("boundaries_T", "default")),
    "level1_fixup": (("boundaries", "small"), ("boundaries_T", "small")),
    "remap_remainder": (("ragged", "small"), ("ragged", "small")),
}

_PLANS = {}


def _plan(hg, graph, name):
    """(incidence, host-only plan) of a cell of the matrix, built once."""
    from hypergef_amd.plan import Plan, make_opts
    if (graph, name) not in _PLANS:
        inc = ir.schedule_graph(graph)
        opts = make_opts(host_only=True, row_stream=False, **ir.option_sets()[name])
        _PLANS[graph, name] = (inc, Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=opts))
    return _PLANS[graph, name]


def _features(inc, plan, name, hop):
    """The FEATURES hop's schedule of this plan has."""
    info, sched = plan.info, plan.schedule(hop)
    ptr = inc.csrptr if hop == 0 else plan.vertex_csr()[0]
    lens = np.diff(ptr.astype(np.int64))
    panels, tasks, fixups = sched["panels"], sched["tasks"], sched["fixups"]
    in_panel = np.zeros(lens.shape[0], bool)
    for row0, n, nnz0, cnt in panels:
        assert ptr[row0] == nnz0 and ptr[row0 + n] - nnz0 == cnt
        in_panel[row0:row0 + n] = True
    is_task = np.zeros(lens.shape[0], bool)
    is_task[tasks[:, 0]] = True
    assert not (in_panel & is_task).any() and (in_panel | is_task).all()
    have = set()
    if len(panels):
        first, last = lens[panels[:, 0]], lens[panels[:, 0] + panels[:, 1] - 1]
        if (panels[:, 3] == info["panel_nnz"]).any():
            have.add("panel_nnz_full")
        if (panels[:, 1] == info["panel_rows"]).any():
            have.add("panel_rows_full")
        if (first == 0).any():
            have.add("panel_begins_empty")
        if (last == 0).any():
            have.add("panel_ends_empty")
        if len(panels) % 8 and ir.option_sets()[name].get("xcd_remap", True):
            have.add("remap_remainder")
    if (in_panel & (lens == info["short_max"])).any():
        have.add("cut_row_in_panel")
    if (is_task & (lens == info["short_max"] + 1)).any():
        have.add("cut_plus_one_is_task")
    if len(tasks) and (tasks[:, 3] >= 0).any():
        have.add("partial_slot")
    if len(fixups) and (fixups[:, 3] > 0).any():
        have.add("level1_fixup")
    return have


def test_option_sets_are_the_ones_the_plan_runs(hg):
    sets = ir.option_sets()
    assert tuple(sets) == ir.OPTION_SETS
    inc, plan = _plan(hg, "toy", "lat")
    assert plan.info["short_max"] == ir.lat_short_max() < _plan(hg, "toy", "default")[1].info["short_max"]
    for name, kw in sets.items():
        info = _plan(hg, "toy", name)[1].info
        for key in ("short_max", "split_len", "panel_rows", "panel_nnz"):
            assert key not in kw or info[key] == kw[key], (name, key, info)


def test_wide_is_the_largest_panel_the_weighted_entry_accepts(hg):
    from hypergef_amd import _lib
    from hypergef_amd.plan import Plan, make_opts
    rows = ir.wide_panel_rows()
    assert ir.option_sets()["wide"] == dict(panel_rows=rows, panel_nnz=ir.PANEL_NNZ_MAX)
    assert ir.weighted_lds_bytes(rows, ir.PANEL_NNZ_MAX) <= ir.LDS_BYTES < ir.weighted_lds_bytes(rows + 1, ir.PANEL_NNZ_MAX)
    inc = ir.schedule_graph("toy")
    for r in (rows, rows + 1):  # hg_plan_create limits neither: its own bound counts panel_nnz once
        info = Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind,
                              opts=make_opts(host_only=True, panel_rows=r, panel_nnz=ir.PANEL_NNZ_MAX)).info
        assert (info["panel_rows"], info["panel_nnz"]) == (r, ir.PANEL_NNZ_MAX)
    with pytest.raises(_lib.HgError):  # and panel_nnz cannot grow instead
        Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True, panel_nnz=ir.PANEL_NNZ_MAX + 1))


def test_matrix_reaches_every_schedule_feature_on_both_hops(hg):
    seen = {(f, hop): [] for f in FEATURES for hop in (0, 1)}
    for graph in ir.GRAPHS:
        for name in ir.OPTION_SETS:
            inc, plan = _plan(hg, graph, name)
            for hop in (0, 1):
                for f in _features(inc, plan, name, hop):
                    seen[f, hop].append((graph, name))
    for (f, hop), cells in sorted(seen.items()):
        print("%-22s hop %d: %s" % (f, hop, ", ".join("%s/%s" % c for c in cells)))
    assert set(SUPPLIERS) == set(FEATURES)
    for f in FEATURES:
        for hop in (0, 1):
            assert SUPPLIERS[f][hop] in seen[f, hop], "%s on hop %d: %s does not supply it (%s do)" % (
                f, hop, SUPPLIERS[f][hop], seen[f, hop])


def test_every_cut_is_crossed_on_both_sides(hg):
    """boundaries holds a hyperedge, boundaries_T a vertex, of every length 0 .. 70: each set's short_max and split_len is met
    at -1 / 0 / +1 where it is below 70 (the default split_len of 512 is not: its rows of 1023 .. 1025 and 5000 are cut)."""
    for graph, hop in (("boundaries", 0), ("boundaries_T", 1)):
        for name in ir.OPTION_SETS:
            inc, plan = _plan(hg, graph, name)
            lens = set(np.diff(inc.csrptr if hop == 0 else plan.vertex_csr()[0]).tolist())
            for key in ("short_max", "split_len"):
                t = plan.info[key]
                if t <= 69:
                    assert {t - 1, t, t + 1} <= lens, (graph, name, key)
            assert max(lens) > 2 * plan.info["split_len"], (graph, name)


@pytest.mark.parametrize("graph", ir.GRAPHS)
def test_integer_inputs_stay_exact_in_fp32(graph):
    inc = ir.schedule_graph(graph)
    g = gr.Graph(inc)
    for heads, F in [(1, max(ir.WIDTHS))] + [(h, h * c) for h, c in ir.EXACT_PAIRS]:
        X, v2e, e2v = ir.integer_inputs(inc, F, heads)
        assert set(np.unique(X)) <= {-1.0, 0.0, 1.0} and set(np.unique(v2e)) | set(np.unique(e2v)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        top_xe, top_y = ir.exact_mass(g, X, v2e, e2v, heads)
        print("%s heads %d F %d: mass of hop 1 <= %g, of Y <= %g (2^24 = %d)" % (graph, heads, F, top_xe, top_y, 1 << 24))
        assert top_xe < 2 ** 24 and top_y < 2 ** 24, (graph, heads, F, top_xe, top_y)
