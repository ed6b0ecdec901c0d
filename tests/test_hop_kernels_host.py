"""CPU-only: Plan.pin / Plan.unpin (hg_plan_set_choice) and Plan.has_latency_schedule on host-only plans -- what
test_hop_kernels_gpu.py relies on to name the kernel it checks.

1. Every refusal of the header leaves the plan's AUTO answer as it was and a message in hg_last_error: F < 1, a mask outside
   0 .. 8, a mask naming kernel 2 on a plan without a latency schedule, any variant but fused / pull / auto.
2. pin(F, "pull", m) makes auto_variant(F) "pull", pin(F, "fused", 0) makes it "fused", unpin(F) restores the static answer;
   a pin on F = 32 does not move F = 64; what Plan.tune returns is accepted as keywords.
3. The plan reports a latency schedule exactly when nnz <= 2^18 and the resolved short_max is above kLatShortMax.
4. hg_plan_workspace_bytes under every pin is at least the unpinned value (printed).
5. The integer inputs of the GPU file's exact check cannot round: the unweighted mass, times the largest scale product, in
   units of the smallest, stays below 2^24 on every graph.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _incidence_ref as ir  # noqa: E402

WIDTHS = (32, 64)
_PLANS = {}


def _plan(hg, graph="ragged", name="default", **kw):
    """A host-only plan of a graph under an option set, with the default row_stream: fresh for every caller that pins."""
    from hypergef_amd.plan import Plan, make_opts
    if graph not in _PLANS:
        _PLANS[graph] = ir.schedule_graph(graph)
    inc = _PLANS[graph]
    opts = dict(ir.option_sets()[name], **kw)
    return Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True, **opts))


def _raw_pin(plan, F, variant, mask):
    """hg_plan_set_choice with raw codes: (status, message)."""
    from hypergef_amd import _lib
    st = _lib.lib().hg_plan_set_choice(plan._h, F, variant, mask)
    return st, (_lib.lib().hg_last_error() or b"").decode()


def test_the_two_plans_are_the_ones_the_issue_names(hg):
    default, small = _plan(hg), _plan(hg, name="small")
    assert default.has_latency_schedule() and ir.hop_masks(True) == tuple(range(9))
    assert small.info["short_max"] == 6 and not small.has_latency_schedule()
    assert ir.hop_masks(False) == (0, 1, 3, 4)


@pytest.mark.parametrize("name", ["default", "small"])
def test_refusals_leave_the_plan_as_it_was(hg, name):
    from hypergef_amd import _lib
    for state in ("static", "pinned"):
        plan = _plan(hg, name=name)
        if state == "pinned":
            for F in WIDTHS:
                plan.pin(F, "pull" if plan.auto_variant(F) == "fused" else "fused", 1)  # not the static answer
        before = {F: plan.auto_variant(F) for F in WIDTHS}
        sizes = {F: plan.workspace_bytes(F) for F in WIDTHS}
        bad = [(0, _lib.HG_VARIANT_PULL, 0), (-1, _lib.HG_VARIANT_PULL, 0), (-32, _lib.HG_VARIANT_FUSED, 0),
               (0, _lib.HG_VARIANT_AUTO, 0)]
        for F in WIDTHS:
            bad += [(F, v, m) for v in (_lib.HG_VARIANT_PULL, _lib.HG_VARIANT_FUSED) for m in (-1, 9, 10, 27, -9, 1 << 30)]
            bad += [(F, v, m) for v in (_lib.HG_VARIANT_PUSH_ATOMIC, 4, -1, 7, 1 << 20) for m in (0, 4)]
            if not plan.has_latency_schedule():
                bad += [(F, v, m) for v in (_lib.HG_VARIANT_PULL, _lib.HG_VARIANT_FUSED) for m in (2, 5, 6, 7, 8)]
        for F, v, m in bad:
            st, msg = _raw_pin(plan, F, v, m)
            assert st == _lib.HG_ERR_INVALID and "hg_plan_set_choice" in msg, (name, state, F, v, m, st, msg)
            plan.__dict__.pop("_ws_bytes", None)
            assert {G: plan.auto_variant(G) for G in WIDTHS} == before, (name, state, F, v, m)
            assert {G: plan.workspace_bytes(G) for G in WIDTHS} == sizes, (name, state, F, v, m)
        # the Python layer: the same refusals as exceptions
        with pytest.raises(_lib.HgError) as err:
            plan.pin(32, "push_atomic")
        assert err.value.status == _lib.HG_ERR_INVALID
        with pytest.raises(_lib.HgError):
            plan.pin(0, "pull")
        with pytest.raises(_lib.HgError):
            plan.pin(32, "pull", 9)
        with pytest.raises(ValueError):
            plan.pin(32, "latency")
        assert {G: plan.auto_variant(G) for G in WIDTHS} == before
    assert _lib.lib().hg_plan_set_choice(None, 32, _lib.HG_VARIANT_PULL, 0) == _lib.HG_ERR_INVALID
    assert _lib.lib().hg_plan_has_latency_schedule(None) == _lib.HG_ERR_INVALID


@pytest.mark.parametrize("name", ["default", "small"])
def test_pin_and_unpin(hg, name):
    plan = _plan(hg, name=name)
    static = {F: plan.auto_variant(F) for F in WIDTHS}
    masks = ir.hop_masks(plan.has_latency_schedule())
    assert len(masks) == (9 if name == "default" else 4)
    for m in masks:
        plan.pin(32, "pull", m)
        assert plan.auto_variant(32) == "pull" and plan.auto_variant(64) == static[64], m
        plan.pin(32, "fused", 0)
        assert plan.auto_variant(32) == "fused" and plan.auto_variant(64) == static[64], m
        plan.pin(32, "fused", m)  # a fused pin keeps hop kernels for forced pull calls
        assert plan.auto_variant(32) == "fused", m
        plan.unpin(32)
        assert plan.auto_variant(32) == static[32] and plan.auto_variant(64) == static[64], m
    plan.pin(64, "fused" if static[64] == "pull" else "pull", masks[-1])
    assert plan.auto_variant(64) != static[64] and plan.auto_variant(32) == static[32]
    plan.unpin(64)
    plan.unpin(64)  # nothing to remove: fine
    plan.unpin(7)   # a width never seen
    assert {F: plan.auto_variant(F) for F in WIDTHS} == static
    # a plan that never resolved AUTO for the width takes a pin too, and what Plan.tune returns goes in as keywords
    fresh = _plan(hg, name=name)
    tuned = {"variant": "pull", "pull_hop_kernels": masks[-1], "us": {"pull": 1.0}}
    fresh.pin(32, **{k: tuned[k] for k in ("variant", "pull_hop_kernels")})
    assert fresh.auto_variant(32) == "pull"
    fresh.unpin(32)
    assert fresh.auto_variant(32) == static[32]


def test_latency_schedule_exists_as_the_code_states(hg):
    from hypergef_amd import synth
    from hypergef_amd.plan import Plan, make_opts
    cut = ir.lat_short_max()
    seen = set()
    for graph in ("toy", "ragged"):
        for name in ir.OPTION_SETS:
            plan = _plan(hg, graph, name)
            want = ir.expect_latency_schedule(plan.nnz, plan.info["short_max"])
            assert plan.has_latency_schedule() == want, (graph, name, plan.info["short_max"])
            if name in ir.HOP_SETS_WITH_LAT:
                assert want == ir.HOP_SETS_WITH_LAT[name], (graph, name)
            seen.add(want)
        for short_max, want in ((cut - 1, False), (cut, False), (cut + 1, True)):  # the cut itself
            assert _plan(hg, graph, "default", short_max=short_max).has_latency_schedule() == want, (graph, short_max)
    assert seen == {True, False}
    for graph in ir.GRAPHS:  # the GPU file's graphs: all launch-bound
        assert _PLANS.setdefault(graph, ir.schedule_graph(graph)).nnz <= ir.LAT_NNZ_MAX, graph
    big = synth.random_incidence(60000, 50000, 6.0, seed=2)  # above 2^18 incidences: none, whatever short_max
    plan = Plan.from_host(big.N, big.M, big.csrptr, big.colind, opts=make_opts(host_only=True))
    assert big.nnz > ir.LAT_NNZ_MAX and plan.info["short_max"] > cut and not plan.has_latency_schedule()
    from hypergef_amd import _lib
    assert _raw_pin(plan, 32, _lib.HG_VARIANT_PULL, 8)[0] == _lib.HG_ERR_INVALID
    plan.pin(32, "pull", 4)


@pytest.mark.parametrize("name", ["default", "small"])
def test_workspace_under_every_pin(hg, name):
    plan = _plan(hg, name=name)
    for F in (1, 3, 32, 33, 64, 260):
        base = plan.workspace_bytes(F)
        assert base > 0 and base % 256 == 0
        got = {}
        for variant in ("pull", "fused"):
            for m in ir.hop_masks(plan.has_latency_schedule()):
                plan.pin(F, variant, m)
                got[variant, m] = plan.workspace_bytes(F)
                assert got[variant, m] >= base and got[variant, m] % 256 == 0, (name, F, variant, m, got[variant, m], base)
                assert plan.incidence_workspace_bytes(F) <= got[variant, m]
        plan.unpin(F)
        print("%s F %d: %d bytes unpinned (%s); pinned pull %s, pinned fused %s" % (
            name, F, base, plan.auto_variant(F), sorted({v for (k, _), v in got.items() if k == "pull"}),
            sorted({v for (k, _), v in got.items() if k == "fused"})))
        assert plan.workspace_bytes(F) >= base  # a fused schedule built under a pin stays and may keep the size up


@pytest.mark.parametrize("graph", ir.GRAPHS)
def test_integer_sums_with_power_of_two_scales_stay_exact(graph):
    """X in {-1, 0, 1}, unit incidence weights, degE / degV in {0.25, 0.5, 1}, W in {0.5, 1, 2}: every partial sum of either
    hop, in any order, is a multiple of SCALE_GRANULE (times degV's 2^-2 after the last product) of magnitude at most
    SCALE_PRODUCT_MAX * mass, so it is exact in fp32 while mass * SCALE_PRODUCT_MAX / SCALE_GRANULE < 2^24."""
    import numpy as np
    inc = ir.schedule_graph(graph)
    degE, degV, W = ir.power_of_two_scales(inc)
    assert set(np.unique(degE)) | set(np.unique(degV)) <= {0.25, 0.5, 1.0} and set(np.unique(W)) <= {0.5, 1.0, 2.0}
    assert float((degE * W).max()) <= ir.SCALE_PRODUCT_MAX and float((degE * W).min()) >= ir.SCALE_GRANULE
    top_xe, top_y = ir.unweighted_mass_bound(inc)
    print("%s: unweighted mass of hop 1 <= %g, of Y <= %g; times %g: %g (2^24 = %d)" % (
        graph, top_xe, top_y, ir.SCALE_PRODUCT_MAX / ir.SCALE_GRANULE, top_y * ir.SCALE_PRODUCT_MAX / ir.SCALE_GRANULE, 1 << 24))
    assert max(top_xe, top_y) * ir.SCALE_PRODUCT_MAX < 2 ** 24                      # the issue's condition
    assert max(top_xe, top_y) * ir.SCALE_PRODUCT_MAX / ir.SCALE_GRANULE < 2 ** 24  # and with the scales' low bits
