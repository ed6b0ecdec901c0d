"""What the C entries of include/hg_aggr.h refuse, in which order, with which status and which text of hg_last_error():
every bad call that can be made without a device -- a host-only plan of a handful of vertices, one host buffer that no
call reads or writes, and null pointers.

Each entry decides its refusals in an order of its own and the orders differ on purpose: a host-only plan is
HG_ERR_INVALID where the entry goes through the aggregation's common check and HG_ERR_UNSUPPORTED elsewhere; the plain
and dropout softmax entries look at the plan's kind before the group, the entry-logit ones after it;
hg_incidence_attention_heads_f32 reports itself as hg_incidence_attention_f32.  Where an order is documented, two faults
are made at once and the one that must win is asserted.

Not reachable here: whatever an entry decides only after it has refused a host-only plan -- the slope, p_drop and rng_dev
of the softmax entries, the arrays and widths of the entries behind the common check."""
import ctypes
import math

import numpy as np
import pytest

from hypergef_amd import synth

INV, WS, UNS = -1, -4, -5  # HG_ERR_INVALID, HG_ERR_WORKSPACE, HG_ERR_UNSUPPORTED
AUTO, PULL, PUSH, FUSED = 0, 1, 2, 3
NAN, INF = float("nan"), float("inf")


def small():
    """6 vertices x 5 hyperedges: hyperedge 2 is empty, hyperedge 3 lists vertex 4 twice, vertex 5 is in no hyperedge."""
    members = [[0, 1, 2], [1, 3], [], [4, 4, 0], [2, 3, 1, 0]]
    ptr = np.cumsum([0] + [len(m) for m in members]).astype(np.int32)
    return synth.Incidence(6, 5, ptr, np.concatenate([np.asarray(m, np.int32) for m in members]))


@pytest.fixture(scope="module")
def env(hg):
    from hypergef_amd import _lib
    from hypergef_amd.plan import Plan, make_opts
    inc = small()
    plan = Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True))
    buf = np.zeros(1024, np.float32)  # a non-null host address: never read, every call is refused before
    base = (buf.ctypes.data + 255) & ~255

    class Env:
        L = _lib.lib()
        h = plan._h
        null = ctypes.c_void_p()
        some = ctypes.c_void_p(base)      # 256-byte aligned
        off4 = ctypes.c_void_p(base + 4)  # no 8- or 16-byte lane
        off16 = ctypes.c_void_p(base + 16)  # lanes, but no 256-byte workspace

        def refused(self, status, want, fragment):
            msg = self.L.hg_last_error()
            assert status == want and fragment.encode() in msg, (status, msg)

    e = Env()
    e.keep = (plan, buf)
    yield e
    assert not buf.any()


def args(defaults, **kw):
    unknown = set(kw) - set(defaults)
    assert not unknown, unknown
    return [kw.get(k, v) for k, v in defaults.items()]


# ---- the segment softmax: plain, heads, dropout, entry, their backwards ---------------------------------------------

def softmax_entries(e):
    """name -> (function of keyword overrides, name the entry reports).  Every entry takes plan, group, heads (the two
    single-head entries: none), the CSR, the scores, slope, and outputs; dropout adds p_drop / rng, entry adds entry."""
    s, n = e.some, e.null
    L = e.L

    def make(fn, order, who):
        d = dict(plan=e.h, group=0, heads=1, ptr=s, ind=s, sv=s, se=s, entry=s, slope=0.2, p_drop=0.5, rng=s,
                 a=s, b=s, c=s, d=s, e=s, stream=n)
        return (lambda **kw: fn(*[args(d, **kw)[list(d).index(k)] for k in order]), who)

    fwd, bwd = ["a"], ["a", "b", "c", "d", "e"]
    head = ["plan", "group", "heads", "ptr", "ind", "sv", "se"]
    return {
        "plain1": make(L.hg_incidence_attention_f32, ["plan", "group", "ptr", "ind", "sv", "se", "slope"] + fwd + ["stream"],
                       "hg_incidence_attention_f32"),
        "plain": make(L.hg_incidence_attention_heads_f32, head + ["slope"] + fwd + ["stream"], "hg_incidence_attention_f32"),
        "plain1_bwd": make(L.hg_incidence_attention_bwd_f32,
                           ["plan", "group", "ptr", "ind", "sv", "se", "slope"] + bwd + ["stream"],
                           "hg_incidence_attention_bwd_f32"),
        "plain_bwd": make(L.hg_incidence_attention_heads_bwd_f32, head + ["slope"] + bwd + ["stream"],
                          "hg_incidence_attention_bwd_f32"),
        "drop": make(L.hg_incidence_attention_dropout_heads_f32, head + ["slope", "p_drop", "rng", "a", "b", "stream"],
                     "hg_incidence_attention_dropout_heads_f32"),
        "drop_bwd": make(L.hg_incidence_attention_dropout_heads_bwd_f32, head + ["slope", "p_drop", "rng"] + bwd + ["stream"],
                         "hg_incidence_attention_dropout_heads_bwd_f32"),
        "entry": make(L.hg_incidence_attention_entry_heads_f32, head + ["entry", "slope"] + fwd + ["stream"],
                      "hg_incidence_attention_entry_heads_f32"),
        "entry_bwd": make(L.hg_incidence_attention_entry_heads_bwd_f32, head + ["entry", "slope"] + bwd + ["stream"],
                          "hg_incidence_attention_entry_heads_bwd_f32"),
        "entry_drop": make(L.hg_incidence_attention_entry_dropout_heads_f32,
                           head + ["entry", "slope", "p_drop", "rng", "a", "b", "stream"],
                           "hg_incidence_attention_entry_dropout_heads_f32"),
        "entry_drop_bwd": make(L.hg_incidence_attention_entry_dropout_heads_bwd_f32,
                               head + ["entry", "slope", "p_drop", "rng"] + bwd + ["stream"],
                               "hg_incidence_attention_entry_dropout_heads_bwd_f32"),
    }


def test_softmax_entries(env):
    e = env
    for name, (call, who) in softmax_entries(e).items():
        has_heads = not name.startswith("plain1")
        # a null plan before everything else, every other argument bad too
        e.refused(call(plan=e.null, group=7, heads=0, ptr=e.null, slope=NAN, p_drop=2.0, rng=e.off4, entry=e.null),
                  INV, who + ": null plan")
        if has_heads:
            for heads in (0, -3):
                e.refused(call(heads=heads, group=7, ptr=e.null), INV, who + ": heads must be at least 1")
        if name.startswith("entry"):
            # the group and the logits are arguments: decided before the plan's kind
            for group in (2, -1):
                e.refused(call(group=group, entry=e.null), INV, who + ": group / side must be 0 (hyperedge) or 1 (vertex)")
            e.refused(call(entry=e.null, ptr=e.null), INV, who + ": null entry_score")
        else:
            # the plan's kind before the group
            e.refused(call(group=2), UNS, who + ": plan was built with HG_PLAN_HOST_ONLY and holds no device arrays")
        e.refused(call(ptr=e.null, slope=NAN, p_drop=-1.0, rng=e.null, a=e.null), UNS,
                  who + ": plan was built with HG_PLAN_HOST_ONLY and holds no device arrays")


# ---- attention statistics and the two attention gathers ---------------------------------------------------------------

def test_attention_stats(env):
    e, who = env, "hg_incidence_attention_stats_heads_f32"
    d = dict(plan=e.h, group=0, heads=1, ptr=e.some, ind=e.some, sv=e.some, se=e.some, slope=0.2, mx=e.some, inv=e.some,
             stream=e.null)
    call = lambda **kw: e.L.hg_incidence_attention_stats_heads_f32(*args(d, **kw))
    e.refused(call(plan=e.null, group=2, heads=0), INV, who + ": null plan")
    e.refused(call(group=2, heads=0), INV, who + ": group must be 0 (hyperedge) or 1 (vertex)")
    e.refused(call(heads=0, ptr=e.null), INV, who + ": heads must be at least 1")
    for k in ("ptr", "ind", "mx", "inv"):
        e.refused(call(**{k: e.null}, slope=NAN), INV, who + ": null array")
    for slope in (NAN, INF, -INF):
        e.refused(call(slope=slope), INV, who + ": non-finite slope")  # before the plan's kind
    e.refused(call(), UNS, who + ": plan was built with HG_PLAN_HOST_ONLY and holds no device arrays")


def attention_gathers(e):
    s, n = e.some, e.null
    d = dict(plan=e.h, hop=0, group=0, F=8, heads=2, ptr=s, ind=s, src=s, sv=s, se=s, slope=0.2, mx=s, inv=s, sA=n, sB=n,
             Xe=n, dst=s, ws=s, nbytes=1 << 20, stream=n)
    one = ["plan", "hop", "group", "F", "heads", "ptr", "ind", "src", "sv", "se", "slope", "mx", "inv", "sA", "sB", "dst", "ws",
           "nbytes", "stream"]
    two = ["plan", "F", "heads", "group", "ptr", "ind", "src", "sv", "se", "slope", "mx", "inv", "sA", "sB", "sB", "Xe", "dst",
           "ws", "nbytes", "stream"]
    pick = lambda order, kw: [args(d, **kw)[list(d).index(k)] for k in order]
    return {"hg_gather_rows_attention_heads_f32": lambda **kw: e.L.hg_gather_rows_attention_heads_f32(*pick(one, kw)),
            "hg_aggr_incidence_attention_heads_f32": lambda **kw: e.L.hg_aggr_incidence_attention_heads_f32(*pick(two, kw))}


def test_attention_gathers(env):
    e = env
    for who, call in attention_gathers(e).items():
        e.refused(call(plan=e.null, hop=2, group=2, heads=0, F=0), INV, who + ": null plan")
        if who.startswith("hg_gather"):
            for hop in (2, -1):
                e.refused(call(hop=hop, group=2), INV, who + ": hop must be 0 (to the hyperedges) or 1 (to the vertices)")
        for group in (2, -1):
            e.refused(call(group=group, heads=0), INV, who + ": group must be 0 (hyperedge) or 1 (vertex)")
        e.refused(call(heads=0, F=0), INV, who + ": heads must be at least 1")
        e.refused(call(F=9, src=e.null), INV, who + ": the feature width 9 must be a positive multiple of heads = 2")
        e.refused(call(F=0), INV, who + ": the feature width 0 must be a positive multiple of heads = 2")
        for k in ("ptr", "ind", "src", "dst", "mx", "inv"):
            e.refused(call(**{k: e.null}, slope=NAN), INV, who + ": null array")
        for slope in (NAN, INF, -INF):
            e.refused(call(slope=slope, nbytes=0), INV, who + ": non-finite slope")
        e.refused(call(nbytes=0), WS, who + ": workspace too small: need 768 bytes, got 0")
        e.refused(call(ws=e.null), WS, who + ": workspace too small: need 768 bytes")
        e.refused(call(ws=e.off16), INV, who + ": workspace must be 256-byte aligned")  # before the plan's kind
        e.refused(call(), UNS, who + ": plan was built with HG_PLAN_HOST_ONLY and holds no device schedule")


# ---- incidence-weighted aggregation and gather, fp32 and bf16 --------------------------------------------------------------

def test_incidence_aggregation(env):
    e, s, n = env, env.some, env.null
    d = dict(plan=e.h, F=8, heads=2, ptr=s, ind=s, X=s, v2e=s, e2v=s, degE=n, degV=n, W=n, Xe=n, Y=s, ws=s, nbytes=1 << 20,
             stream=n)
    single = [k for k in d if k != "heads"]
    plain = lambda **kw: e.L.hg_aggr_incidence_f32(*[args(d, **kw)[list(d).index(k)] for k in single])
    # the single-head entry goes through the aggregation's common check: INVALID, no name
    e.refused(plain(plan=n, F=0), INV, "null plan")
    e.refused(plain(F=0, ptr=n, ws=e.off16), INV, "plan was built with HG_PLAN_HOST_ONLY and holds no device schedule")
    for fn, who in ((e.L.hg_aggr_incidence_heads_f32, "hg_aggr_incidence_heads_f32"),
                    (e.L.hg_aggr_incidence_heads_bf16, "hg_aggr_incidence_heads_bf16")):
        call = lambda **kw: fn(*args(d, **kw))
        e.refused(call(plan=n, heads=0), INV, who + ": null plan")
        e.refused(call(heads=0, F=9), INV, who + ": heads must be at least 1")
        e.refused(call(F=9), INV, who + ": the feature width 9 is no multiple of heads = 2")
        e.refused(call(ptr=n, X=e.off4), UNS, who + ": plan was built with HG_PLAN_HOST_ONLY and holds no device arrays")


def test_incidence_gather(env):
    e, s, n = env, env.some, env.null
    d = dict(plan=e.h, hop=0, F=8, heads=2, ptr=s, ind=s, src=s, w=s, sA=n, sB=n, dst=s, ws=s, nbytes=1 << 20, io=1, stream=n)
    f32 = lambda **kw: e.L.hg_gather_rows_incidence_heads_f32(*[v for k, v in zip(d, args(d, **kw)) if k != "io"])
    b16 = lambda **kw: e.L.hg_gather_rows_incidence_heads_bf16(*args(d, **kw))
    for call, who in ((f32, "hg_gather_rows_incidence_heads_f32"), (b16, "hg_gather_rows_incidence_heads_bf16")):
        for hop in (2, -1):  # an argument: before the plan is looked at
            e.refused(call(plan=n, hop=hop, heads=0), INV, who + ": hop must be 0 (to the hyperedges) or 1 (to the vertices)")
        e.refused(call(plan=n, heads=0), INV, who + ": null plan")
        e.refused(call(heads=0, F=9), INV, who + ": heads must be at least 1")
        e.refused(call(F=9), INV, who + ": the feature width 9 is no multiple of heads = 2")
        e.refused(call(src=n, ws=e.off16), UNS, who + ": plan was built with HG_PLAN_HOST_ONLY and holds no device arrays")
    for io in (0, 4, -1):  # before the hop
        e.refused(b16(io=io, hop=2, plan=n), INV, "hg_gather_rows_incidence_heads_bf16: io must be HG_ROWS_SRC_BF16")


def test_plain_gather_and_fused(env):
    e, s, n = env, env.some, env.null
    g = dict(plan=e.h, hop=0, F=8, ptr=s, ind=s, src=s, sA=n, sB=n, dst=s, ws=s, nbytes=1 << 20, stream=n)
    gather = lambda **kw: e.L.hg_gather_rows_f32(*args(g, **kw))
    e.refused(gather(plan=n, hop=2), INV, "null plan")
    e.refused(gather(hop=2, F=0, src=n), INV, "plan was built with HG_PLAN_HOST_ONLY and holds no device schedule")
    d = dict(plan=e.h, F=8, ptr=s, ind=s, X=s, degE=n, degV=n, W=n, Y=s, ws=s, nbytes=1 << 20, variant=AUTO, stream=n)
    for fn, who in ((e.L.hg_aggr_fused_f32, "hg_aggr_fused_f32"), (e.L.hg_aggr_fused_bf16, "hg_aggr_fused_bf16")):
        call = lambda **kw: fn(*args(d, **kw))
        for variant in (4, -1, 99):  # before the plan
            e.refused(call(variant=variant, plan=n), UNS, who + ": unknown variant")
        for variant in (AUTO, PULL, FUSED):
            e.refused(call(variant=variant, plan=n, F=0), INV, "null plan")
            e.refused(call(variant=variant, F=0, X=n, ws=e.off16), INV,
                      "plan was built with HG_PLAN_HOST_ONLY and holds no device schedule")
    e.refused(e.L.hg_aggr_fused_f32(*args(d, variant=PUSH, plan=n)), INV, "null plan")
    e.refused(e.L.hg_aggr_fused_f32(*args(d, variant=PUSH, F=0)), INV, "hg_aggr_push_groups_f32: bad argument")
    e.refused(e.L.hg_aggr_fused_f32(*args(d, variant=PUSH, X=n)), INV, "hg_aggr_push_groups_f32: bad argument")
    e.refused(e.L.hg_aggr_fused_bf16(*args(d, variant=PUSH, plan=n)), UNS, "hg_aggr_fused_bf16: HG_VARIANT_PUSH_ATOMIC is fp32 only")


# ---- max / min and their select ------------------------------------------------------------------------------------------

def test_reduce_and_select(env):
    e, s, n = env, env.some, env.null
    r = dict(plan=e.h, hop=0, F=8, op=1, ptr=s, ind=s, src=s, sA=n, sB=n, dst=s, arg=s, ws=s, nbytes=1 << 20, stream=n)
    reduce = lambda **kw: e.L.hg_gather_rows_reduce_f32(*args(r, **kw))
    select = lambda **kw: e.L.hg_gather_rows_select_f32(
        *[v for k, v in zip(r, args(r, **kw)) if k not in ("op", "sA", "sB")])  # gs = src, arg = dst, dsrc = arg
    for call, who in ((reduce, "hg_gather_rows_reduce_f32"), (select, "hg_gather_rows_select_f32")):
        e.refused(call(plan=n, hop=2, F=0), INV, who + ": null plan")
        for hop in (2, -1):
            e.refused(call(hop=hop, F=0, src=n), INV, who + ": hop must be 0 (to the hyperedges) or 1 (to the vertices)")
        for hop in (0, 1):  # the plan's kind before the width, the arrays and the workspace
            e.refused(call(hop=hop, F=0, src=n, ws=e.off16, nbytes=0), UNS,
                      who + ": plan was built with HG_PLAN_HOST_ONLY and holds no device arrays")
    for op in (0, 3, -1):
        e.refused(reduce(op=op, hop=2), INV, "hg_gather_rows_reduce_f32: hop must be")  # the hop before the op
        e.refused(reduce(op=op), INV, "hg_gather_rows_reduce_f32: op must be HG_REDUCE_MAX or HG_REDUCE_MIN")  # the op before the plan's kind


# ---- products per incidence ------------------------------------------------------------------------------------------------

def test_incidence_dot(env):
    e, s, n = env, env.some, env.null
    d = dict(plan=e.h, F=8, heads=2, ptr=s, ind=s, A=s, B=s, out=s, io=1, stream=n)
    plain = lambda **kw: e.L.hg_incidence_dot_f32(*[v for k, v in zip(d, args(d, **kw)) if k not in ("heads", "io")])
    heads = lambda **kw: e.L.hg_incidence_dot_heads_f32(*[v for k, v in zip(d, args(d, **kw)) if k != "io"])
    b16 = lambda **kw: e.L.hg_incidence_dot_heads_bf16(*args(d, **kw))
    e.refused(plain(plan=n, F=0), INV, "null plan")
    e.refused(plain(F=0, A=n), INV, "plan was built with HG_PLAN_HOST_ONLY and holds no device schedule")
    for call, who in ((heads, "hg_incidence_dot_heads_f32"), (b16, "hg_incidence_dot_heads_bf16")):
        e.refused(call(plan=n, heads=0), INV, who + ": null plan")
        e.refused(call(heads=0, F=9), INV, who + ": heads must be at least 1")
        e.refused(call(F=9), INV, who + ": the feature width 9 is no multiple of heads = 2")
        e.refused(call(A=n), UNS, who + ": plan was built with HG_PLAN_HOST_ONLY and holds no device arrays")
    e.refused(heads(heads=1), UNS, "hg_incidence_dot_heads_f32: plan was built with HG_PLAN_HOST_ONLY")  # not the single-head entry's answer
    for io in (0, 4, -1):  # before the plan
        e.refused(b16(io=io, plan=n), INV, "hg_incidence_dot_heads_bf16: io must be HG_DOT_A_BF16")
    h = dict(plan=e.h, F=8, heads=2, ptr=s, ind=s, A=s, wa=n, B=s, wb=n, out=s, stream=n)
    edge = lambda **kw: e.L.hg_hyperedge_dot_heads_f32(*args(h, **kw))
    who = "hg_hyperedge_dot_heads_f32"
    e.refused(edge(plan=n, F=0), INV, who + ": null plan")
    e.refused(edge(F=0, heads=0), INV, who + ": the feature width must be at least 1")
    e.refused(edge(heads=0), INV, who + ": heads must be at least 1")
    e.refused(edge(F=9), INV, who + ": the feature width 9 is no multiple of heads = 2")
    e.refused(edge(A=n, ptr=n), UNS, who + ": plan was built with HG_PLAN_HOST_ONLY and holds no device arrays")


# ---- the linear layer folded into the aggregation ---------------------------------------------------------------------------

WIDTHS = "need F_in in {32, 64, 128}, F_out a positive multiple of 16"
BAD_WIDTHS = ((48, 16), (0, 16), (256, 16), (32, 0), (32, 24), (32, -16))


def test_linear_f32(env):
    e, s, n = env, env.some, env.null
    d = dict(plan=e.h, F_in=32, F_out=16, ptr=s, ind=s, X=s, degE=n, degV=n, W=n, wfrag=s, R=n, ca=1.0, cb=0.0, relu=0, T_out=n,
             Y=s, ws=s, nbytes=1 << 20, variant=AUTO, stream=n)
    res = lambda **kw: e.L.hg_aggr_linear_res_f32(*args(d, **kw))
    dev = lambda **kw: e.L.hg_aggr_linear_res_dev_f32(*args(d, **dict(dict(cb=s), **kw)))
    lin = lambda **kw: e.L.hg_aggr_linear_f32(
        *[v for k, v in zip(d, args(d, **kw)) if k not in ("R", "ca", "cb", "relu", "T_out")])
    who = "hg_aggr_linear_f32"  # all three report this name
    e.refused(dev(cb=n, plan=n), INV, "hg_aggr_linear_res_dev_f32: cb_dev is null")
    for call in (res, dev, lin):
        for k in ("plan", "wfrag", "Y"):
            e.refused(call(**{k: n}, F_in=48), INV, who + ": null argument")
        for F_in, F_out in BAD_WIDTHS:
            e.refused(call(F_in=F_in, F_out=F_out, variant=PUSH), UNS, who + ": " + WIDTHS)
        e.refused(call(variant=PUSH, ws=n), UNS, who + ": push-atomic variant not supported")
        e.refused(call(ws=n, Y=e.off4), WS, who + ": workspace smaller than hg_aggr_linear_workspace_bytes")
        e.refused(call(nbytes=16, wfrag=e.off4), WS, who + ": workspace smaller than hg_aggr_linear_workspace_bytes")
        e.refused(call(Y=e.off4), INV, who + ": wfrag, R, T_out and Y must be 16-byte aligned")  # before the plan's kind
        e.refused(call(wfrag=e.off4), INV, who + ": wfrag, R, T_out and Y must be 16-byte aligned")
        e.refused(call(variant=9), UNS, "hg_aggr_fused_f32: unknown variant")
        e.refused(call(), INV, "plan was built with HG_PLAN_HOST_ONLY and holds no device schedule")
    for call in (res, dev):
        for k in ("R", "T_out"):
            e.refused(call(**{k: e.off4}), INV, who + ": wfrag, R, T_out and Y must be 16-byte aligned")
    rows = dict(nrows=4, F_in=32, F_out=16, T=s, wfrag=s, Y=s, stream=n)
    call = lambda **kw: e.L.hg_linear_rows_f32(*args(rows, **kw))
    e.refused(call(nrows=-1, F_in=48), INV, "hg_linear_rows_f32: bad argument")
    for k in ("T", "wfrag", "Y"):
        e.refused(call(**{k: n}, F_in=48), INV, "hg_linear_rows_f32: bad argument")
    for F_in, F_out in BAD_WIDTHS:
        e.refused(call(F_in=F_in, F_out=F_out, T=e.off4), UNS, "hg_linear_rows_f32: " + WIDTHS)
    for k in ("T", "wfrag", "Y"):
        e.refused(call(**{k: e.off4}), INV, "hg_linear_rows_f32: arrays must be 16-byte aligned")
    pack = lambda F_out, F_in, w, frag: e.L.hg_linear_pack_f32(F_out, F_in, w, frag, n)
    e.refused(pack(16, 32, n, s), INV, "hg_linear_pack_f32: " + WIDTHS)  # a null array: INVALID, under the widths' text
    e.refused(pack(16, 32, s, n), INV, "hg_linear_pack_f32: " + WIDTHS)
    for F_in, F_out in BAD_WIDTHS:
        e.refused(pack(F_out, F_in, s, s), UNS, "hg_linear_pack_f32: " + WIDTHS)


def test_linear_bf16(env):
    e, s, n = env, env.some, env.null
    who = "hg_aggr_linear_res_bf16"
    d = dict(plan=e.h, F_in=32, F_out=16, ptr=s, ind=s, X=s, degE=n, degV=n, W=n, wfrag=s, R=n, ca=1.0, cb=0.0, cb_dev=n, flags=0,
             T_out=n, Y=s, ws=s, nbytes=1 << 20, variant=AUTO, stream=n)
    call = lambda **kw: e.L.hg_aggr_linear_res_bf16(*args(d, **kw))
    # the documented order: arguments, flags, variant, widths, alignment, the plan's kind, the workspace
    for k in ("plan", "ptr", "ind", "X", "wfrag", "Y"):
        e.refused(call(**{k: n}, flags=2), INV, who + ": null argument")
    for flags in (2, 4, 3, -1):
        e.refused(call(flags=flags, variant=PUSH), INV, who + ": flags takes HG_LIN_RELU only")
    for variant in (PUSH, 4, -1):
        e.refused(call(variant=variant, F_in=48), UNS, who + ": variant must be auto, pull or fused")
    for F_in, F_out in BAD_WIDTHS:
        e.refused(call(F_in=F_in, F_out=F_out, X=e.off4), UNS, who + ": " + WIDTHS)
    for k in ("X", "Y", "R", "T_out", "wfrag"):
        e.refused(call(**{k: e.off4}), UNS, who + ": X, Y, R and T_out must be 8-byte aligned, wfrag 16-byte aligned")
    e.refused(call(ws=n), UNS, who + ": plan was built with HG_PLAN_HOST_ONLY and holds no device schedule")
    e.refused(call(flags=1), UNS, who + ": plan was built with HG_PLAN_HOST_ONLY and holds no device schedule")

    path = lambda plan=e.h, F_in=32, F_out=16, variant=AUTO: e.L.hg_aggr_linear_bf16_path(plan, F_in, F_out, variant)
    e.refused(path(plan=n, F_in=48), INV, "hg_aggr_linear_bf16_path: null plan")
    for variant in (PUSH, 4, -1):
        e.refused(path(variant=variant), UNS, "hg_aggr_linear_bf16_path: need variant auto, pull or fused")
    for F_in, F_out in BAD_WIDTHS:
        e.refused(path(F_in=F_in, F_out=F_out), UNS, "hg_aggr_linear_bf16_path: need variant auto, pull or fused")
        assert e.L.hg_linear_pack_bf16_bytes(F_out, F_in) == 0
    assert e.L.hg_linear_pack_bf16_bytes(16, 32) == 2 * 16 * 32
    assert path(variant=PULL) == 2  # every row through the rows kernel: decided on the host

    rows = dict(nrows=4, F_in=32, F_out=16, T=s, wfrag=s, Y=s, stream=n)
    call = lambda **kw: e.L.hg_linear_rows_bf16(*args(rows, **kw))
    e.refused(call(nrows=-1, F_in=48), INV, "hg_linear_rows_bf16: bad argument")
    for k in ("T", "wfrag", "Y"):
        e.refused(call(**{k: n}, F_in=48), INV, "hg_linear_rows_bf16: bad argument")
    for F_in, F_out in BAD_WIDTHS:
        e.refused(call(F_in=F_in, F_out=F_out, T=e.off4), UNS, "hg_linear_rows_bf16: " + WIDTHS)
    for k in ("T", "wfrag", "Y"):
        e.refused(call(**{k: e.off4}), UNS, "hg_linear_rows_bf16: T and Y must be 8-byte aligned, wfrag 16-byte aligned")
    pack = lambda F_out, F_in, w, frag: e.L.hg_linear_pack_bf16(F_out, F_in, w, frag, n)
    e.refused(pack(16, 48, n, s), INV, "hg_linear_pack_bf16: null argument")
    e.refused(pack(16, 48, s, n), INV, "hg_linear_pack_bf16: null argument")
    for F_in, F_out in BAD_WIDTHS:
        e.refused(pack(F_out, F_in, s, s), UNS, "hg_linear_pack_bf16: " + WIDTHS + ", wfrag 16-byte aligned")
    e.refused(pack(16, 32, s, e.off4), UNS, "hg_linear_pack_bf16: " + WIDTHS + ", wfrag 16-byte aligned")


def test_nothing_was_written(env):
    """Runs last: the three addresses are what their names say, and no refused call wrote through one of them."""
    base = env.some.value
    assert base % 256 == 0 and env.off4.value == base + 4 and env.off16.value == base + 16
    assert math.isnan(NAN) and math.isinf(INF)
    assert not env.keep[1].any()
