"""Max / min / mean reductions without a device: what incidence_gather(reduce=...) and reduce_aggr refuse before a device is
touched, the exported names, the C entries' refusal codes and their order on a host-only plan, and the exact reference of
tests/_reduce_ref.py against the definition written as loops."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _reduce_ref as rr  # noqa: E402

from hypergef_amd import synth  # noqa: E402

SYMBOLS = ("hg_gather_rows_reduce_workspace_bytes", "hg_gather_rows_reduce_f32", "hg_gather_rows_select_f32")
BF = torch.bfloat16


def small():
    """6 vertices x 5 hyperedges: hyperedge 2 is empty, hyperedge 3 lists vertex 4 twice, vertex 5 is in no hyperedge."""
    members = [[0, 1, 2], [1, 3], [], [4, 4, 0], [2, 3, 1, 0]]
    ptr = np.cumsum([0] + [len(m) for m in members]).astype(np.int32)
    return synth.Incidence(6, 5, ptr, np.concatenate([np.asarray(m, np.int32) for m in members]))


def test_exports(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hg_aggr.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert "%s(" % name in header, name
    for name, value in (("HG_REDUCE_MAX", 1), ("HG_REDUCE_MIN", 2)):
        assert getattr(_lib, name) == value and "#define %s %d" % (name, value) in header, name
    assert L.hg_version() == 410  # detected by symbol: the version does not move
    for name in ("reduce_aggr", "incidence_gather", "HyperGsysUniSAGE"):
        assert hasattr(hg, name), name
    assert hg.reduce_aggr is hg.ops.reduce_aggr and hg.HyperGsysUniSAGE is hg.models.HyperGsysUniSAGE
    for name in ("gather_rows_reduce", "gather_rows_select", "row_recip"):
        assert hasattr(hg.Plan, name), name


def test_incidence_gather_refusals(hg):
    ops = hg.ops
    inc = small()
    ptr, ind = torch.from_numpy(inc.csrptr), torch.from_numpy(inc.colind)
    x, w = torch.zeros(inc.N, 8), torch.zeros(inc.nnz)
    with pytest.raises(ValueError, match="reduce must be one of"):
        ops.incidence_gather(ptr, ind, x, reduce="prod")
    for op in ("max", "min"):
        with pytest.raises(ValueError, match="takes no weight"):
            ops.incidence_gather(ptr, ind, x, w, reduce=op)
        with pytest.raises(TypeError, match="no bfloat16 form"):
            ops.incidence_gather(ptr, ind, x.to(BF), reduce=op)
        with pytest.raises(TypeError, match="no bfloat16 form"):  # 'rows' lets bfloat16 into the sum only
            ops.incidence_gather(ptr, ind, x.to(BF), reduce=op, options=ops.Options(incidence_bf16="rows"))
        with pytest.raises(ValueError, match="heads"):
            ops.incidence_gather(ptr, ind, x, reduce=op, heads=2)
        with pytest.raises(RuntimeError, match="GPU"):  # what is left is the device
            ops.incidence_gather(ptr, ind, x, reduce=op)
    with pytest.raises(ValueError, match="scale_b must be None"):
        ops.incidence_gather(ptr, ind, x, reduce="mean", scale_b=torch.zeros(inc.M))
    with pytest.raises(TypeError, match="no bfloat16 form"):  # the TypeError of today's call
        ops.incidence_gather(ptr, ind, x.to(BF), reduce="mean")
    for r in ("sum", "mean"):
        with pytest.raises(ValueError, match="return_index"):
            ops.incidence_gather(ptr, ind, x, reduce=r, return_index=True)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_gather(ptr, ind, x, reduce="mean")


def test_reduce_aggr_refusals(hg):
    ops = hg.ops
    inc = small()
    ptr, ind = torch.from_numpy(inc.csrptr), torch.from_numpy(inc.colind)
    x = torch.zeros(inc.N, 8)
    with pytest.raises(ValueError, match="first must be one of"):
        ops.reduce_aggr(ptr, ind, x, first="median")
    with pytest.raises(ValueError, match="second must be one of"):
        ops.reduce_aggr(ptr, ind, x, second="prod")
    with pytest.raises(TypeError, match="no bfloat16 form"):
        ops.reduce_aggr(ptr, ind, x.to(BF), first="max")
    with pytest.raises(ValueError, match="num_nodes"):
        ops.reduce_aggr(ptr, ind, x, num_nodes=inc.N + 1)
    for first, second in (("max", "sum"), ("mean", "min"), ("sum", "mean")):
        with pytest.raises(RuntimeError, match="GPU"):
            ops.reduce_aggr(ptr, ind, x, first=first, second=second)
    with pytest.raises(ValueError, match="first_aggr"):
        hg.HyperGsysUniSAGE(None, 4, 4, first_aggr="median")


def test_c_entries_refuse_on_a_host_only_plan(hg):
    """The order: a null plan, the hop and the op (arguments: HG_ERR_INVALID) before the plan's kind (HG_ERR_UNSUPPORTED);
    nothing is read or written."""
    from hypergef_amd import _lib
    from hypergef_amd.plan import Plan, make_opts
    L = _lib.lib()
    inc = small()
    plan = Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True))
    buf = np.zeros(64, np.float32)  # a non-null host address: never read, every call is refused before
    some, null = buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p()

    def reduce(h, hop, op):
        return L.hg_gather_rows_reduce_f32(h, hop, 8, op, some, some, some, null, null, some, some, some, 1 << 20, null)

    def select(h, hop):
        return L.hg_gather_rows_select_f32(h, hop, 8, some, some, some, some, some, some, 1 << 20, null)

    for op in (_lib.HG_REDUCE_MAX, _lib.HG_REDUCE_MIN):
        for hop in (0, 1):
            assert reduce(plan._h, hop, op) == _lib.HG_ERR_UNSUPPORTED
            assert b"HG_PLAN_HOST_ONLY" in L.hg_last_error()
    for hop in (0, 1):
        assert select(plan._h, hop) == _lib.HG_ERR_UNSUPPORTED
        assert b"HG_PLAN_HOST_ONLY" in L.hg_last_error()
    for op in (0, 3, -1):
        assert reduce(plan._h, 0, op) == _lib.HG_ERR_INVALID
        assert b"op must be" in L.hg_last_error()
    for hop in (2, -1):
        assert reduce(plan._h, hop, 0) == _lib.HG_ERR_INVALID  # the hop before the op
        assert b"hop must be" in L.hg_last_error()
        assert select(plan._h, hop) == _lib.HG_ERR_INVALID
        assert b"hop must be" in L.hg_last_error()
    assert reduce(null, 2, 0) == _lib.HG_ERR_INVALID and b"null plan" in L.hg_last_error()
    assert select(null, 2) == _lib.HG_ERR_INVALID and b"null plan" in L.hg_last_error()
    assert L.hg_gather_rows_reduce_workspace_bytes(null, 8) == 0
    assert L.hg_gather_rows_reduce_workspace_bytes(plan._h, 0) == 0
    # two tables of partial slots, a multiple of 256 each; hg_aggr_incidence_workspace_bytes keeps its answer
    assert L.hg_gather_rows_reduce_workspace_bytes(plan._h, 8) % 512 == 0
    assert L.hg_aggr_incidence_workspace_bytes(plan._h, 8) == 256 * 3
    assert not buf.any()


@pytest.mark.parametrize("op", ["max", "min"])
@pytest.mark.parametrize("hop", [0, 1])
def test_reference_agrees_with_the_loops(hop, op):
    inc = small()
    rng = np.random.default_rng(5)
    nsrc = inc.N if hop == 0 else inc.M
    for kind in ("randn", "ties", "inf"):
        if kind == "randn":
            src = rng.standard_normal((nsrc, 5)).astype(np.float32)
        elif kind == "ties":
            src = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), size=(nsrc, 5))
        else:
            src = rng.choice(np.array([-np.inf, np.inf, 0.5], np.float32), size=(nsrc, 5))
            src[:, 0] = -np.inf
        want_v, want_a = rr.brute_force(inc, hop, src, op)
        got_v, got_a = rr.reduce_hop(inc, hop, torch.from_numpy(src), op)
        assert np.array_equal(got_a.numpy(), want_a), (kind, hop, op)
        assert np.array_equal(got_v.numpy().view(np.int32), want_v.view(np.int32)), (kind, hop, op)
        # empty rows: hyperedge 2, vertex 5
        empty = 2 if hop == 0 else 5
        assert (want_a[empty] == -1).all() and not want_v[empty].view(np.int32).any()
        # the gradient lands once per (row, column) with a winner, on the winner's source row
        g = torch.from_numpy(rng.integers(-3, 4, size=want_a.shape).astype(np.float64))
        d = rr.select_grad(inc, hop, g, got_a)
        want_d = np.zeros((nsrc, 5))
        rows = np.repeat(np.arange(inc.M), np.diff(inc.csrptr))
        other = inc.colind if hop == 0 else rows
        for r in range(want_a.shape[0]):
            for c in range(5):
                if want_a[r, c] >= 0:
                    want_d[other[want_a[r, c]], c] += g[r, c].item()
        assert np.array_equal(d.numpy(), want_d), (kind, hop, op)
    # the duplicate: hyperedge 3 lists vertex 4 at positions 5 and 6; under ties the first wins
    if hop == 0:
        src = np.zeros((inc.N, 1), np.float32)
        _, a = rr.reduce_hop(inc, 0, torch.from_numpy(src), op)
        assert int(a[3, 0]) == 5
