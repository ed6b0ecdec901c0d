"""The linear layer on bf16 rows (hg_aggr_linear_res_bf16 and its companions), host side (no GPU): declared, exported,
sized, and refusing what it cannot run -- in the order include/hg_aggr.h documents -- before a device is touched."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from hypergef_amd import synth

SYMBOLS = ("hg_linear_pack_bf16_bytes", "hg_linear_pack_bf16", "hg_aggr_linear_res_bf16", "hg_linear_rows_bf16",
           "hg_aggr_linear_bf16_path")


def test_the_five_symbols_are_declared_and_exported(hg):
    from hypergef_amd import _lib
    header = open(os.path.join(ROOT, "include", "hg_aggr.h")).read()
    L = _lib.lib()
    for name in SYMBOLS:
        assert re.search(r"HG_API (int|size_t) %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name


def test_pack_bytes(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    for F_in in (32, 64, 128):
        for F_out in (16, 64, 80, 128, 256):
            assert L.hg_linear_pack_bf16_bytes(F_out, F_in) == F_out * F_in * 2
    for F_out, F_in in ((16, 16), (16, 96), (16, 256), (24, 32), (0, 32), (-16, 32), (16, 0)):
        assert L.hg_linear_pack_bf16_bytes(F_out, F_in) == 0, (F_out, F_in)


def test_options_field(hg):
    from hypergef_amd import ops
    assert ops.Options().linear_bf16 == "torch"
    assert ops.Options(linear_bf16="mfma").linear_bf16 == "mfma"
    assert "linear_bf16" in ops.Options._CHOICES
    with pytest.raises(ValueError, match="linear_bf16"):
        ops.Options(linear_bf16="x")


def _call(L, plan, F_in=128, F_out=64, ptr=1, ind=1, X=8, wfrag=16, R=None, flags=0, T_out=None, Y=8, ws=None, nbytes=0,
          variant=0):
    """hg_aggr_linear_res_bf16 with made-up addresses (never dereferenced: every case here is refused first)."""
    return L.hg_aggr_linear_res_bf16(plan, F_in, F_out, ptr, ind, X, None, None, None, wfrag, R, 1.0, 0.0, None, flags,
                                     T_out, Y, ws, nbytes, variant, None)


def test_refusal_order_on_a_host_only_plan(hg):
    from hypergef_amd import _lib, plan as planmod
    L = _lib.lib()
    inc = synth.cora_shape()
    plan = planmod.Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, planmod.make_opts(host_only=True))
    h = plan._h
    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED
    # 1. null plan / arrays and bad flags: INVALID, whatever else is wrong with the call
    assert _call(L, None, F_in=48, variant=_lib.HG_VARIANT_PUSH_ATOMIC) == INV
    for kw in (dict(ptr=None), dict(ind=None), dict(X=None), dict(wfrag=None), dict(Y=None)):
        assert _call(L, h, F_in=48, **kw) == INV, kw
        assert b"null argument" in L.hg_last_error()
    for flags in (2, 3, 4, -1):  # HG_LIN_BF16X6 and everything else but HG_LIN_RELU
        assert _call(L, h, flags=flags, F_in=48) == INV
        assert b"HG_LIN_RELU" in L.hg_last_error()
    # 2. variant and widths: UNSUPPORTED, before alignment and before the host-only plan is noticed
    assert _call(L, h, variant=_lib.HG_VARIANT_PUSH_ATOMIC, X=2) == UNS
    assert b"variant" in L.hg_last_error()
    for F_in, F_out in ((16, 16), (48, 16), (256, 16), (32, 8), (32, 24), (32, 0)):
        assert _call(L, h, F_in=F_in, F_out=F_out, X=2) == UNS
        assert b"F_in in {32, 64, 128}" in L.hg_last_error()
    # 3. alignment: X, Y, R, T_out 8 bytes, wfrag 16
    for kw in (dict(X=4), dict(Y=12), dict(R=2), dict(T_out=4), dict(wfrag=8)):
        assert _call(L, h, **kw) == UNS, kw
        assert b"aligned" in L.hg_last_error()
    # 4. the host-only plan itself
    for flags in (0, 1):
        assert _call(L, h, flags=flags, R=8, T_out=8) == UNS
        assert b"HG_PLAN_HOST_ONLY" in L.hg_last_error()
    # the path query needs no device: it answers on the host-only plan
    for F_in in (32, 64):
        assert L.hg_aggr_linear_bf16_path(h, F_in, 32, _lib.HG_VARIANT_FUSED) == 2
    assert L.hg_aggr_linear_bf16_path(h, 128, 32, _lib.HG_VARIANT_PULL) == 2
    assert L.hg_aggr_linear_bf16_path(h, 128, 256, _lib.HG_VARIANT_FUSED) == 2  # wider than the panels' staged form
    assert L.hg_aggr_linear_bf16_path(h, 128, 24, _lib.HG_VARIANT_FUSED) == UNS
    assert L.hg_aggr_linear_bf16_path(h, 128, 32, _lib.HG_VARIANT_PUSH_ATOMIC) == UNS
    assert L.hg_aggr_linear_bf16_path(None, 128, 32, 0) == INV


def test_rows_and_pack_entries_refuse_without_a_device(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    assert L.hg_linear_pack_bf16(16, 32, None, 16, None) == _lib.HG_ERR_INVALID
    assert L.hg_linear_pack_bf16(16, 48, 16, 16, None) == _lib.HG_ERR_UNSUPPORTED
    assert L.hg_linear_pack_bf16(16, 32, 16, 8, None) == _lib.HG_ERR_UNSUPPORTED
    assert L.hg_linear_rows_bf16(-1, 32, 16, 8, 16, 8, None) == _lib.HG_ERR_INVALID
    assert L.hg_linear_rows_bf16(4, 32, 16, None, 16, 8, None) == _lib.HG_ERR_INVALID
    assert L.hg_linear_rows_bf16(4, 32, 24, 8, 16, 8, None) == _lib.HG_ERR_UNSUPPORTED
    assert L.hg_linear_rows_bf16(4, 32, 16, 4, 16, 8, None) == _lib.HG_ERR_UNSUPPORTED
    assert L.hg_linear_rows_bf16(0, 32, 16, None, 16, None, None) == _lib.HG_OK  # no rows: nothing to launch


def test_plan_method_refuses_dtypes_and_shapes_before_a_device_is_touched(hg):
    import torch
    from hypergef_amd import plan as planmod
    inc = synth.cora_shape()
    plan = planmod.Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, planmod.make_opts(host_only=True))
    ptr, ind = torch.from_numpy(inc.csrptr), torch.from_numpy(inc.colind)
    bf = torch.bfloat16
    X, Wl = torch.zeros(inc.N, 32, dtype=bf), torch.zeros(16, 32, dtype=bf)
    with pytest.raises(TypeError, match="node_feat must be a bfloat16"):
        plan.aggregate_linear_bf16(ptr, ind, X.float(), Wl)
    with pytest.raises(TypeError, match="weight must be a bfloat16"):
        plan.aggregate_linear_bf16(ptr, ind, X, Wl.float())
    for t in (X.half(), Wl.half()):
        with pytest.raises(TypeError, match="bfloat16"):
            plan.aggregate_linear_bf16(ptr, ind, t if t.shape[0] == inc.N else X, t if t.shape[0] == 16 else Wl)
    with pytest.raises(TypeError, match="residual must be a bfloat16"):
        plan.aggregate_linear_bf16(ptr, ind, X, Wl, residual=X.float())
    with pytest.raises(TypeError, match="t_out must be a bfloat16"):
        plan.aggregate_linear_bf16(ptr, ind, X, Wl, t_out=X.float())
    with pytest.raises(TypeError, match="out must be a bfloat16"):
        plan.aggregate_linear_bf16(ptr, ind, X, Wl, out=torch.zeros(inc.N, 16))
    with pytest.raises(TypeError, match="cb must be float32"):
        plan.aggregate_linear_bf16(ptr, ind, X, Wl, residual=X, cb=torch.ones(1, dtype=bf))
    with pytest.raises(ValueError, match="node_feat must be"):
        plan.aggregate_linear_bf16(ptr, ind, X[:-1], Wl)
    with pytest.raises(ValueError, match="weight must be"):
        plan.aggregate_linear_bf16(ptr, ind, X, torch.zeros(16, 64, dtype=bf))
    with pytest.raises(ValueError, match="F_in in"):
        plan.aggregate_linear_bf16(ptr, ind, torch.zeros(inc.N, 48, dtype=bf), torch.zeros(16, 48, dtype=bf))
    with pytest.raises(ValueError, match="F_in in"):
        plan.aggregate_linear_bf16(ptr, ind, X, torch.zeros(24, 32, dtype=bf))
    with pytest.raises(ValueError, match="residual must be"):
        plan.aggregate_linear_bf16(ptr, ind, X, Wl, residual=torch.zeros(inc.N, 16, dtype=bf))
    with pytest.raises(ValueError, match="out must be"):
        plan.aggregate_linear_bf16(ptr, ind, X, Wl, out=torch.zeros(inc.N, 32, dtype=bf))
    with pytest.raises(ValueError, match="one element"):
        plan.aggregate_linear_bf16(ptr, ind, X, Wl, residual=X, cb=torch.ones(2))
    # everything the host can decide is in order: only now is the tensors' place looked at
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        plan.aggregate_linear_bf16(ptr, ind, X, Wl)
    # the fp32 entry keeps refusing bf16
    with pytest.raises(TypeError, match="float32 tensor"):
        plan.aggregate_linear(ptr, ind, X, Wl)
    for fn in (planmod.pack_linear_bf16, planmod.packed_linear_bf16_cached):
        with pytest.raises(TypeError, match="bfloat16"):
            fn(Wl.float())
        with pytest.raises(ValueError, match="F_in in"):
            fn(torch.zeros(16, 48, dtype=bf))
    with pytest.raises(TypeError, match="bfloat16"):
        planmod.linear_rows_bf16(X.float(), Wl)
