"""bf16 aggregation entry point, host side (no GPU): declared, exported, and refusing plans it cannot run on."""
import os
import re

from conftest import ROOT
from hypergef_amd import synth


def test_bf16_entry_point_declared_and_exported(hg):
    from hypergef_amd import _lib
    header = open(os.path.join(ROOT, "include", "hg_aggr.h")).read()
    assert re.search(r"HG_API int hg_aggr_fused_bf16\s*\(", header)
    assert "hg_aggr_fused_bf16" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "hg_aggr_fused_bf16")


def test_bf16_entry_point_rejects_null_and_host_only_plans(hg):
    from hypergef_amd import _lib, plan as planmod
    L = _lib.lib()
    rc = L.hg_aggr_fused_bf16(None, 32, None, None, None, None, None, None, None, None, 0, 0, None)
    assert rc == _lib.HG_ERR_INVALID
    assert b"null plan" in L.hg_last_error()
    inc = synth.cora_shape()
    plan = planmod.Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, planmod.make_opts(host_only=True))
    for variant in (_lib.HG_VARIANT_AUTO, _lib.HG_VARIANT_FUSED, _lib.HG_VARIANT_PULL):
        rc = L.hg_aggr_fused_bf16(plan._h, 32, None, None, None, None, None, None, None, None, 0, variant, None)
        assert rc == _lib.HG_ERR_INVALID
        assert b"HG_PLAN_HOST_ONLY" in L.hg_last_error()
    # the workspace size is the fp32 call's: one query answers for both forms
    assert plan.workspace_bytes(32) >= inc.M * 32 * 4


def test_bf16_entry_point_refuses_push_atomic_without_a_device(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    rc = L.hg_aggr_fused_bf16(None, 32, None, None, None, None, None, None, None, None, 0,
                              _lib.HG_VARIANT_PUSH_ATOMIC, None)
    assert rc == _lib.HG_ERR_UNSUPPORTED
    assert b"fp32 only" in L.hg_last_error()


def test_bf16_passes_the_dtype_check_fp16_and_fp64_do_not(hg):
    """Plan.aggregate checks the dtype before anything touches a device: float16 / float64 are refused with a TypeError
    that names both accepted dtypes; bf16 gets past it (and is refused only for being on the CPU)."""
    import pytest
    import torch
    from hypergef_amd import plan as planmod
    inc = synth.cora_shape()
    plan = planmod.Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, planmod.make_opts(host_only=True))
    ptr, ind = torch.from_numpy(inc.csrptr), torch.from_numpy(inc.colind)
    for dt in (torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32 or bfloat16"):
            plan.aggregate(ptr, ind, torch.zeros(inc.N, 8, dtype=dt))
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        plan.aggregate(ptr, ind, torch.zeros(inc.N, 8, dtype=torch.bfloat16))
    # the linear-folded entry point stays fp32
    with pytest.raises(TypeError, match="float32 tensor"):
        plan.aggregate_linear(ptr, ind, torch.zeros(inc.N, 32, dtype=torch.bfloat16), torch.zeros(16, 32))
