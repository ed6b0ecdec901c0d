"""bf16 feature rows on the incidence path without a device: the exported symbols, Options.incidence_bf16, the default that
still refuses with the pinned TypeErrors, and what 'rows' still refuses before a device is touched."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402

BF16_SYMBOLS = ("hg_gather_rows_incidence_heads_bf16", "hg_aggr_incidence_heads_bf16", "hg_incidence_dot_heads_bf16")
BF = torch.bfloat16


def _host_tensors():
    inc = ar.toy()
    return inc, torch.from_numpy(inc.csrptr), torch.from_numpy(inc.colind)


def test_exports(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hg_aggr.h")).read()
    for name in BF16_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert "HG_API int %s(" % name in header, name
    for name, value in (("HG_ROWS_SRC_BF16", 1), ("HG_ROWS_DST_BF16", 2), ("HG_DOT_A_BF16", 1), ("HG_DOT_B_BF16", 2)):
        assert getattr(_lib, name) == value and "#define %s %d" % (name, value) in header, name
    assert L.hg_version() == 410  # detected by symbol: the version does not move


def test_the_option(hg, monkeypatch):
    ops = hg.ops
    assert ops.Options().incidence_bf16 == "refuse" and ops.Options(incidence_bf16="rows").incidence_bf16 == "rows"
    assert ops.Options._CHOICES["incidence_bf16"] == ("refuse", "rows")
    assert "incidence_bf16" in ops.Options.__doc__
    with pytest.raises(ValueError, match="incidence_bf16"):
        ops.Options(incidence_bf16="sometimes")
    with ops.options(incidence_bf16="rows") as o:
        assert o.incidence_bf16 == "rows" and ops.current_options().incidence_bf16 == "rows"
    assert ops.current_options().incidence_bf16 == "refuse"
    # the environment sets the process default, like its neighbours: read in a fresh interpreter that loads no library
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (("rows", "rows"), ("refuse", "refuse"), ("sometimes", "refuse")):
        env = dict(os.environ, HG_INCIDENCE_BF16=value)
        out = subprocess.run([sys.executable, "-c", "from hypergef_amd import ops; print(ops.current_options().incidence_bf16)"],
                             cwd=root, env=env, capture_output=True, text=True, check=True).stdout.strip()
        assert out == want, (value, out)


def test_the_default_still_refuses(hg):
    ops = hg.ops
    inc, ptr, ind = _host_tensors()
    N, M, nnz = inc.N, inc.M, inc.nnz
    x, xe, w = torch.zeros(N, 8), torch.zeros(M, 8), torch.zeros(nnz)
    with pytest.raises(TypeError, match="node_feat must be a float32 tensor \\(incidence_aggr has no bfloat16 form\\)"):
        ops.incidence_aggr(ptr, ind, x.to(BF), w, w)
    with pytest.raises(TypeError, match="src must be a float32 tensor \\(incidence_gather has no bfloat16 form\\)"):
        ops.incidence_gather(ptr, ind, x.to(BF), w)
    with pytest.raises(TypeError, match="A must be a float32 tensor \\(incidence_dot has no bfloat16 form\\)"):
        ops.incidence_dot(ptr, ind, x.to(BF), xe)
    with pytest.raises(TypeError, match="B must be a float32 tensor \\(incidence_dot has no bfloat16 form\\)"):
        ops.incidence_dot(ptr, ind, x, xe.to(BF))
    with pytest.raises(TypeError, match="no bfloat16 form"):
        ops.incidence_aggr(ptr, ind, x.to(BF), w, w, options=ops.Options(incidence_bf16="refuse"))


def test_rows_still_refuses_before_a_device_is_touched(hg):
    ops = hg.ops
    inc, ptr, ind = _host_tensors()
    N, M, nnz = inc.N, inc.M, inc.nnz
    rows = ops.Options(incidence_bf16="rows")
    xb, xeb, w = torch.zeros(N, 8, dtype=BF), torch.zeros(M, 8, dtype=BF), torch.zeros(nnz)
    # bf16 weights (and scales) stay a TypeError
    for kw in (dict(v2e_weight=w.to(BF)), dict(e2v_weight=w.to(BF))):
        with pytest.raises(TypeError, match="no bfloat16 form"):
            ops.incidence_aggr(ptr, ind, xb, options=rows, **kw)
    with pytest.raises(TypeError, match="weight must be a float32 tensor"):
        ops.incidence_gather(ptr, ind, xb, w.to(BF), options=rows)
    with pytest.raises(TypeError, match="scale_a must be a float32 tensor"):
        ops.incidence_gather(ptr, ind, xb, w, scale_a=torch.zeros(M, dtype=BF), options=rows)
    # other 16-bit and 64-bit rows are not let through by 'rows'
    with pytest.raises(TypeError, match="no bfloat16 form"):
        ops.incidence_aggr(ptr, ind, xb.to(torch.float16), w, w, options=rows)
    with pytest.raises(TypeError, match="no bfloat16 form"):
        ops.incidence_dot(ptr, ind, xb.double(), xeb, options=rows)
    # width mismatches
    with pytest.raises(ValueError, match="multiple of heads"):
        ops.incidence_aggr(ptr, ind, xb, torch.zeros(nnz, 3), None, heads=3, options=rows)
    with pytest.raises(ValueError, match="multiple of heads"):
        ops.incidence_gather(ptr, ind, xb, torch.zeros(nnz, 3), heads=3, options=rows)
    with pytest.raises(ValueError, match="A must be"):
        ops.incidence_dot(ptr, ind, xb, torch.zeros(M, 12, dtype=BF), options=rows)
    with pytest.raises(ValueError, match="multiple of heads"):
        ops.incidence_dot(ptr, ind, xb, xeb, heads=3, options=rows)
    # the pull kernels only
    fused = ops.Options(incidence_bf16="rows", variant="fused")
    with pytest.raises(ValueError, match="variant"):
        ops.incidence_aggr(ptr, ind, xb, w, w, options=fused)
    with pytest.raises(ValueError, match="variant"):
        ops.incidence_gather(ptr, ind, xb, w, options=fused)
    # what is left is the device: the tensors of this test live on the host
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_aggr(ptr, ind, xb, w, w, options=rows)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_gather(ptr, ind, xb, w, options=rows)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_dot(ptr, ind, xb, xeb, options=rows)
    # the operators beside them stay float32 only under 'rows'
    with ops.options(incidence_bf16="rows"):
        with pytest.raises(TypeError, match="bfloat16"):
            ops.incidence_softmax(ptr, ind, torch.zeros(N, dtype=BF), torch.zeros(M))
        with pytest.raises(TypeError, match="bfloat16"):
            ops.incidence_sum(ptr, ind, w.to(BF), num_nodes=N)
        with pytest.raises(TypeError, match="no bfloat16 form"):
            ops.incidence_attention_aggr(ptr, ind, xb, torch.zeros(N), torch.zeros(M))


def test_c_entries_refuse_on_a_host_only_plan(hg):
    """check_heads' order: a bad io first (an argument, like hop), then the plan's kind; nothing is read or written."""
    from hypergef_amd import _lib
    from hypergef_amd.plan import Plan, make_opts
    L = _lib.lib()
    inc = ar.toy()
    plan = Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True))
    buf = np.zeros(64, np.float32)  # a non-null host address: never read, every call is refused before
    some, null = buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p()
    for io in (1, 2, 3):
        assert L.hg_gather_rows_incidence_heads_bf16(plan._h, 0, 8, 2, some, some, some, some, null, null, some, null, 0, io,
                                                     null) == _lib.HG_ERR_UNSUPPORTED
        assert b"HG_PLAN_HOST_ONLY" in L.hg_last_error()
        assert L.hg_incidence_dot_heads_bf16(plan._h, 8, 2, some, some, some, some, some, io, null) == _lib.HG_ERR_UNSUPPORTED
        assert b"HG_PLAN_HOST_ONLY" in L.hg_last_error()
    assert L.hg_aggr_incidence_heads_bf16(plan._h, 8, 2, some, some, some, some, some, null, null, null, null, some, null, 0,
                                          null) == _lib.HG_ERR_UNSUPPORTED
    assert b"HG_PLAN_HOST_ONLY" in L.hg_last_error()
    for io in (0, 4, -1):
        assert L.hg_gather_rows_incidence_heads_bf16(plan._h, 0, 8, 2, some, some, some, some, null, null, some, null, 0, io,
                                                     null) == _lib.HG_ERR_INVALID
        assert b"io must be" in L.hg_last_error()
        assert L.hg_incidence_dot_heads_bf16(plan._h, 8, 2, some, some, some, some, some, io, null) == _lib.HG_ERR_INVALID
        assert b"io must be" in L.hg_last_error()
    assert L.hg_gather_rows_incidence_heads_bf16(plan._h, 2, 8, 2, some, some, some, some, null, null, some, null, 0, 1,
                                                 null) == _lib.HG_ERR_INVALID  # hop, decided first
    assert b"hop must be" in L.hg_last_error()
    assert not buf.any()
