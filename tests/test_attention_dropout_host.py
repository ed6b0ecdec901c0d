"""Attention dropout without a device: the Philox mask against the published known answers and against its restatement in
tests/_dropout_ref.py, its rate and independence, and the refusals of ops.incidence_softmax(dropout=...) and
HypergraphAttnConv(dropout=...), all decided before a device is touched."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402
import _dropout_ref as dr  # noqa: E402

KEY = 0x0123456789ABCDEF  # the fixed key of the rate tests; test_drop_rate_and_independence holds for it
STATES = ((KEY, 0), (0xFEDCBA9876543210, 0xFFFFFFFF00000001))


def test_philox_known_answers():
    for counter, key, want in dr.KAT:
        got = dr.philox4x32_10(counter, key)
        assert tuple(int(w) for w in got) == want, (counter, key)
    # vectorised: the three at once, one key at a time
    for counter, key, want in dr.KAT:
        got = dr.philox4x32_10(tuple(np.array([c, c]) for c in counter), key)
        assert all(int(g[1]) == w for g, w in zip(got, want))


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("pd", [0.0, 0.1, 0.5, 0.9, 1.0 - 2.0 ** -24])
def test_host_mask_equals_restatement(hg, pd, heads):
    for key, sid in STATES:
        got = dr.keep_host(key, sid, pd, 1000, heads)
        want = dr.keep(key, sid, pd, 1000, heads)
        assert got.shape == (1000, heads) and np.array_equal(got, want), (pd, heads, key, sid)
        if pd == 0.0:
            assert got.all()
    assert dr.threshold(1.0 - 2.0 ** -24) == 2 ** 32 - 256 and dr.threshold(0.0) == 0 and dr.threshold(0.5) == 2 ** 31


def test_host_mask_refusals(hg):
    from hypergef_amd import _lib
    buf = np.empty(4, np.uint8)
    for pd in (-0.1, 1.0, 1.5, float("nan")):
        assert _lib.lib().hg_dropout_keep_host(1, 2, pd, 4, 1, buf.ctypes.data) == _lib.HG_ERR_INVALID
    assert _lib.lib().hg_dropout_keep_host(1, 2, 0.5, 4, 0, buf.ctypes.data) == _lib.HG_ERR_INVALID
    assert _lib.lib().hg_dropout_keep_host(1, 2, 0.5, 4, 1, None) == _lib.HG_ERR_INVALID


def test_drop_rate_and_independence(hg):
    n, pd = 1 << 20, 0.5
    sigma = math.sqrt(pd * (1 - pd) / n)
    agree = pd * pd + (1 - pd) * (1 - pd)
    sigma_agree = math.sqrt(agree * (1 - agree) / n)
    a = dr.keep_host(KEY, 7, pd, n, 2)
    b = dr.keep_host(KEY, 8, pd, n, 1)
    dropped = 1.0 - a[:, 0].mean()
    print("dropped %.6f (5 sigma %.6f); agreement sid / sid + 1 %.6f, heads 0 / 1 %.6f (5 sigma %.6f)" % (
        dropped, 5 * sigma, (a[:, 0] == b[:, 0]).mean(), (a[:, 0] == a[:, 1]).mean(), 5 * sigma_agree))
    assert abs(dropped - pd) <= 5 * sigma
    assert abs((a[:, 0] == b[:, 0]).mean() - agree) <= 5 * sigma_agree
    assert abs((a[:, 0] == a[:, 1]).mean() - agree) <= 5 * sigma_agree


def test_refusals_need_no_device(hg, monkeypatch):
    from hypergef_amd import ops
    monkeypatch.setattr(ops, "cached_plan", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device touched")))
    inc = ar.toy()
    ptr, ind = torch.from_numpy(inc.csrptr), torch.from_numpy(inc.colind)
    sv, se = torch.zeros(inc.N), torch.zeros(inc.M)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="dropout"):
            ops.incidence_softmax(ptr, ind, sv, se, dropout=bad)
    with pytest.raises(ValueError, match="infinite"):
        ops.incidence_softmax(ptr, ind, sv, se, dropout=1.0)
    with pytest.raises(TypeError, match="rng_state"):
        ops.incidence_softmax(ptr, ind, sv, se, dropout=0.5, rng_state=torch.zeros(2))
    with pytest.raises(ValueError, match="rng_state"):
        ops.incidence_softmax(ptr, ind, sv, se, dropout=0.5, rng_state=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU"):  # a good state, CPU tensors: refused as by every operator
        ops.incidence_softmax(ptr, ind, sv, se, dropout=0.5, rng_state=torch.zeros(2, dtype=torch.int64))
    # dropout = 0.0 and training=False are today's call: its refusal of CPU tensors, no look at rng_state
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_softmax(ptr, ind, sv, se, dropout=0.0)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_softmax(ptr, ind, sv, se, dropout=0.5, training=False)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.incidence_softmax(ptr, ind, sv, se, dropout=0.0, rng_state=torch.zeros(2))


def test_layer_refuses_dropout_one(hg):
    class _H:  # refused before the hypergraph is looked at
        pass
    with pytest.raises(ValueError, match="dropout"):
        hg.HypergraphAttnConv(_H(), 4, 4, dropout=1.0)
    with pytest.raises(ValueError, match="dropout"):
        hg.HypergraphAttnConv(_H(), 4, 4, dropout=-0.5)


def test_exports(hg):
    from hypergef_amd import _lib
    for name in ("hg_incidence_attention_dropout_heads_f32", "hg_incidence_attention_dropout_heads_bwd_f32",
                 "hg_dropout_keep_host"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    from hypergef_amd.plan import Plan
    assert hasattr(Plan, "incidence_attention_dropout") and hasattr(Plan, "incidence_attention_dropout_backward")
