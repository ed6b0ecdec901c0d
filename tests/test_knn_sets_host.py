"""ops.knn(set_rows=) without a device: what is refused before a device is touched and where in the order, and the C
entries' refusal codes and workspace bound (hg_knn_sets_f32, hg_knn_dot_sets_f32 / _bf16, hg_knn_dot_sets_workspace_bytes)."""
import ctypes

import numpy as np
import pytest
import torch

ENTRIES = ("hg_knn_sets_f32", "hg_knn_dot_sets_f32", "hg_knn_dot_sets_bf16")
X = torch.zeros(12, 4)
# in the order ops.knn decides them: every refusal of today before the first of set_rows
REFUSALS = [
    (TypeError, "float32", dict(X=X.double(), set_rows=5)),
    (ValueError, "form must be one of", dict(set_rows=5, form="auto")),
    (ValueError, "k must be an integer", dict(k=0, set_rows=5)),
    (ValueError, "queries must be", dict(set_rows=4, queries=torch.zeros(3, 5))),
    (ValueError, 'form="dot" cannot be combined with segments', dict(set_rows=5, segments=[0, 6, 12], form="dot")),
    (ValueError, "segment 0 has 2 rows", dict(set_rows=5, segments=[0, 2, 12])),
    (ValueError, "cand_slices must be", dict(set_rows=5, cand_slices=33)),
    (ValueError, "set_rows must be an integer", dict(set_rows=2.5)),
    (ValueError, "exceeds the set_rows", dict(set_rows=2)),
    (ValueError, "no multiple of set_rows = 5", dict(set_rows=5)),
    (ValueError, "set_rows cannot be combined with queries", dict(set_rows=4, queries=torch.zeros(3, 4))),
    (ValueError, "set_rows cannot be combined with segments", dict(set_rows=4, segments=[0, 4, 8, 12])),
    (TypeError, "float32", dict(X=X.bfloat16(), set_rows=4)),  # bfloat16 rows stay the dot form's
    (RuntimeError, "GPU", dict(set_rows=12, form="dot", return_fallback=True, return_mean=True)),  # what is left is the device
    (RuntimeError, "GPU", dict(X=X.bfloat16(), set_rows=4, form="dot")),
]


@pytest.mark.parametrize("error,match,kw", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_fire_without_a_device_and_in_order(hg, error, match, kw):
    kw = dict(kw)
    with pytest.raises(error, match=match):
        hg.ops.knn(kw.pop("X", X), kw.pop("k", 3), **kw)


def test_the_layers_pass_set_rows_on(hg):
    with pytest.raises(ValueError, match="no multiple of set_rows"):
        hg.KnnHypergraph.build(X, 3, set_rows=5)
    with pytest.raises(ValueError, match="no multiple of set_rows"):
        hg.HyperGraph.from_knn(X, 3, "cpu", set_rows=5, form="dot")
    for device_graph in (False, True):
        layer = hg.DynamicHypergraphConv(4, 4, 3, device_graph=device_graph, set_rows=5)
        assert list(layer.state_dict()) == list(hg.DynamicHypergraphConv(4, 4, 3).state_dict())
        with pytest.raises(ValueError, match="no multiple of set_rows"):
            layer(X)


@pytest.mark.parametrize("entry", ENTRIES)
def test_c_entry_refusals(hg, entry):
    from hypergef_amd import _lib
    L = _lib.lib()
    assert entry in _lib.SYMBOLS and L.hg_version() == 410
    n, F = 12, 4
    rows = np.zeros((n, F), np.float32 if entry.endswith("f32") else np.uint16)
    idx, dist = np.zeros((n, 64), np.int32), np.zeros((n, 64), np.float32)
    ws = np.zeros(1 << 16, np.uint8)
    null = ctypes.c_void_p()
    p = lambda a: null if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def call(k=3, set_rows=4, x=rows, out=idx, slices=2, workspace=ws):
        tail = (p(workspace), 0 if workspace is None else workspace.nbytes, null)
        return getattr(L, entry)(p(x), n, F, k, set_rows, 1, slices, p(out), p(dist), null, *((null,) if "dot" in entry else ()), *tail)

    INV, UNS = _lib.HG_ERR_INVALID, _lib.HG_ERR_UNSUPPORTED
    assert call(x=None) == INV and call(out=None) == INV and b"null" in L.hg_last_error()
    assert call(k=0) == INV and entry.encode() + b": k must be in 1 .. 64" in L.hg_last_error()
    assert call(k=13) == INV and b"exceeds" in L.hg_last_error()
    assert call(slices=33, set_rows=5) == UNS  # the sibling's refusals first, then the sets' own
    assert call(set_rows=0) == INV and b"set_rows must be at least 1" in L.hg_last_error()
    assert call(set_rows=5) == INV and b"no multiple of set_rows = 5" in L.hg_last_error()
    assert call(set_rows=2) == INV and b"fewer than k = 3" in L.hg_last_error()
    assert call(workspace=None) == _lib.HG_ERR_WORKSPACE
    assert call(workspace=np.zeros(8, np.uint8)) == _lib.HG_ERR_WORKSPACE and b"asks for" in L.hg_last_error()
    assert not idx.any() and not dist.any() and not ws.any()


def test_dot_sets_workspace_bytes(hg):
    """4 (n + B) + slices n (8 kp + 4) and the rounding of five pieces: nothing of m x m or n x n; 0 for what the entries refuse."""
    from hypergef_amd import _lib
    size = _lib.lib().hg_knn_dot_sets_workspace_bytes
    for B, m, k in ((1, 1, 1), (1, 100000, 64), (1024, 32, 10), (32, 1024, 17), (3, 129, 49), (50000, 1, 1)):
        kp = min(m, 32 * ((k + 16 + 31) // 32))
        for cs in (0, 1, 32):
            assert 0 < size(B * m, 1024, k, cs, m) <= 4 * (B * m + B) + 32 * B * m * (8 * kp + 4) + 1280, (B, m, k, cs)
    for args in ((0, 4, 1, 0, 1), (12, 0, 1, 0, 4), (12, 65537, 1, 0, 4), (12, 4, 0, 0, 4), (12, 4, 1, 33, 4), (12, 4, 1, 0, 0),
                 (12, 4, 1, 0, 5), (12, 4, 5, 0, 4)):
        assert size(*args) == 0, args
