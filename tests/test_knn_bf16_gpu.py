"""ops.knn(form="dot") on bfloat16 rows on the device (include/hg_aggr.h, hg_knn_dot_bf16): idx and dist are those of the
float32 difference-form search of the widened rows, bit for bit; the fallback is the host model's; the matrix unit's sums
stay inside the bound E1b derived from hypothesis H; the raw entry stays inside its buffers; and the layers take bfloat16."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_bf16_ref as br  # noqa: E402
import _raw_table as raw  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def _rows(kind, n, F, seed):
    rng = np.random.default_rng(seed)
    if kind == "integer":  # many exact ties
        X = rng.integers(-2, 3, (n, F)).astype(np.float64)
    elif kind == "duplicates":  # every row twice (an odd n: the last row once)
        X = np.concatenate([rng.standard_normal(((n + 1) // 2, F))] * 2)[:n]
    elif kind == "offset":  # bfloat16 spacing 0.5: many ties at the shortlist's edge
        X = rng.standard_normal((n, F)) + 100.0
    elif kind == "outlier":  # one row of norm 1e4 among unit rows
        X = rng.standard_normal((n, F))
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        X[n // 2] *= 1e4
    elif kind == "overflow":  # squared norms at or above 1e37
        X = rng.standard_normal((n, F)) * (4e18 / np.sqrt(F))
    else:
        X = rng.standard_normal((n, F))
    return torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(DEV).to(BF)


def _same(hg, Xb, k, **kw):
    Qb = kw.pop("queries", None)
    got = hg.ops.knn(Xb, k, queries=Qb, form="dot", return_fallback=True, **kw)
    want = hg.ops.knn(Xb.float(), k, queries=None if Qb is None else Qb.float(), form="difference", **kw)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32
    assert torch.equal(got[0], want[0]), (tuple(Xb.shape), k, kw)
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (tuple(Xb.shape), k, kw)
    return got


# (kind, n, F, k, nq or None, self_first or None, cand_slices)
CELLS = [
    ("randn", 1, 1, 1, None, None, 0), ("randn", 31, 7, 10, None, None, 1), ("randn", 33, 8, 16, None, False, 3),
    ("randn", 127, 15, 17, None, None, 0), ("randn", 129, 16, 48, None, None, 32), ("randn", 300, 17, 49, None, False, 3),
    ("randn", 1000, 31, 64, None, None, 0), ("randn", 1000, 64, 10, None, None, 32), ("randn", 300, 65, 10, 129, None, 3),
    ("randn", 1000, 200, 16, 1, None, 0), ("randn", 300, 1024, 10, None, None, 1), ("randn", 129, 1024, 64, 129, None, 0),
    ("integer", 300, 8, 17, None, None, 3), ("integer", 1000, 17, 48, None, False, 0), ("integer", 127, 64, 10, 129, None, 1),
    ("duplicates", 300, 16, 10, None, None, 0), ("duplicates", 129, 65, 49, None, False, 32), ("duplicates", 1000, 7, 1, 1, None, 3),
    ("offset", 300, 64, 10, None, None, 0), ("offset", 1000, 200, 16, None, False, 3), ("offset", 33, 31, 17, 129, None, 1),
    ("outlier", 300, 64, 10, None, None, 0), ("outlier", 1000, 15, 48, None, None, 32), ("outlier", 129, 200, 10, 1, None, 1),
    ("overflow", 300, 64, 10, None, None, 0), ("overflow", 127, 17, 16, 129, None, 3),
]


@pytest.mark.parametrize("kind,n,F,k,nq,self_first,cs", CELLS)
def test_bits_equal_the_float32_difference_search(hg, kind, n, F, k, nq, self_first, cs):
    Xb = _rows(kind, n, F, 11)
    kw = dict(cand_slices=cs)
    if nq is not None:
        kw["queries"] = _rows(kind, nq, F, 12)
    elif self_first is not None:
        kw["self_first"] = self_first
    _same(hg, Xb, k, **kw)


def test_a_base_that_is_only_two_byte_aligned(hg):
    for n, F, k in ((300, 64, 10), (129, 17, 16), (200, 1024, 10)):
        flat = torch.zeros(n * F + 8, dtype=BF, device=DEV)
        Xb = flat[1:1 + n * F].view(n, F)
        Xb.copy_(_rows("randn", n, F, 13))
        assert Xb.data_ptr() % 4 == 2 and Xb.is_contiguous()
        got = _same(hg, Xb, k)
        aligned = hg.ops.knn(Xb.clone(), k, form="dot", return_mean=True)
        assert torch.equal(got[0], aligned[0])
        assert torch.equal(hg.ops.knn(Xb, k, form="dot", return_mean=True)[2], aligned[2])  # the same chunking of every sum


def test_fallback_is_the_host_models_both_ways(hg):
    X = br.to_bf16(np.random.default_rng(1).standard_normal((1000, 64)))
    assert br.certifiable(None, X, 10)
    got = _same(hg, torch.from_numpy(X).to(DEV).to(BF), 10)
    assert not got[2].any()
    I = np.repeat(br.to_bf16(np.random.default_rng(2).standard_normal((1, 64))), 300, axis=0)
    assert br.never_certifiable(None, I, 10)
    got = _same(hg, torch.from_numpy(I).to(DEV).to(BF), 10)
    assert got[2].all()


def test_determinism_and_the_mean(hg):
    Xb = _rows("randn", 1000, 200, 21)
    D64 = br.distances(Xb.float().cpu().numpy(), Xb.float().cpu().numpy())
    E1 = br.bound_bf16(Xb.float().cpu().numpy(), Xb.float().cpu().numpy()).astype(np.float64)
    want = np.sqrt(D64).mean(axis=1)
    base = None
    for cs in (0, 1, 3, 32):
        a = hg.ops.knn(Xb, 10, form="dot", return_mean=True, cand_slices=cs)
        b = hg.ops.knn(Xb, 10, form="dot", return_mean=True, cand_slices=cs)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        if base is None:
            base = a
        assert torch.equal(a[0], base[0]) and torch.equal(a[1], base[1])
        mean = a[2].double().cpu().numpy()
        # n float32 additions of non-negative terms and one division: (n + 1) u relative, on top of mean sqrt(E1b)
        assert (np.abs(mean - want) <= np.sqrt(E1) + (1000 + 1) * 2.0 ** -24 * want).all(), cs


@pytest.mark.parametrize("kind", br.KINDS)
def test_the_hardware_stays_inside_the_bound(hg, kind):
    """hg_knn_dot_estimates_bf16: the prefilter's own tile code on adversarial rows; |est - d2_f64| <= e1 for every pair, and e1
    is bound_bf16's value.  If this fails hypothesis H (include/hg_aggr.h) is false."""
    from hypergef_amd import _lib
    L = _lib.lib()
    n = 128
    for F in (1, 15, 16, 17, 33, 1024, 4096):
        X, Q = br.rows(kind, n, F, 100 + F), br.rows(kind, n, F, 200 + F)
        Xb, Qb = torch.from_numpy(X).to(DEV).to(BF), torch.from_numpy(Q).to(DEV).to(BF)
        est = torch.full((n, n), float("nan"), device=DEV)
        e1 = torch.full((n,), float("nan"), device=DEV)
        with torch.cuda.device(DEV):
            _lib.check(L.hg_knn_dot_estimates_bf16(ctypes.c_void_p(Qb.data_ptr()), n, ctypes.c_void_p(Xb.data_ptr()), n, F,
                                                   ctypes.c_void_p(est.data_ptr()), ctypes.c_void_p(e1.data_ptr()),
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        E1 = br.bound_bf16(Q, X)
        assert np.array_equal(e1.cpu().numpy().view(np.int32), E1.view(np.int32)), (kind, F)
        err = np.abs(est.double().cpu().numpy() - br.distances(Q, X))
        ratio = float((err / E1.astype(np.float64)[:, None]).max())
        print("%s F=%d: max |est - d2| / e1 = %.3g" % (kind, F, ratio))
        assert (err <= E1.astype(np.float64)[:, None]).all(), (kind, F, ratio)


def test_the_raw_entry_stays_inside_its_buffers(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    n, F, k, cs = 300, 65, 10, 3
    Xb = _rows("randn", n, F, 31)
    want = hg.ops.knn(Xb, k, form="dot", return_mean=True, return_fallback=True, cand_slices=cs)
    nbytes = int(L.hg_knn_dot_bf16_workspace_bytes(n, n, F, k, cs))
    bufs = [raw.guarded(n * k, 0x7FC00001, 1), raw.guarded(n * k, 0x7FC00001, 3), raw.guarded(n, 0x7FC00001, 5),
            raw.guarded(n, 0x7FC00001, 7), raw.guarded_bytes(nbytes, 0xFFFFFFFF, 9)]
    (_, idx), (_, dist), (_, mean), (_, fb), (_, ws) = bufs

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    with torch.cuda.device(DEV):
        _lib.check(L.hg_knn_dot_bf16(p(Xb), n, p(Xb), n, F, k, 1, cs, p(idx), p(dist), p(mean), p(fb), p(ws), nbytes,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for buf, view in bufs:
        assert raw.guards_intact(buf, view)
    assert torch.equal(idx.view(n, k), want[0]) and torch.equal(dist.view(torch.float32).view(n, k), want[1])
    assert torch.equal(mean.view(torch.float32), want[2]) and torch.equal(fb, want[3])


def test_the_hypergraphs_take_bfloat16_rows(hg):
    Xb = _rows("randn", 200, 32, 41)
    want = hg.ops.knn(Xb.float(), 5, self_first=True)
    g = hg.KnnHypergraph.build(Xb, 5, form="dot")
    assert g.idx.dtype == torch.int32 and g.dist.dtype == g.mean.dtype == g.degV.dtype == torch.float32
    assert torch.equal(g.idx, want[0]) and torch.equal(g.dist, want[1])
    ref = hg.KnnHypergraph.build(Xb.float(), 5)
    assert torch.equal(g.ptr_v, ref.ptr_v) and torch.equal(g.pos_v, ref.pos_v) and torch.equal(g.degV, ref.degV)
    h = hg.HyperGraph.from_knn(Xb.cpu(), 5, DEV, form="dot")
    assert torch.equal(h.H_T_colind.cpu(), want[0].reshape(-1).cpu().to(h.H_T_colind.dtype)) and torch.equal(h.knn_dist, want[1])


def test_a_captured_build_replays_on_new_rows(hg):
    Xb = _rows("randn", 300, 64, 51)
    hg.KnnHypergraph.build(Xb, 5, form="dot")  # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = hg.KnnHypergraph.build(Xb, 5, form="dot")
    Xb.copy_(_rows("randn", 300, 64, 52))
    graph.replay()
    torch.cuda.synchronize()
    want = hg.ops.knn(Xb.float(), 5, self_first=True)
    assert torch.equal(g.idx, want[0]) and torch.equal(g.dist, want[1])


@pytest.mark.parametrize("probabilistic", [False, True])
def test_the_dynamic_layer_runs_in_bfloat16(hg, probabilistic):
    torch.manual_seed(3)
    Xb = _rows("randn", 200, 32, 61).requires_grad_(True)
    layer = hg.DynamicHypergraphConv(32, 16, 5, probabilistic=probabilistic, knn_form="dot").to(DEV).to(BF)
    Y = layer(Xb)
    assert Y.dtype == BF and tuple(Y.shape) == (200, 16)
    f32 = hg.DynamicHypergraphConv(32, 16, 5, probabilistic=probabilistic).to(DEV)
    f32(Xb.detach().float())
    assert torch.equal(layer.hyperg.H_T_colind, f32.hyperg.H_T_colind) and torch.equal(layer.hyperg.H_T_csrptr, f32.hyperg.H_T_csrptr)
    assert torch.equal(layer.hyperg.knn_dist, f32.hyperg.knn_dist)
    g = layer.hyperg
    Z = layer.lin(Xb.detach())
    Wdiag = torch.ones(g.num_edges, device=DEV)
    if probabilistic:
        w = g.knn_weights(1.0)
        direct = hg.ops.HGNNAggrIncidence(g, Z, w, w, g.degE, g.degV, Wdiag,
                                          options=hg.ops.current_options().replace(incidence_bf16="rows"))
    else:
        direct = hg.HGNNAggr(g, Z, g.degE, g.degV, Wdiag, "sum")
    assert torch.equal(Y.detach().view(torch.int16), direct.view(torch.int16))
    Y.float().sum().backward()
    assert torch.isfinite(layer.lin.weight.grad.float()).all() and torch.isfinite(Xb.grad.float()).all()
    assert layer.lin.weight.grad.float().abs().sum() > 0 and Xb.grad.float().abs().sum() > 0
