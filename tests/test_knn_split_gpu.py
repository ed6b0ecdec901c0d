"""ops.knn(form="dot_split") on the device (include/hg_aggr.h, hg_knn_dot_split_f32): idx and dist are form="difference"'s bit
for bit on the certified path and on the exhaustive one; the matrix unit's sums of the split rows stay inside E1s; the layer
gives knn_form="difference"'s step and is captured by torch.cuda.graph."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_bf16_ref as br  # noqa: E402
import _knn_split_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(X, offset_bytes=0):
    """X on the device; offset_bytes = 4: a contiguous view whose base is 4- but not 16-byte aligned."""
    X = torch.from_numpy(np.ascontiguousarray(X, np.float32))
    flat = torch.zeros(X.numel() + 4, device=DEV)
    view = flat[offset_bytes // 4:offset_bytes // 4 + X.numel()].view(X.shape)
    view.copy_(X)
    assert view.data_ptr() % 16 == offset_bytes
    return view


def _randn(n, F, seed):
    return np.random.default_rng(seed).standard_normal((n, F))


def _same(hg, X, k, **kw):
    got = hg.ops.knn(X, k, form="dot_split", return_fallback=True, **kw)
    want = hg.ops.knn(X, k, form="difference", **kw)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32
    assert torch.equal(got[0], want[0]), (tuple(X.shape), k, kw)
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (tuple(X.shape), k, kw)
    return got


# (n, F, k, nq or None, self_first, cand_slices, base offset in bytes): every F (the tail inside an instruction and inside a chunk,
# F % 4 != 0: element loads), every n (tile edges, partly empty tiles), KS = 1 (k 1, 10), 2 (k 33) and 3 (k 64)
CELLS = [
    (129, 1, 1, None, True, 1, 0), (257, 7, 10, None, False, 3, 0), (300, 16, 33, None, True, 3, 0), (129, 17, 64, None, False, 1, 0),
    (257, 63, 10, 130, None, 3, 0), (300, 64, 33, 129, None, 1, 0), (129, 65, 10, 300, None, 3, 0), (257, 130, 64, None, True, 3, 0),
    (300, 64, 10, None, True, 3, 4), (257, 16, 1, 129, None, 1, 4), (300, 130, 33, None, False, 1, 4), (129, 64, 64, 257, None, 3, 0),
]


@pytest.mark.parametrize("n,F,k,nq,self_first,cs,offset", CELLS)
def test_bits_equal_the_difference_search(hg, n, F, k, nq, self_first, cs, offset):
    X = _dev(_randn(n, F, 11), offset)
    kw = dict(cand_slices=cs)
    if nq is not None:
        kw["queries"] = _dev(_randn(nq, F, 12), offset)
    else:
        kw["self_first"] = self_first
    _same(hg, X, k, **kw)


def test_the_certified_path_is_the_one_tested(hg):
    got = _same(hg, _dev(_randn(2048, 64, 1)), 10)
    assert int(got[2].sum()) == 0


@pytest.mark.parametrize("kind", ["offset", "identical"])
def test_the_exhaustive_path_is_reached_and_exact(hg, kind):
    """randn + 100: the estimates cancel eight digits, no row can be certified.  300 identical rows, more than kp = 32: ties
    at the shortlist's edge."""
    X = _randn(300, 64, 2) + 100.0 if kind == "offset" else np.repeat(_randn(1, 64, 3), 300, axis=0)
    for self_first in (True, False):
        got = _same(hg, _dev(X), 10, self_first=self_first)
        assert bool(got[2].all())


def test_determinism_and_the_mean(hg):
    n = 300
    Xn = np.ascontiguousarray(_randn(n, 130, 21), np.float32)
    E1 = sr.bound_split(Xn, Xn).astype(np.float64)
    want = np.sqrt(br.distances(Xn, Xn)).mean(axis=1)
    X = _dev(Xn)
    for cs in (1, 3):
        a = hg.ops.knn(X, 10, form="dot_split", return_mean=True, return_fallback=True, cand_slices=cs)
        b = hg.ops.knn(X, 10, form="dot_split", return_mean=True, return_fallback=True, cand_slices=cs)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        # n float32 additions of non-negative terms and one division: (n + 1) u relative, on top of mean sqrt(E1s)
        assert (np.abs(a[2].double().cpu().numpy() - want) <= np.sqrt(E1) + (n + 1) * 2.0 ** -24 * want).all(), cs


@pytest.mark.parametrize("kind", sr.KINDS)
def test_the_hardware_stays_inside_the_bound(hg, kind):
    """hg_knn_dot_estimates_split_f32: the prefilter's own tile code on adversarial rows; |est - d2_f64| <= e1 for every pair,
    and e1 is bound_split's value.  If this fails, hypothesis H or the proof of E1s (include/hg_aggr.h) is wrong."""
    from hypergef_amd import _lib
    L = _lib.lib()
    n, worst = 128, 0.0
    for F in sr.WIDTHS:
        Xn, Qn = sr.rows(kind, n, F, 100 + F), sr.rows(kind, n, F, 200 + F)
        X, Q = _dev(Xn), _dev(Qn)
        est = torch.full((n, n), float("nan"), device=DEV)
        e1 = torch.full((n,), float("nan"), device=DEV)
        with torch.cuda.device(DEV):
            _lib.check(L.hg_knn_dot_estimates_split_f32(ctypes.c_void_p(Q.data_ptr()), n, ctypes.c_void_p(X.data_ptr()), n, F,
                                                        ctypes.c_void_p(est.data_ptr()), ctypes.c_void_p(e1.data_ptr()),
                                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        E1 = sr.bound_split(Qn, Xn)
        assert np.array_equal(e1.cpu().numpy().view(np.int32), E1.view(np.int32)), (kind, F)
        err = np.abs(est.double().cpu().numpy() - br.distances(Qn, Xn))
        ratio = float((err / E1.astype(np.float64)[:, None]).max())
        worst = max(worst, ratio)
        print("%s F=%d: max |est - d2| / e1 = %.3g" % (kind, F, ratio))
        assert (err <= E1.astype(np.float64)[:, None]).all(), (kind, F, ratio)
    print("%s: largest ratio %.3g" % (kind, worst))


def test_the_dynamic_layer_steps_as_under_difference_and_is_captured(hg):
    """One training step of the device-only layer: output, gradients and neighbours equal knn_form="difference"'s bit for bit;
    captured once and replayed on new inputs, the neighbours are searched again."""
    n, F, k = 200, 32, 4
    inputs = [_dev(_randn(n, F, 70 + i)) for i in range(3)]
    G = _dev(_randn(n, F, 80))

    def fresh(form):
        torch.manual_seed(5)
        return hg.DynamicHypergraphConv(F, F, k, device_graph=True, knn_form=form).to(DEV)

    def eager(layer, X):
        layer.lin.weight.grad = None
        X = X.clone().requires_grad_(True)
        y = layer(X)
        y.backward(G)
        return y.detach().clone(), layer.lin.weight.grad.detach().clone(), X.grad.clone(), layer.hyperg.idx.clone()

    layer, plain = fresh("dot_split"), fresh("difference")
    want = [eager(layer, X) for X in inputs]
    for got, ref in zip(want, [eager(plain, X) for X in inputs]):
        for u, v in zip(got, ref):
            assert torch.equal(u, v), "knn_form='dot_split' and 'difference' differ in the eager step"
    assert not torch.equal(want[1][3], want[2][3])  # a stale graph could not pass

    static_x = inputs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            layer.lin.weight.grad = None
            layer(static_x).backward(G)
    torch.cuda.current_stream().wait_stream(side)
    layer.lin.weight.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = layer(static_x)
        static_y.backward(G)
    static_idx = layer.hyperg.idx
    for i in (1, 2, 1):
        static_x.copy_(inputs[i])
        graph.replay()
        torch.cuda.synchronize()
        y, gw, _, idx = want[i]
        assert torch.equal(static_idx, idx), "replay with input %d: the neighbours were not searched again" % i
        assert torch.equal(static_y, y) and torch.equal(layer.lin.weight.grad, gw), "replay with input %d" % i
