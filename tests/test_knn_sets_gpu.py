"""ops.knn(set_rows=m) on the device: idx and dist are the segments + "difference" call's bit for bit under every form, the
certificate is per set, and a layer with set_rows is recorded by torch.cuda.graph."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_bf16_ref as br  # noqa: E402
import _knn_dot_ref as dr  # noqa: E402
import _knn_ref as kr  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U23 = 2.0 ** -23
FORMS = {"difference": ("difference", torch.float32), "dot": ("dot", torch.float32), "dot_bf16": ("dot", torch.bfloat16)}
# (B, m, F, k): m == k (the shortlist is the set); m just above kp = 32, odd F; one tile; a second, one-row tile, kp = 64;
# kp = 96, three tiles; B = 1
SHAPES = [(3, 10, 7, 10), (5, 33, 17, 10), (2, 128, 64, 16), (3, 129, 65, 33), (2, 300, 8, 64), (1, 200, 32, 5)]


@functools.lru_cache(maxsize=None)
def _rows(shape, kind, bf16):
    """The rows as float32 on the host (bf16: rounded to bfloat16 first; the integers are exact either way)."""
    B, m, F, _ = shape
    rng = np.random.default_rng(1000 * m + F)
    X = rng.integers(-4, 5, (B * m, F)).astype(np.float32) if kind == "integer" else rng.standard_normal((B * m, F)).astype(np.float32)
    return torch.from_numpy(X).to(torch.bfloat16).float().numpy() if bf16 else X


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, bf16, self_first):
    B, m, _, k = shape
    return kr.knn(_rows(shape, kind, bf16), k, segments=np.arange(0, B * m + 1, m), self_first=self_first)


@pytest.mark.parametrize("cs", [0, 3])
@pytest.mark.parametrize("self_first", [True, False])
@pytest.mark.parametrize("kind", ["integer", "randn"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", list(FORMS))
def test_bit_identity(hg, form, shape, kind, self_first, cs):
    B, m, F, k = shape
    form_kw, dtype = FORMS[form]
    bf16 = dtype == torch.bfloat16
    X = _rows(shape, kind, bf16)
    wide = torch.from_numpy(X).to(DEV)
    x = wide.to(dtype)  # exact: bf16 rows are already rounded
    ref_idx, ref_dist, ref_mean = _reference(shape, kind, bf16, self_first)
    kw = dict(self_first=self_first, cand_slices=cs, return_mean=True)
    idx, dist, mean = hg.ops.knn(x, k, set_rows=m, form=form_kw, **kw)
    want = hg.ops.knn(wide, k, segments=list(range(0, B * m + 1, m)), form="difference", **kw)
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and torch.equal(idx, want[0])
    assert torch.equal(dist.view(torch.int32), want[1].view(torch.int32))
    d = dist.double().cpu().numpy()
    if kind == "integer":  # exact in float32 and float64: (d2, j) is one order in both
        assert np.array_equal(idx.cpu().numpy(), ref_idx) and np.array_equal(d, ref_dist)
    else:  # float32 may order a near tie of float64 the other way; the s-th smallest distance moves by no more than a
        # distance does: F subtractions and F fmas in float32, (F + 2) 2^-24 relative
        assert (np.abs(d - ref_dist) <= (F + 2) * 2.0 ** -24 * ref_dist).all()
    if form == "difference":
        assert torch.equal(mean.view(torch.int32), want[2].view(torch.int32))
    else:  # per set, test_knn_dot_gpu.py's bound with n = m: sqrt(E1) a term, m + 2 float32 roundings
        bound = br.bound_bf16 if bf16 else dr.bound
        E1 = np.concatenate([bound(X[b * m:(b + 1) * m], X[b * m:(b + 1) * m]) for b in range(B)]).astype(np.float64)
        tol = np.sqrt(E1) + (m + 2) * U23 * (ref_mean + np.sqrt(E1)) + 2.0 ** -63
        err = np.abs(mean.double().cpu().numpy() - ref_mean)
        print("max |mean - mean_f64| / bound = %.3g" % float((err / tol).max()))
        assert (err <= tol).all()
    again = hg.ops.knn(x, k, set_rows=m, form=form_kw, **kw)
    assert all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(again, (idx, dist, mean))), "two calls differ"
    if B == 1:
        for u, v in zip(hg.ops.knn(x, k, form=form_kw, **kw), (idx, dist, mean)):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "differs from the call without set_rows"


@pytest.mark.parametrize("form", ["dot", "dot_bf16"])
def test_certificate_uses_the_sets_own_norm_maximum(hg, form):
    """Set 1 lies 1e4 from the origin: E1 under its norms is about 1e5, far above every distance of the near sets."""
    B, m, F, k = 3, 96, 64, 10
    dtype = FORMS[form][1]
    X = np.random.default_rng(5).integers(-4, 5, (B * m, F)).astype(np.float32)
    X[m:2 * m] += np.float32(1e4)
    x = torch.from_numpy(X).to(DEV).to(dtype)
    X = x.float().cpu().numpy()  # bfloat16 rounds the shifted set; the near sets stay exact
    idx, dist, fb = hg.ops.knn(x, k, set_rows=m, form="dot", return_fallback=True)
    ref = kr.knn(X, k, segments=np.arange(0, B * m + 1, m))
    assert np.array_equal(idx.cpu().numpy(), ref[0]) and np.array_equal(dist.double().cpu().numpy(), ref[1])
    for b in range(B):
        alone = hg.ops.knn(x[b * m:(b + 1) * m].contiguous(), k, form="dot", return_fallback=True)[2]
        assert torch.equal(fb[b * m:(b + 1) * m], alone), "set %d" % b
    assert not fb[:m].any() and not fb[2 * m:].any()


@pytest.mark.parametrize("dtype,form", [(torch.float32, "difference"), (torch.bfloat16, "dot")], ids=["f32-difference", "bf16-dot"])
def test_layer_with_set_rows_is_captured_and_replayed(hg, dtype, form):
    """One training step on a 4 x 64 batch, recorded once and replayed on new input; it equals the eager step."""
    B, m, F, k = 4, 64, 16, 8
    rng = np.random.default_rng(3)
    inputs = [torch.from_numpy(rng.standard_normal((B * m, F)).astype(np.float32)).to(DEV).to(dtype) for _ in range(3)]
    G = torch.from_numpy(rng.standard_normal((B * m, F)).astype(np.float32)).to(DEV).to(dtype)
    torch.manual_seed(5)
    layer = hg.DynamicHypergraphConv(F, F, k, device_graph=True, set_rows=m, knn_form=form).to(DEV).to(dtype)

    def eager(X):
        layer.lin.weight.grad = None
        y = layer(X)
        y.backward(G)
        return y.detach().clone(), layer.lin.weight.grad.detach().clone(), layer.hyperg.idx.clone()

    want = [eager(X) for X in inputs]
    assert not torch.equal(want[1][2], want[2][2])  # a stale graph could not pass
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
    for i in (1, 2):
        static_x.copy_(inputs[i])
        graph.replay()
        torch.cuda.synchronize()
        y, gw, idx = want[i]
        assert torch.equal(static_idx, idx), "replay with input %d: the neighbours were not searched again" % i
        assert torch.equal(static_idx // m, (torch.arange(B * m, device=DEV) // m)[:, None].expand(-1, k)), "a neighbour outside its set"
        assert torch.equal(static_y, y) and torch.equal(layer.lin.weight.grad, gw), "replay with input %d" % i
