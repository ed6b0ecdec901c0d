"""bfloat16 rows over a neighbour table on the device (include/hg_aggr.h, hg_table_*_bf16): ops.knn_aggr, ops.knn_dist and the
dynamic layer equal the float32 call on the widened rows bit for bit (a bfloat16 result rounded once), at every lane-group
width of the 16-byte geometry, on long, empty and out-of-range rows, and on the widths that take the widen path."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
N = 150  # no multiple of any rows-per-workgroup: the last workgroup is partial
KS = (1, 9, 64)  # below one batch of gathers, one over a batch, the maximum
WIDTHS = (8, 24, 64, 264, 520, 4, 12, 7)  # L8 = 1, 3, 8, 33, 64 (two column passes); then the widen path
_CACHE = {}


def _table(k):
    """idx [N, k] on the device and its in-degrees: vertex 0 is named 140 times (a long row), 1 exactly HG_TABLE_SEQ_MAX = 128
    times, 2 129 times -- as far as N k positions allow, in that order -- vertex 3 never, and two entries name no vertex."""
    if k not in _CACHE:
        g = torch.Generator().manual_seed(k)
        flat = torch.randint(4, N, (N * k,), generator=g, dtype=torch.int32)
        perm, at, met = torch.randperm(N * k, generator=g), 0, {3: 0}
        for v, count in ((0, 140), (1, 128), (2, 129)):
            if at + count <= N * k - 2:
                flat[perm[at:at + count]] = v
                at, met[v] = at + count, count
        flat[perm[at]], flat[perm[at + 1]] = -1, N
        indeg = torch.bincount(flat[(flat >= 0) & (flat < N)].long(), minlength=N)
        assert all(int(indeg[v]) == c for v, c in met.items()) and (len(met) == 4 or k == 1)
        _CACHE[k] = flat.view(N, k).to(DEV), indeg.to(DEV)
    return _CACHE[k]


def _rows(n, F, seed):
    return torch.randn(n, F, generator=torch.Generator().manual_seed(seed)).to(BF).to(DEV)


def _scale(n, seed):
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) + 0.5).to(DEV)


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32), b.view(torch.int16 if b.dtype == BF else torch.int32))


def _aggr64(idx, X, w, degE, degV):
    """Y = degV . H_w (degE . (H_w^T X)) in float64 by index_add_, entries out of range dropped."""
    k = idx.shape[1]
    flat = idx.reshape(-1).long()
    ok = (flat >= 0) & (flat < N)
    e, v, w = torch.arange(N * k, device=DEV)[ok] // k, flat[ok], w.double()[ok][:, None]
    Xe = degE.double()[:, None] * torch.zeros(N, X.shape[1], dtype=torch.float64, device=DEV).index_add_(0, e, X.double()[v] * w)
    return degV.double()[:, None] * torch.zeros_like(Xe).index_add_(0, v, Xe[e] * w)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("k", KS)
def test_aggr_is_the_float32_call_rounded_once(hg, k, F, weighted):
    idx, indeg = _table(k)
    rows = hg.ops.current_options().replace(incidence_bf16="rows")
    Xb, dY = _rows(N, F, 1), _rows(N, F, 2)
    w = _scale(N * k, 3) if weighted else None
    degE, degV = _scale(N, 4), _scale(N, 5)
    got, want = [], []
    for X, d, out, opt in ((Xb, dY, got, rows), (Xb.float(), dY.float(), want, None)):
        X = X.clone().requires_grad_(True)
        wt = w.clone().requires_grad_(True) if weighted else None
        Y = hg.ops.knn_aggr(idx, X, wt, degE, degV, weight_grad=weighted, options=opt)
        Y.backward(d)
        out += [Y.detach(), X.grad] + ([wt.grad] if weighted else [])
    assert got[0].dtype == got[1].dtype == BF
    assert _same_bits(got[0], want[0].to(BF)) and _same_bits(got[1], want[1].to(BF))
    if weighted:  # dw: float32, from hg_table_dot_bf16
        assert _same_bits(got[2], want[2])
    ones = torch.ones(N * k, device=DEV)
    Y64 = _aggr64(idx, Xb, ones if w is None else w, degE, degV)
    M = _aggr64(idx, Xb.abs(), ones if w is None else w, degE, degV)
    bound = 2.0 ** -8 * Y64.abs() + (k + indeg.double()[:, None] + 8) * 2.0 ** -23 * M
    assert ((got[0].double() - Y64).abs() <= bound).all()
    assert not got[0][3].any() and not torch.signbit(got[0][3].float()).any()  # the vertex no hyperedge names: +0.0


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("k", KS)
def test_dist_and_its_gradients(hg, k, F):
    idx, _ = _table(k)
    rows = hg.ops.current_options().replace(incidence_bf16="rows")
    Xb, Qb = _rows(N, F, 6), _rows(N, F, 7)
    dD = torch.randn(N, k, generator=torch.Generator().manual_seed(8)).to(DEV)
    for queries in (None, Qb):
        got, want = [], []
        for wide, out, opt in ((False, got, rows), (True, want, None)):
            X = (Xb.float() if wide else Xb).clone().requires_grad_(True)
            Q = None if queries is None else (queries.float() if wide else queries).clone().requires_grad_(True)
            dist = hg.ops.knn_dist(idx, X, queries=Q, options=opt)
            dist.backward(dD)
            out += [dist.detach(), X.grad] + ([] if Q is None else [Q.grad])
        assert got[0].dtype == torch.float32 and _same_bits(got[0], want[0])
        for a, b in zip(got[1:], want[1:]):
            assert a.dtype == BF and _same_bits(a, b.to(BF))


def test_dist_of_a_searched_table_is_the_search_s_dist(hg):
    Xb = _rows(300, 64, 9)
    idx, dist = hg.ops.knn(Xb, 5, form="dot")
    assert _same_bits(hg.ops.knn_dist(idx, Xb, options=hg.ops.current_options().replace(incidence_bf16="rows")), dist)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dst_bf16", [False, True])
@pytest.mark.parametrize("F", [24, 264])
def test_raw_gather_entries_write_every_row_and_nothing_else(hg, F, dst_bf16, transposed):
    from hypergef_amd import _lib
    k = 9
    idx, _ = _table(k)
    ptr_v, pos_v = hg.ops.knn_transpose(idx, N)
    src = _rows(N, F, 10)
    src = src.float() if dst_bf16 else src
    guard = 64  # elements of NaN in front of and behind dst; dst stays 16-byte aligned
    buf = torch.full((N * F + 2 * guard,), float("nan"), dtype=BF if dst_bf16 else torch.float32, device=DEV)
    dst = buf[guard:guard + N * F]
    io = _lib.HG_ROWS_DST_BF16 if dst_bf16 else _lib.HG_ROWS_SRC_BF16
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    head = (p(ptr_v), p(pos_v)) if transposed else (p(idx),)
    entry = _lib.lib().hg_table_gather_t_bf16 if transposed else _lib.lib().hg_table_gather_bf16
    _lib.check(entry(*head, N, k, N, F, p(src), None, None, None, None, p(dst), io, None))
    torch.cuda.synchronize()
    assert not torch.isnan(dst).any()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + N * F:]).all()
    gather = hg.knn_graph.table_gather_t if transposed else hg.knn_graph.table_gather
    want = gather(*((ptr_v, pos_v, k) if transposed else (idx,)), src.float())
    assert _same_bits(dst.view(N, F), want.to(dst.dtype))


def _layer(hg, dtype, **kw):
    torch.manual_seed(3)
    return hg.DynamicHypergraphConv(32, 16, 5, device_graph=True, knn_form="dot", **kw).to(DEV).to(dtype)


@pytest.mark.parametrize("kw", [dict(probabilistic=False), dict(probabilistic=True),
                                dict(probabilistic=True, learn_distances=True)], ids=["plain", "probabilistic", "learn"])
def test_the_device_graph_layer_runs_in_bfloat16(hg, kw):
    Xb = _rows(200, 32, 11).requires_grad_(True)
    layer = _layer(hg, BF, **kw)
    Y = layer(Xb)
    assert Y.dtype == BF and tuple(Y.shape) == (200, 16)
    rows = hg.ops.current_options().replace(incidence_bf16="rows")
    Z = layer.lin(Xb.detach())
    prob = kw["probabilistic"]
    direct = hg.KnnHypergraph.build(Xb, 5, form="dot").aggregate(Z, probabilistic=prob, options=rows)
    assert _same_bits(Y.detach(), direct)
    f32 = _layer(hg, torch.float32, **kw)
    f32(Xb.detach().float())
    assert torch.equal(f32.hyperg.idx, layer.hyperg.idx) and _same_bits(f32.hyperg.dist, layer.hyperg.dist)
    f32.hyperg.mean = layer.hyperg.mean  # under "dot" the mean is each search's own estimate (ops.knn): the weights' constant
    assert _same_bits(Y.detach(), f32.hyperg.aggregate(Z.float(), probabilistic=prob).to(BF))
    Y.float().sum().backward()
    for g in (layer.lin.weight.grad, Xb.grad):
        assert torch.isfinite(g.float()).all() and g.float().abs().sum() > 0


def test_the_captured_layer_replays_on_new_rows(hg):
    Xb = _rows(200, 32, 12)
    layer = _layer(hg, BF, probabilistic=True)
    with torch.no_grad():
        layer(Xb)  # warm up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            Y = layer(Xb)
        first = layer.hyperg.idx.clone()
        Xb.copy_(_rows(200, 32, 13))
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        replayed, table = Y.clone(), layer.hyperg.idx.clone()
        assert _same_bits(replayed, layer(Xb)) and not torch.equal(table, first)
