"""Aggregation over a neighbour table on the device (-m gpu): hg_table_transpose against the stable argsort, the two gathers
bit for bit against float32 loops in the contract's order -- rows one lane group sums, and rows a whole workgroup sums in
the pieces and the tree of the header's ORDER paragraph (tests/_table_ref.py, gather_t_ordered), at every width where that
path changes shape, wherever the row stands, with ignored positions in it -- and against float64,
ops.knn_aggr and its gradient against float64 and against the planned operators on
HyperGraph.from_knn, DynamicHypergraphConv(device_graph=True) against the layer as it was, and its hipGraph capture."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _table_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _assert_close(y, ref, what=""):
    """Class (b) of tests/test_gpu_parity.py: a deterministic kernel whose order may differ from the reference's."""
    y = _np(y) if hasattr(y, "detach") else y
    ref = np.asarray(ref)
    bad = ~(np.abs(y - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref)))
    assert not bad.any(), "%s: 1e-5 max(1, |ref|): %d off, worst %g" % (what, bad.sum(), np.abs(y - ref).max())
    bad = ~np.isclose(y, ref, rtol=1e-4, atol=1e-6)
    assert not bad.any(), "%s: allclose(1e-4, 1e-6): %d off, worst %g" % (what, bad.sum(), np.abs(y - ref).max())


def _check_transpose(hg, idx, n):
    ptr, pos = hg.ops.knn_transpose(_dev(idx), n)
    want_ptr, want_pos = tr.transpose(idx, n)
    assert ptr.dtype == torch.int32 and pos.dtype == torch.int32
    assert tuple(ptr.shape) == (n + 1,) and tuple(pos.shape) == (idx.size,)
    assert np.array_equal(_np(ptr), want_ptr), (idx.shape, n)
    assert np.array_equal(_np(pos)[:want_pos.shape[0]], want_pos), (idx.shape, n)


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 300])
def test_transpose_of_knn_tables(hg, rows):
    rng = np.random.default_rng(rows)
    X = _dev(rng.integers(-1, 2, (rows, 3)).astype(np.float32))  # integer-valued: ties everywhere
    for k in (1, 2, 10, 64):
        if k > rows:
            continue
        idx, _ = hg.ops.knn(X, k)
        _check_transpose(hg, _np(idx), rows)


def test_transpose_of_hand_made_tables(hg):
    rng = np.random.default_rng(0)
    _check_transpose(hg, np.array([[0, 2, 2], [1, 0, 3], [2, 0, 1], [3, 1, 2]], np.int32), 4)  # a duplicate within a row
    idx = rng.integers(-1, 8, (40, 5)).astype(np.int32)  # -1 and n = 7 are ignored
    assert (idx == -1).any() and (idx == 7).any()
    _check_transpose(hg, idx, 7)
    _check_transpose(hg, rng.integers(0, 1000, (30, 4)).astype(np.int32), 1000)  # n != rows, most vertices unnamed
    _check_transpose(hg, rng.integers(0, 5, (300, 10)).astype(np.int32), 5)
    idx = rng.integers(0, 9, (50, 3)).astype(np.int32)
    idx[idx == 4] = 5  # a vertex no row names
    _check_transpose(hg, idx, 9)
    idx = rng.integers(1, 1500, (1500, 2)).astype(np.int32)
    idx[:, 0] = 0  # every row names vertex 0
    _check_transpose(hg, idx, 1500)
    _check_transpose(hg, rng.integers(0, 70000, (3000, 7)).astype(np.int32), 70000)  # keys of 17 bits: three passes, many tiles


def test_transpose_where_the_scan_carries_and_the_key_widens(hg):
    rng = np.random.default_rng(1)
    # 19 tiles of 2048 entries: 4864 counters, more than the 4096 one trip of the scan takes, so the second trip starts from
    # the first one's carry; -1 and n = 999 are ignored and sort behind every vertex
    idx = rng.integers(-1, 1000, (600, 64)).astype(np.int32)
    assert (idx == -1).any() and (idx == 999).any()
    _check_transpose(hg, idx, 999)
    # exactly one tile, and one tile and one entry
    _check_transpose(hg, rng.integers(0, 50, (32, 64)).astype(np.int32), 50)
    _check_transpose(hg, rng.integers(0, 50, (2049, 1)).astype(np.int32), 50)
    # the key of an ignored entry is n itself: 8 bits at n = 255 and 9 at 256 (one radix pass, then two), 16 and 17 (three)
    for n in (255, 256, 65535, 65536):
        idx = rng.integers(-1, n + 1, (40, 5)).astype(np.int32)
        idx[0, :2], idx[39, 3:] = (-1, n), (n, -1)
        idx[1, 0], idx[38, 4] = 0, n - 1
        assert (idx == -1).any() and (idx == n).any()
        _check_transpose(hg, idx, n)


@pytest.fixture(scope="module")
def short_table():
    """A table whose every vertex row has at most HG_TABLE_SEQ_MAX entries, with an empty row, a duplicate and ignored entries."""
    rng = np.random.default_rng(21)
    rows, k, n = 150, 7, 90
    idx = rng.integers(0, n, (rows, k)).astype(np.int32)
    idx[idx == 11] = 12       # vertex 11 is empty
    idx[3, 1] = idx[3, 0]     # a duplicate
    idx[5, 2], idx[6, 0] = -1, n
    ptr, pos = tr.transpose(idx, n)
    w = rng.random(rows * k).astype(np.float32) + 0.5
    return dict(rows=rows, k=k, n=n, idx=idx, ptr=ptr, pos=pos, w=w, rng_seed=22)


@pytest.mark.parametrize("F", [1, 3, 4, 32, 33, 128, 260])
def test_gathers_bit_exact(hg, short_table, F):
    from hypergef_amd import knn_graph as kg
    t = short_table
    rows, k, n, idx = t["rows"], t["k"], t["n"], t["idx"]
    assert np.diff(t["ptr"]).max() <= kg.table_seq_max() and np.diff(t["ptr"])[11] == 0
    rng = np.random.default_rng(t["rng_seed"] + F)
    Xv = rng.standard_normal((n, F)).astype(np.float32)
    Xe = rng.standard_normal((rows, F)).astype(np.float32)
    sv, se = rng.standard_normal(n).astype(np.float32), rng.standard_normal(rows).astype(np.float32)
    ptr_d, pos_d = hg.ops.knn_transpose(_dev(idx), n)
    for use_w, use_src, use_dst in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        w = t["w"] if use_w else None
        got = kg.table_gather(_dev(idx), _dev(Xv), _dev(w), _dev(sv if use_src else None), _dev(se if use_dst else None))
        want = tr.gather(idx, Xv, w, sv if use_src else None, se if use_dst else None)
        assert np.array_equal(_np(got), want), ("gather", F, use_w, use_src, use_dst)
        got = kg.table_gather_t(ptr_d, pos_d, k, _dev(Xe), _dev(w), _dev(se if use_src else None), _dev(sv if use_dst else None))
        want = tr.gather_t(t["ptr"], t["pos"], k, Xe, w, se if use_src else None, sv if use_dst else None)
        assert np.array_equal(_np(got), want), ("gather_t", F, use_w, use_src, use_dst)
    scale = np.ones(n, np.float32)
    scale[11] = np.inf  # an empty row is +0.0 under a scale of inf
    got = _np(kg.table_gather_t(ptr_d, pos_d, k, _dev(Xe), None, None, _dev(scale)))
    assert not got[11].any() and not np.signbit(got[11]).any()
    assert np.array_equal(got, tr.gather_t(t["ptr"], t["pos"], k, Xe, None, None, scale))


def _hub_table(length, extra_rows=0, k=2, seed=31):
    """`length` rows that name vertex 0 in slot 0, then `extra_rows` that do not; the other slots name vertices >= 1."""
    rng = np.random.default_rng(seed)
    rows = length + extra_rows
    idx = rng.integers(1, 40, (rows, k)).astype(np.int32)
    idx[:length, 0] = 0
    return idx


@pytest.mark.parametrize("F", [32, 33])
def test_long_rows(hg, F):
    from hypergef_amd import knn_graph as kg
    seq = kg.table_seq_max()
    big = max(1500, 8 * seq + 60)
    k = 2
    for length in (big, seq + 1, 4 * seq + 3):  # the last: no multiple of the four waves
        idx = _hub_table(length)
        rows, n = idx.shape[0], idx.shape[0]
        rng = np.random.default_rng(40 + F)
        src = rng.standard_normal((rows, F)).astype(np.float32)
        w = (rng.random(rows * k) + 0.5).astype(np.float32)
        ptr, pos = tr.transpose(idx, n)
        assert ptr[1] == length > seq
        deg = np.diff(ptr).astype(np.float64)
        degV = np.where(deg > 0, np.maximum(deg, 1) ** -0.5, 1.0).astype(np.float32)  # the operator's vertex scale
        ptr_d, pos_d = hg.ops.knn_transpose(_dev(idx), n)
        got = kg.table_gather_t(ptr_d, pos_d, k, _dev(src), _dev(w), None, _dev(degV))
        ref = np.zeros((n, F))
        for v in range(n):
            p = pos[ptr[v]:ptr[v + 1]]
            ref[v] = degV[v].astype(np.float64) * (src[p // k].astype(np.float64) * w[p].astype(np.float64)[:, None]).sum(0)
        _assert_close(got, ref, "gather_t, hub of %d, F = %d" % (length, F))
        again = kg.table_gather_t(ptr_d, pos_d, k, _dev(src), _dev(w), None, _dev(degV))
        assert torch.equal(got, again)
        plain = kg.table_gather_t(ptr_d, pos_d, k, _dev(src))
        assert torch.equal(plain, kg.table_gather_t(ptr_d, pos_d, k, _dev(src)))
        _assert_close(plain[0] * float(degV[0]), degV[0].astype(np.float64) * src[:length].astype(np.float64).sum(0),
                      "unweighted hub of %d, F = %d" % (length, F))
        if length == big:
            # the same positions in a table padded with 700 rows that do not name vertex 0: the hub's bits do not move
            idx2 = _hub_table(length, extra_rows=700)
            assert np.array_equal(idx2[:length, 0], idx[:, 0]) and not (idx2[length:] == 0).any()
            src2 = np.concatenate([src, rng.standard_normal((700, F)).astype(np.float32)])
            ptr2, pos2 = hg.ops.knn_transpose(_dev(idx2), idx2.shape[0])
            padded = kg.table_gather_t(ptr2, pos2, k, _dev(src2))
            assert torch.equal(padded[0], plain[0])
            assert np.array_equal(_np(pos2)[:length], _np(pos_d)[:length])


def _dev_rows(a, aligned16=True):
    """A [rows, F] array on the device, on a 16-byte boundary or one float past one."""
    if aligned16:
        t = _dev(a)
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.zeros(a.size + 1, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[1:].view(*a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


FACTORS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))  # which of w, src_scale, dst_scale a call is given


@pytest.mark.parametrize("F,aligned,P", tr.LONG_ROW_WIDTHS)
def test_long_rows_bit_exact_wherever_they_stand(hg, F, aligned, P):
    """Vertex rows above HG_TABLE_SEQ_MAX in the header's order, bit for bit: in another lane group, another wave and another
    workgroup than the first, two in one tile, the last vertex of a partial tile, beside short rows, a row of exactly
    HG_TABLE_SEQ_MAX entries and an empty one -- and the same entries under another vertex number give the same bits."""
    from hypergef_amd import knn_graph as kg
    seq = kg.table_seq_max()
    c, L, R, got_P, P2 = tr.long_row_shape(F, aligned)
    assert got_P == P, "the header's P = 4 * (64 / L) at F = %d is %d, the table of widths says %d" % (F, got_P, P)
    t = tr.hub_table(F, aligned, seq, seed=F)
    idx, n, hubs, k = t["idx"], t["n"], t["hubs"], 2
    rows = idx.shape[0]
    ptr, pos = tr.transpose(idx, n)
    lens = np.diff(ptr)
    assert n % (4 * R) and set(hubs) == {0, 1, R, 4 * R - 1, 4 * R, n - 1} and (lens[hubs] > seq).all()
    assert {seq + 1, seq + 2, 4 * seq + 3} <= set(lens[hubs].tolist()) and lens[hubs].max() >= 1000
    assert lens[t["full"]] == seq and lens[t["empty"]] == 0 and (np.delete(lens, hubs) <= seq).all()
    rng = np.random.default_rng(300 + F)
    src = rng.standard_normal((rows, F)).astype(np.float32)
    w = (rng.random(rows * k) + 0.5).astype(np.float32)
    ss, ds = rng.standard_normal(rows).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    # the second table: vertex v is called perm[v]; the positions and the source rows stay, every row moves
    perm = (np.arange(n) + 2 * R + 1) % n
    assert (perm[hubs] != hubs).all()
    inv = np.argsort(perm)
    ptr_d, pos_d = hg.ops.knn_transpose(_dev(idx), n)
    ptr2_d, pos2_d = hg.ops.knn_transpose(_dev(perm[idx].astype(np.int32)), n)
    assert np.array_equal(_np(ptr_d), ptr) and np.array_equal(_np(pos_d), pos)
    ptr2, pos2 = _np(ptr2_d), _np(pos2_d)
    for h in hubs:
        assert np.array_equal(pos2[ptr2[perm[h]]:ptr2[perm[h] + 1]], pos[ptr[h]:ptr[h + 1]])
    src_d = _dev_rows(src, aligned)
    for use_w, use_src, use_dst in FACTORS:
        what = "F = %d, w %d, src_scale %d, dst_scale %d" % (F, use_w, use_src, use_dst)
        a = (w if use_w else None, ss if use_src else None, ds if use_dst else None)
        got = kg.table_gather_t(ptr_d, pos_d, k, src_d, *[_dev(x) for x in a])
        assert got.data_ptr() % 16 == 0
        want = tr.gather_t_ordered(ptr, pos, k, src, *a, aligned16=aligned, seq_max=seq)
        bad = np.flatnonzero((_np(got) != want).any(1))
        assert np.array_equal(_np(got), want), "%s: rows %s differ (hubs %s)" % (what, bad.tolist(), hubs)
        assert not _np(got)[t["empty"]].any() and not np.signbit(_np(got)[t["empty"]]).any(), what
        again = kg.table_gather_t(ptr_d, pos_d, k, src_d, *[_dev(x) for x in a])
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)), what + ": two calls differ"
        a2 = (a[0], a[1], None if a[2] is None else a[2][inv])
        moved = kg.table_gather_t(ptr2_d, pos2_d, k, src_d, *[_dev(x) for x in a2])
        for h in hubs:
            assert torch.equal(moved[perm[h]], got[h]), "%s: hub %d as vertex %d has other bits" % (what, h, perm[h])
        assert torch.equal(moved[_dev(perm)], got), what + ": a short row moved with its place"


@pytest.mark.parametrize("F", [3, 32])
def test_ignored_positions_of_a_hand_made_transpose(hg, F):
    """pos_v entries outside 0 .. rows k - 1 in a short row and in the first, a middle and the last piece of a long one: each
    keeps its place in the row's length and pieces, adds nothing and is not read through."""
    from hypergef_amd import knn_graph as kg
    seq = kg.table_seq_max()
    t = tr.hub_table(F, True, seq, seed=50 + F)
    idx, n, k = t["idx"], t["n"], 2
    rows = idx.shape[0]
    ptr, pos = tr.transpose(idx, n)
    pos = pos.copy()
    assert pos.shape[0] == rows * k
    outside = (-1, rows * k, 2 ** 31 - 1)
    lens = np.diff(ptr)
    hub = t["hubs"][int(np.argmax(lens[t["hubs"]]))]
    length, P = int(lens[hub]), t["P"]
    chunk = -(-length // P)
    last = (length - 1) // chunk  # the last piece that holds an entry
    assert last > P // 2 > 0 and length > seq
    for g, bad in zip((0, P // 2, last), outside):
        pos[ptr[hub] + g * chunk + (min(chunk, length - g * chunk) - 1) * (g % 2)] = bad  # a piece's first or last entry
    pos[ptr[hub] + 1] = outside[1]
    short = next(v for v in range(n) if v not in t["hubs"] and 4 <= lens[v] < seq)
    pos[ptr[short]:ptr[short] + 3] = outside
    lonely = next(v for v in range(n) if v not in t["hubs"] and v != short and 1 <= lens[v] < seq)
    pos[ptr[lonely]:ptr[lonely + 1]] = -1  # a row of ignored entries only: not empty, +0.0 times its scale
    rng = np.random.default_rng(400 + F)
    src = rng.standard_normal((rows, F)).astype(np.float32)
    w = (rng.random(rows * k) + 0.5).astype(np.float32)
    ss, ds = rng.standard_normal(rows).astype(np.float32), np.abs(rng.standard_normal(n)).astype(np.float32) + 0.5
    ptr_d, pos_d, src_d = _dev(ptr), _dev(pos), _dev(src)
    for use_w, use_src, use_dst in FACTORS:
        a = (w if use_w else None, ss if use_src else None, ds if use_dst else None)
        got = _np(kg.table_gather_t(ptr_d, pos_d, k, src_d, *[_dev(x) for x in a]))
        want = tr.gather_t_ordered(ptr, pos, k, src, *a, seq_max=seq)
        assert np.array_equal(got, want), (F, use_w, use_src, use_dst, np.flatnonzero((got != want).any(1)).tolist())
        assert not got[lonely].any() and not np.signbit(got[lonely]).any()


@pytest.mark.parametrize("F", [5, 32])
def test_operator_and_gradient_over_hubs(hg, F):
    """ops.knn_aggr over a table with long vertex rows: both the forward's and the backward's table_gather_t take the long
    path.  Against float64 at the file's tolerance, and the forward bit for bit against the two launches in float32."""
    from hypergef_amd import knn_graph as kg
    t = tr.hub_operator_case(F, kg.table_seq_max())
    idx, n, w, degE, degV = t["idx"], t["n"], t["w"], t["degE"], t["degV"]
    X = _dev(t["X"]).requires_grad_(True)
    Y = hg.ops.knn_aggr(_dev(idx), X, _dev(w), _dev(degE), _dev(degV))
    (dX,) = torch.autograd.grad(Y, X, _dev(t["G"]))
    _assert_close(Y, tr.aggr(idx, t["X"], w, degE, degV), "Y over hubs, F = %d" % F)
    _assert_close(dX, tr.aggr_grad(idx, t["G"], w, degE, degV), "dX over hubs, F = %d" % F)
    ptr, pos = tr.transpose(idx, n)
    want = tr.gather_t_ordered(ptr, pos, 2, tr.gather(idx, t["X"], w, None, degE), w, None, degV, seq_max=kg.table_seq_max())
    assert np.array_equal(_np(Y), want)
    want = tr.gather_t_ordered(ptr, pos, 2, tr.gather(idx, t["G"], w, degV, degE), w, seq_max=kg.table_seq_max())
    assert np.array_equal(_np(dX), want)


@pytest.fixture(scope="module")
def knn_case(hg):
    """ops.knn's table of 300 randn points, k = 10, with its mean distances, and the planned hypergraph of the same points."""
    torch.manual_seed(5)
    P = torch.randn(300, 6, device=DEV)
    idx, dist, mean = hg.ops.knn(P, 10, self_first=True, return_mean=True)
    hyperg = hg.HyperGraph.from_knn(P, 10, DEV)
    assert torch.equal(hyperg.H_T_colind.reshape(300, 10), idx)
    return dict(P=P, idx=idx, w=hg.ops.knn_incidence_weights(dist, mean), hyperg=hyperg)


@pytest.mark.parametrize("F", [32, 33])
@pytest.mark.parametrize("weighted", [False, True])
def test_operator_and_gradient(hg, knn_case, F, weighted):
    c = knn_case
    idx, hyperg = c["idx"], c["hyperg"]
    w = c["w"] if weighted else None
    rng = np.random.default_rng(60 + F)
    Xn = rng.standard_normal((300, F)).astype(np.float32)
    Gn = rng.standard_normal((300, F)).astype(np.float32)
    X = _dev(Xn).requires_grad_(True)
    Y = hg.ops.knn_aggr(idx, X, w, hyperg.degE, hyperg.degV)
    (dX,) = torch.autograd.grad(Y, X, _dev(Gn))
    wn = None if w is None else _np(w)
    degE, degV = _np(hyperg.degE), _np(hyperg.degV)
    _assert_close(Y, tr.aggr(_np(idx), Xn, wn, degE, degV), "Y")
    _assert_close(dX, tr.aggr_grad(_np(idx), Gn, wn, degE, degV), "dX")
    # the planned operators on HyperGraph.from_knn of the same points (adjoint backward: the true gradient)
    X2 = _dev(Xn).requires_grad_(True)
    ones = torch.ones(300, device=DEV)
    with hg.ops.options(backward="adjoint"):
        if weighted:
            Y2 = hg.ops.HGNNAggrIncidence(hyperg, X2, w, w, hyperg.degE, hyperg.degV, ones)
        else:
            Y2 = hg.HGNNAggr(hyperg, X2, hyperg.degE, hyperg.degV, ones, "sum")
        (dX2,) = torch.autograd.grad(Y2, X2, _dev(Gn))
    _assert_close(Y, _np(Y2).astype(np.float64), "Y against the planned operator")
    _assert_close(dX, _np(dX2).astype(np.float64), "dX against the planned operator")
    # a transpose handed in gives the same bits as the one computed; nothing of rows * F elements is saved
    tp = hg.ops.knn_transpose(idx)
    X3 = _dev(Xn).requires_grad_(True)
    Y3 = hg.ops.knn_aggr(idx, X3, w, hyperg.degE, hyperg.degV, transpose=tp)
    assert all(t is None or t.numel() <= 300 * 10 for t in Y3.grad_fn.saved_tensors)
    (dX3,) = torch.autograd.grad(Y3, X3, _dev(Gn))
    assert torch.equal(Y3, Y) and torch.equal(dX3, dX)
    g = hg.KnnHypergraph.build(c["P"], 10)
    assert torch.equal(g.idx, idx) and torch.equal(g.ptr_v, tp[0]) and torch.equal(g.pos_v, tp[1])
    assert torch.allclose(g.degE, hyperg.degE, rtol=1e-7, atol=0) and torch.allclose(g.degV, hyperg.degV, rtol=1e-6, atol=0)
    if weighted:
        assert torch.equal(g.weights(), w)


@pytest.mark.parametrize("probabilistic", [False, True])
@pytest.mark.parametrize("segments", [None, [0, 100, 300]])
def test_layer_against_the_planned_layer(hg, probabilistic, segments):
    torch.manual_seed(9)
    X = torch.randn(300, 12, device=DEV)
    G = torch.randn(300, 32, device=DEV)
    old = hg.DynamicHypergraphConv(12, 32, k=10, probabilistic=probabilistic, segments=segments).to(DEV)
    new = hg.DynamicHypergraphConv(12, 32, k=10, probabilistic=probabilistic, segments=segments, device_graph=True).to(DEV)
    new.load_state_dict(old.state_dict())
    outs = []
    with hg.ops.options(backward="adjoint"):  # the planned sum operator's true gradient, which knn_aggr's always is
        for layer in (old, new):
            x = X.clone().requires_grad_(True)
            y = layer(x)
            gx, gw = torch.autograd.grad(y, (x, layer.lin.weight), G)
            outs.append((y.detach(), gx, gw))
    assert isinstance(new.hyperg, hg.KnnHypergraph)
    assert torch.equal(new.hyperg.idx.reshape(-1), old.hyperg.H_T_colind)
    for a, b, what in zip(outs[1], outs[0], ("output", "input gradient", "weight gradient")):
        _assert_close(a, _np(b).astype(np.float64), what)


def test_layer_capture_searches_again_on_replay(hg):
    torch.manual_seed(13)
    layer = hg.DynamicHypergraphConv(16, 16, k=4, device_graph=True).to(DEV)
    Xa, Xb = torch.randn(130, 16, device=DEV), torch.randn(130, 16, device=DEV)
    G = torch.randn(130, 16, device=DEV)

    def eager(X):
        layer.lin.weight.grad = None
        y = layer(X)
        y.backward(G)
        return y.detach().clone(), layer.lin.weight.grad.detach().clone(), layer.hyperg.idx.clone()

    ya, ga, ia = eager(Xa)
    yb, gb, ib = eager(Xb)
    assert not torch.equal(ia, ib)  # a stale graph could not pass: the neighbours differ between the two inputs
    static_x = Xa.clone()
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
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_y, ya) and torch.equal(layer.lin.weight.grad, ga) and torch.equal(static_idx, ia)
    static_x.copy_(Xb)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_idx, ib)
    assert torch.equal(static_y, yb) and torch.equal(layer.lin.weight.grad, gb)
