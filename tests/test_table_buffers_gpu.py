"""The kNN search (both forms), the table transpose and the two table gathers called through the C entries into guarded,
poisoned, caller-owned buffers (-m gpu; tests/_raw_table.py): every output and the workspace sit between guard bands, the
workspace holds exactly the queried bytes, and each case runs under three poison words, with the outputs and the workspace on
a 256-byte boundary and one word past one -- the 4-byte alignment include/hg_aggr.h promises.

Every run: (a) the outputs equal the numpy reference bit for bit (the mean: within the bound test_knn_gpu.py and
test_knn_dot_gpu.py hold it to), (b) all six runs agree bit for bit, (c) no poison word is left in an element the contract
writes, (d) every guard band is intact, (e) the Python wrapper returns the same bits.  tests/test_table_buffers_host.py shows
on a host model that the poisons would change the answers if a slot that must hold a sentinel kept the buffer's word."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _buffer_cases as bc  # noqa: E402
import _knn_dot_ref as dr  # noqa: E402
import _knn_ref as kr  # noqa: E402
import _table_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U23 = 2.0 ** -23
RUNS = [(word, off) for word in bc.POISONS for off in (0, 1)]  # (poison, words past a 256-byte boundary)


@pytest.fixture(scope="module")
def rt(hg):
    import _raw_table
    return _raw_table


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _words(view):
    return view.cpu().numpy().copy()


def _f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _assert_written(rt, got, want, word, what):
    """(a) and (c): the words equal the reference's, and none that the reference does not itself hold is the poison."""
    p = rt.signed(word)
    assert not ((got == p) & (want != p)).any(), "%s: the poison %08x is left in %d elements" % (what, word, int(((got == p) & (want != p)).sum()))
    assert np.array_equal(got, want), "%s: %d words differ from the reference" % (what, int((got != want).sum()))


def _assert_mean(rt, words, want, tol, word, what):
    """The mean is held to a bound, not to bits: every element lies within `tol` of the float64 mean, and an element that holds
    the poison word does so only where the word is itself such a value (+0.0 for rows that are all identical) -- which the
    agreement of the six runs, under three different words, then shows was written."""
    with np.errstate(invalid="ignore"):
        m = words.view(np.float32).astype(np.float64)
        err = np.abs(m - want) / tol
        left = (words == rt.signed(word)) & ~(err <= 1)
    assert not left.any(), "%s: the poison %08x is left in %d elements of mean" % (what, word, int(left.sum()))
    print("%s: max mean error / bound = %.3g" % (what, float(err.max())))
    assert (err <= 1).all(), what


def _assert_guards(rt, pairs, what):
    for name, (buf, view) in pairs.items():
        assert view is None or rt.guards_intact(buf, view), "%s: a guard band of %s was written" % (what, name)


def _assert_same_runs(first, got, what):
    for name in first:
        assert np.array_equal(first[name], got[name]), "%s: %s differs from the first run's bits" % (what, name)


# ---- the difference form ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("name", [c["name"] for c in bc.DIFF_CASES])
def test_difference_form(hg, rt, name, with_mean):
    c = bc.DIFF_BY_NAME[name]
    X, Q, _ = bc.diff_inputs(name)
    want_idx, want_dist, want_mean = bc.diff_reference(name)
    n, F, k, cs = c["n"], bc.F_DIFF, c["k"], c["slices"]
    nq = n if Q is None else c["nq"]
    x = _dev(X)
    q = x if Q is None else _dev(Q)
    nbytes = rt.knn_workspace_bytes(nq, n, F, k, cs)
    assert nbytes == kr.workspace_bytes(nq, n, k, cs)
    if name == "one-slice-null-workspace":
        nbytes = 0  # the entry needs none for one slice and no segments: a NULL workspace of 0 bytes must do
    want_d = _f32_bits(want_dist)
    assert np.array_equal(want_d.view(np.float32).astype(np.float64), want_dist)
    first = None
    for word, off in RUNS:
        what = "%s mean=%s poison %08x offset %d" % (name, with_mean, word, off)
        pairs = dict(idx=rt.guarded(nq * k, word, off), dist=rt.guarded(nq * k, word, off),
                     mean=rt.guarded(nq, word, off) if with_mean else (None, None),
                     workspace=rt.guarded_bytes(nbytes, word, off))
        if nbytes:
            assert pairs["workspace"][1].numel() * 4 == nbytes and pairs["workspace"][1].data_ptr() % 256 == 4 * off
        rt.knn(q, x, k, pairs["idx"][1], pairs["dist"][1], pairs["mean"][1], c["seg"], c["self_first"], cs, pairs["workspace"][1])
        torch.cuda.synchronize()
        _assert_guards(rt, pairs, what)
        got = dict(idx=_words(pairs["idx"][1]).reshape(nq, k), dist=_words(pairs["dist"][1]).reshape(nq, k))
        _assert_written(rt, got["idx"], want_idx, word, what + ": idx")
        _assert_written(rt, got["dist"], want_d, word, what + ": dist")
        if with_mean:
            got["mean"] = _words(pairs["mean"][1])
            _assert_mean(rt, got["mean"], want_mean, (n + F) * U23 * np.maximum(want_mean, 1e-300), word, what)
        first = got if first is None else first
        _assert_same_runs(first, got, what)
    res = hg.ops.knn(x, k, queries=None if Q is None else q, segments=None if c["seg"] is None else list(c["seg"]),
                     self_first=c["self_first"], return_mean=with_mean, cand_slices=cs)
    wrapped = dict(zip(("idx", "dist", "mean"), (_words(t.view(torch.int32)) for t in res)))
    _assert_same_runs(first, wrapped, name + ": ops.knn")


# ---- the dot form ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_mean,with_fallback", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("name", [c["name"] for c in bc.DOT_CASES])
def test_dot_form(hg, rt, name, with_mean, with_fallback):
    c = bc.DOT_BY_NAME[name]
    X, Q, _, _ = bc.dot_inputs(name)
    want_idx, want_dist, want_fb, want_mean = bc.dot_reference(name)
    n, F, k, cs = c["n"], c["F"], c["k"], c["cand_slices"]
    nq = n if Q is None else c["nq"]
    x = _dev(X)
    q = x if Q is None else _dev(Q)
    nbytes = rt.knn_dot_workspace_bytes(nq, n, F, k, cs)
    assert nbytes == dr.dot_workspace_bytes(nq, n, k, dr.dot_slices(nq, n, cs))
    want_d = _f32_bits(want_dist)
    E1 = dr.bound(X if Q is None else Q, X).astype(np.float64)
    tol = np.sqrt(E1) + (n + 2) * U23 * (want_mean + np.sqrt(E1)) + 2.0 ** -63  # test_knn_dot_gpu.py's bound
    first = None
    for word, off in RUNS:
        what = "%s mean=%s fallback=%s poison %08x offset %d" % (name, with_mean, with_fallback, word, off)
        pairs = dict(idx=rt.guarded(nq * k, word, off), dist=rt.guarded(nq * k, word, off),
                     mean=rt.guarded(nq, word, off) if with_mean else (None, None),
                     fallback=rt.guarded(nq, word, off) if with_fallback else (None, None),
                     workspace=rt.guarded_bytes(nbytes, word, off))
        assert pairs["workspace"][1].numel() * 4 == nbytes and pairs["workspace"][1].data_ptr() % 256 == 4 * off
        rt.knn_dot(q, x, k, pairs["idx"][1], pairs["dist"][1], pairs["mean"][1], pairs["fallback"][1], c["self_first"], cs,
                   pairs["workspace"][1])
        torch.cuda.synchronize()
        _assert_guards(rt, pairs, what)
        got = dict(idx=_words(pairs["idx"][1]).reshape(nq, k), dist=_words(pairs["dist"][1]).reshape(nq, k))
        _assert_written(rt, got["idx"], want_idx, word, what + ": idx")
        _assert_written(rt, got["dist"], want_d, word, what + ": dist")
        if with_fallback:
            got["fallback"] = _words(pairs["fallback"][1])
            _assert_written(rt, got["fallback"], want_fb, word, what + ": fallback")
        if with_mean:
            got["mean"] = _words(pairs["mean"][1])
            _assert_mean(rt, got["mean"], want_mean, tol, word, what)
        first = got if first is None else first
        _assert_same_runs(first, got, what)
    res = hg.ops.knn(x, k, queries=None if Q is None else q, self_first=c["self_first"], return_mean=with_mean, cand_slices=cs,
                     form="dot", return_fallback=with_fallback)
    names = ("idx", "dist") + (("mean",) if with_mean else ()) + (("fallback",) if with_fallback else ())
    wrapped = {key: _words(t.view(torch.int32)) for key, t in zip(names, res)}
    _assert_same_runs(first, wrapped, name + ": ops.knn(form='dot')")


# ---- the transpose ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(bc.TABLES))
def test_transpose(hg, rt, name):
    idx, n = bc.TABLES[name]
    rows, k = idx.shape
    want_ptr, want_pos = tr.transpose(idx, n)
    valid = int(want_ptr[n])
    assert valid == want_pos.shape[0] <= rows * k
    idx_d = _dev(idx)
    nbytes = rt.transpose_workspace_bytes(rows, k, n)
    assert nbytes == tr.transpose_workspace_bytes(rows, k, n)
    for word, off in RUNS:
        what = "%s poison %08x offset %d" % (name, word, off)
        pairs = dict(ptr_v=rt.guarded(n + 1, word, off), pos_v=rt.guarded(rows * k, word, off),
                     workspace=rt.guarded_bytes(nbytes, word, off))
        assert pairs["workspace"][1].numel() * 4 == nbytes and pairs["workspace"][1].data_ptr() % 256 == 4 * off
        rt.transpose(idx_d, n, pairs["ptr_v"][1], pairs["pos_v"][1], pairs["workspace"][1])
        torch.cuda.synchronize()
        _assert_guards(rt, pairs, what)
        _assert_written(rt, _words(pairs["ptr_v"][1]), want_ptr, word, what + ": ptr_v")
        # pos_v is unspecified from ptr_v[n] on: only the valid entries are compared
        _assert_written(rt, _words(pairs["pos_v"][1])[:valid], want_pos, word, what + ": pos_v")
    ptr, pos = hg.ops.knn_transpose(idx_d, n)
    assert np.array_equal(_words(ptr), want_ptr) and np.array_equal(_words(pos)[:valid], want_pos), name + ": ops.knn_transpose"


# ---- the gathers -----------------------------------------------------------------------------------------------------------

WIDTHS = (1, 3, 33, 130, 260)


def _dst_runs(rt, count):
    """Guarded, poisoned destinations of `count` floats: each poison, on a 16-byte boundary and one float past one."""
    for word, off in RUNS:
        buf, view = rt.guarded(count, word, off)
        assert view.data_ptr() % 16 == 4 * off
        yield word, off, buf, view


@pytest.mark.parametrize("rows", [1, 65])
@pytest.mark.parametrize("F", WIDTHS)
def test_gather(hg, rt, F, rows):
    from hypergef_amd import knn_graph as kg
    rng = np.random.default_rng(100 * F + rows)
    n, k = 40, 7
    idx = rng.integers(0, n, (rows, k)).astype(np.int32)
    idx[0, 1], idx[rows - 1, 3] = -1, n  # ignored entries
    src = rng.standard_normal((n, F)).astype(np.float32)
    w = (rng.random(rows * k) + 0.5).astype(np.float32)
    ds = rng.standard_normal(rows).astype(np.float32)
    want = _f32_bits(tr.gather(idx, src, w, None, ds))
    idx_d, src_d, w_d, ds_d = _dev(idx), _dev(src), _dev(w), _dev(ds)
    assert src_d.data_ptr() % 16 == 0
    for word, off, buf, dst in _dst_runs(rt, rows * F):
        what = "gather F=%d rows=%d poison %08x offset %d" % (F, rows, word, off)
        rt.gather(idx_d, n, src_d, dst, w_d, None, ds_d)
        torch.cuda.synchronize()
        assert rt.guards_intact(buf, dst), what + ": a guard band of dst was written"
        _assert_written(rt, _words(dst).reshape(rows, F), want, word, what)
    wrapped = kg.table_gather(idx_d, src_d, w_d, None, ds_d)
    assert np.array_equal(_words(wrapped.view(torch.int32)), want), "table_gather F=%d rows=%d" % (F, rows)


@pytest.mark.parametrize("F", WIDTHS)
def test_gather_t_over_hubs(hg, rt, F):
    """The transposed gather over a _table_ref.hub_table: vertex rows above HG_TABLE_SEQ_MAX entries in every place of a
    workgroup, beside short rows, one of exactly that length and an empty one, which must be +0.0 and not the poison.  The
    lanes take four columns where F % 4 == 0 and src and dst stand on 16-byte boundaries, else one: the table and the
    expected bits follow the destination's alignment."""
    from hypergef_amd import knn_graph as kg
    seq, k = kg.table_seq_max(), 2
    expected = {}
    for word, off in RUNS:
        aligned = off == 0
        shape = tr.long_row_shape(F, aligned)
        if shape not in expected:
            t = tr.hub_table(F, aligned, seq, seed=F)
            idx, n = t["idx"], t["n"]
            rows = idx.shape[0]
            rng = np.random.default_rng(500 + F)
            src = rng.standard_normal((rows, F)).astype(np.float32)
            w = (rng.random(rows * k) + 0.5).astype(np.float32)
            ds = rng.standard_normal(n).astype(np.float32)
            ptr, pos = tr.transpose(idx, n)
            lens = np.diff(ptr)
            assert (lens[t["hubs"]] > seq).all() and lens[t["full"]] == seq and lens[t["empty"]] == 0
            want = tr.gather_t_ordered(ptr, pos, k, src, w, None, ds, aligned16=aligned, seq_max=seq)
            assert not want[t["empty"]].any() and not np.signbit(want[t["empty"]]).any()
            expected[shape] = dict(t=t, n=n, want=_f32_bits(want), dev=[_dev(a) for a in (ptr, pos, src, w, ds)])
        e = expected[shape]
        n, (ptr_d, pos_d, src_d, w_d, ds_d) = e["n"], e["dev"]
        assert src_d.data_ptr() % 16 == 0
        what = "gather_t F=%d poison %08x offset %d" % (F, word, off)
        buf, dst = rt.guarded(n * F, word, off)
        assert dst.data_ptr() % 16 == 4 * off
        rt.gather_t(ptr_d, pos_d, k, src_d, dst, w_d, None, ds_d)
        torch.cuda.synchronize()
        assert rt.guards_intact(buf, dst), what + ": a guard band of dst was written"
        got = _words(dst).reshape(n, F)
        assert not got[e["t"]["empty"]].any(), what + ": the vertex with no entry is not +0.0"
        _assert_written(rt, got, e["want"], word, what)
        if aligned and word == bc.POISONS[0]:
            wrapped = kg.table_gather_t(ptr_d, pos_d, k, src_d, w_d, None, ds_d)
            assert wrapped.data_ptr() % 16 == 0
            assert np.array_equal(_words(wrapped.view(torch.int32)), e["want"]), "table_gather_t F=%d" % F
