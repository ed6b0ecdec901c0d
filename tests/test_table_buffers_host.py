"""Proof, without a device, that tests/test_table_buffers_gpu.py can fail: for every case whose lists have unused slots, the
slots are overwritten with each poison word and a numpy model of the kernel that reads them (knn_merge_kernel's rank search,
the dot form's rerank over its merged shortlists, the transpose's radix passes on counters that start at the word) must give
another answer than the reference.  The models with nothing poisoned must give the reference itself.

Where a word cannot change the answer the test says so and asserts that too, so that the claim is checked and not assumed:
  0x00000000 in the transpose's counters is the value they must start from;
  0xFFFFFFFF in the dot form's shortlists: only the last slice can be short (every tile but the last is full, and a tile holds
    more rows than a shortlist), and a tail of NaN keys in the last list ends every binary search where the sentinels would.
    That word still guards the norms, the partial means and the outputs on the device.
Also here: the constants mirrored from csrc/hg_knn.h and hg_table.h, and the workspace sizes the device cases rely on."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _buffer_cases as bc  # noqa: E402
import _knn_dot_ref as dr  # noqa: E402
import _knn_ref as kr  # noqa: E402
import _table_ref as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hypergef_amd", "csrc")


def _constant(text, name):
    m = re.search(r"constexpr int %s = ([^;]+);" % name, text)
    assert m, name
    return m.group(1).strip()


def test_constants_mirror_the_headers():
    knn = open(os.path.join(CSRC, "hg_knn.h")).read()
    for name, value in (("kKnnTQ", kr.KNN_TQ), ("kKnnTC", kr.KNN_TC), ("kDotTQ", kr.DOT_TQ), ("kDotTC", kr.DOT_TC),
                        ("kDotNormRows", kr.DOT_NORM_ROWS), ("kKnnMaxSlices", kr.KNN_MAX_SLICES), ("kKnnMaxK", kr.KNN_MAX_K)):
        assert int(_constant(knn, name)) == value, name
    assert "return (k + 16 + 31) / 32;" in knn  # knn_dot_slots, which _knn_dot_ref.slots mirrors
    table = open(os.path.join(CSRC, "hg_table.h")).read()
    assert int(_constant(table, "kTableBlock")) * int(_constant(table, "kTableItems")) == tr.TABLE_TILE
    assert _constant(table, "kTableTile") == "kTableBlock * kTableItems"
    assert int(_constant(table, "kTableRadixBits")) == tr.TABLE_RADIX_BITS


def test_workspace_sizes_the_cases_rely_on(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    for c in bc.DIFF_CASES:
        nq = c["n"] if c["nq"] is None else c["nq"]
        got = L.hg_knn_workspace_bytes(nq, c["n"], bc.F_DIFF, c["k"], c["slices"])
        assert got == kr.workspace_bytes(nq, c["n"], c["k"], c["slices"]) and got % 4 == 0, c["name"]
    # slices that own no candidate tile are counted: 31 more lists and partial means than one slice has
    one = L.hg_knn_workspace_bytes(300, 300, 3, 64, 1)
    assert L.hg_knn_workspace_bytes(300, 300, 3, 64, 32) - one == 31 * 300 * (8 * 64 + 4)
    # one slice and no segments: nothing is needed when the queries are rows of their own
    assert L.hg_knn_workspace_bytes(5, 300, 3, 10, 1) == 0 and kr.auto_slices(300, 300) == 2 and kr.auto_slices(300, 200) == 1
    assert (dr.dot_kp(20, 10), dr.dot_kp(257, 10), dr.dot_kp(300, 64)) == (20, 32, 96)
    for c in bc.DOT_CASES:
        nq = c["n"] if c["nq"] is None else c["nq"]
        slices = dr.dot_slices(nq, c["n"], c["cand_slices"])
        got = L.hg_knn_dot_workspace_bytes(nq, c["n"], c["F"], c["k"], c["cand_slices"])
        assert got == dr.dot_workspace_bytes(nq, c["n"], c["k"], slices) and got % 4 == 0, c["name"]
        assert slices == (1 if c["cand_slices"] == 1 or c["n"] <= 128 else 3), c["name"]  # 32 and 0 are clipped to the tiles
    # kp sets the size of a list: one more slice costs nq (8 kp + 4) bytes before the rounding of its three pieces
    for n, k, kp in ((257, 10, 32), (300, 64, 96)):
        step = L.hg_knn_dot_workspace_bytes(64, n, 3, k, 2) - L.hg_knn_dot_workspace_bytes(64, n, 3, k, 1)
        assert step == 64 * (8 * kp + 4), (n, k, step)  # 64 rows: every piece is a multiple of 256 bytes
    for name, (idx, n) in bc.TABLES.items():
        rows, k = idx.shape
        got = L.hg_table_transpose_workspace_bytes(rows, k, n)
        assert got == tr.transpose_workspace_bytes(rows, k, n) and got % 4 == 0, name
    assert [tr.radix_passes(n) for n in (1, 7, 50, 255, 256, 2 ** 20 + 3)] == [1, 1, 1, 1, 2, 3]


def _bits(word):
    return np.array([word], np.uint32).view(np.float32)[0], int(np.array([word], np.uint32).view(np.int32)[0])


def _rows_to_model(nq, slices, k):
    """Every row, or where the lists are long a spread of rows: the first and last query tiles' ends and the middle."""
    if nq * slices * k <= 120000:
        return np.arange(nq)
    return np.unique(np.concatenate([np.arange(6), np.arange(nq // 2 - 3, nq // 2 + 3), np.arange(nq - 6, nq)]))


@pytest.mark.parametrize("name", [c["name"] for c in bc.DIFF_CASES])
def test_difference_form_poisoned_slots_change_the_modelled_merge(name):
    c = bc.DIFF_BY_NAME[name]
    want_idx, want_dist, _ = bc.diff_reference(name)
    ld, lj, used, a, b = bc.diff_lists(name)
    nq, slices, k = ld.shape
    count = b - a
    assert (count.sum(1) == (kr.candidate_ranges(c["n"], nq, c["seg"])[1] - kr.candidate_ranges(c["n"], nq, c["seg"])[0])).all()
    # the model with the sentinels in place is the reference, on every row
    idx, dist = kr.merge(ld, lj)
    assert np.array_equal(idx, want_idx) and np.array_equal(dist.astype(np.float64), want_dist), name
    empty, partial = bool((count == 0).any()), bool(((count >= 1) & (count < k)).any())
    if c["slices"] == 32:
        assert (count == 0).all(0).sum() == 30, "30 of the 32 slices own no candidate of any row"
    if name == "seg-0-100-200-600":
        assert empty and not partial  # what these segments give; the next case has both
    if name == "seg-0-100-300-600":
        assert empty and partial
        X = bc.diff_inputs(name)[0]
        assert np.array_equal(X[250], X[210]) and want_idx[250, :2].tolist() == [250, 210] and want_idx[210, :2].tolist() == [210, 250]
    if not c["sensitive"]:
        # kept beside the shape that replaces it: no unused slot at all, or only a tail of the last slice
        assert used.all() or used[:, :-1].all()
        if not used.all():  # the NaN tail of the last list is inert, as the cases' text says; the other two words are not
            rows = _rows_to_model(nq, slices, k)
            for word in bc.POISONS:
                got = kr.merge(*kr.poison_unused(ld, lj, used, word), rows)
                assert np.array_equal(got[0], want_idx[rows]) == (word == 0xFFFFFFFF), (name, hex(word))
        return
    assert not used.all()
    rows = _rows_to_model(nq, slices, k)
    for word in bc.POISONS:
        pd, pj = kr.poison_unused(ld, lj, used, word)
        got_idx, got_dist = kr.merge(pd, pj, rows)
        differs = not (np.array_equal(got_idx, want_idx[rows]) and np.array_equal(got_dist.astype(np.float64), want_dist[rows]))
        carried = bool(np.isnan(got_dist).any() or (got_idx == -1).any())
        print("%s poison %08x: %d of %d modelled rows differ%s" % (name, word, int(((got_idx != want_idx[rows]).any(1)
              | (got_dist.astype(np.float64) != want_dist[rows]).any(1)).sum()), rows.shape[0], ", NaN or -1 carried" if carried else ""))
        assert differs or carried, "%s: poison %08x leaves the modelled answer as it is" % (name, word)


@pytest.mark.parametrize("name", [c["name"] for c in bc.DOT_CASES])
def test_dot_form_poisoned_shortlists_change_the_modelled_rerank(name):
    c = bc.DOT_BY_NAME[name]
    X, Q, D32, est = bc.dot_inputs(name)
    want = bc.dot_reference(name)
    nq = est.shape[0]
    if c["kind"] == "ints":  # exact estimates and distances: the float64 reference is the same selection, bit for bit
        assert np.array_equal(est, D32)
        ref = kr.knn(X, c["k"], queries=Q, self_first=c["self_first"])
        assert np.array_equal(want[0], ref[0]) and np.array_equal(want[1].astype(np.float64), ref[1]), name
    elif name == "identical":
        assert dr.never_certifiable(None, X, c["k"]) and want[2].all()
    else:
        assert not want[2][:240].any() and want[2][240:].all()
    slices = dr.dot_slices(nq, c["n"], c["cand_slices"])
    ld, lj, used = dr.shortlists(est, c["k"], slices, c["self_first"])
    got = dr.rerank(X, c["k"], ld, lj, Q, c["self_first"], D32=D32)
    for g, w in zip(got, want[:3]):
        assert np.array_equal(g, w), name
    assert used.all() != c["short"], name
    if not c["short"]:
        return
    assert used[:, :-1].all() and not used[:, -1].all()  # only the last slice is short
    for word in bc.POISONS:
        pd, pj = kr.poison_unused(ld, lj, used, word)
        got = dr.rerank(X, c["k"], pd, pj, Q, c["self_first"], D32=D32)
        same = all(np.array_equal(g, w) for g, w in zip(got, want[:3]))
        print("%s poison %08x: idx differs in %d rows, fallback in %d" % (name, word, int((got[0] != want[0]).any(1).sum()),
                                                                         int((got[2] != want[2]).sum())))
        if word == 0xFFFFFFFF:
            assert same, "a NaN tail of the last shortlist is inert in the rank search; if this fails, tighten the module's text"
        else:
            assert not same, "%s: poison %08x leaves the modelled answer as it is" % (name, word)


@pytest.mark.parametrize("name", list(bc.TABLES))
def test_transpose_counters_that_start_at_the_poison_change_the_modelled_sort(name):
    idx, n = bc.TABLES[name]
    want_ptr, want_pos = tr.transpose(idx, n)
    valid = int(want_ptr[n])
    clean = tr.radix_model(idx, n)
    assert np.array_equal(clean[:valid], want_pos), name
    flat = idx.reshape(-1)
    assert ((flat[clean[valid:]] < 0) | (flat[clean[valid:]] >= n)).all()  # the ignored entries sort behind every vertex
    if name == "ignored-entries":
        assert valid < idx.size and (flat == -1).any() and (flat >= n).any()
    for word in bc.POISONS:
        _, start = _bits(word)
        got = tr.radix_model(idx, n, hist0=start, fill=start)
        same = got is not None and np.array_equal(got[:valid], want_pos)
        if word == 0:
            assert same  # the value the counters must start from
        else:
            assert not same, "%s: counters that start at %08x leave the modelled sort as it is" % (name, word)
