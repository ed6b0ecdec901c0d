"""The cases of tests/test_table_buffers_gpu.py and test_table_buffers_host.py: the inputs, the references and the three poison
words.  Numpy only.  Every row is integer-valued (randint(-4, 5), except the two named inputs of _knn_dot_ref.case), so that
every distance is exact in float32 and the references decide every bit of idx and dist.

A case is `sensitive` where the host model shows that a poison word in its unused list slots changes the answer; the cases
that are not are kept beside the shape that replaces them and say why:
  n = 300 under 2 slices: both slices hold at least k candidates at k = 1 and 33 (no unused slot), and at k = 64 the short
    slice is the last one, where a tail of NaN keys ends every binary search of the merge at the place the sentinels would --
    n = 200 under 2 slices (one candidate tile, which slice 1 takes: slice 0 is empty) replaces them;
  one slice and a NULL workspace: there is no list to poison.
At k = 1 the queries are rows of their own: with Q == X every row is at distance 0 from itself, which nothing in a poisoned
slot ranks before except the word 0.
"""
import functools

import numpy as np

import _knn_dot_ref as dr
import _knn_ref as kr

POISONS = (0x00000000, 0xFFFFFFFF, 0x00000001)
F_DIFF = 3


def ints(n, F, seed):
    return np.random.default_rng(seed).integers(-4, 5, (n, F)).astype(np.float32)


# ---- the difference form ---------------------------------------------------------------------------------------------------

def _diff(name, n, k, slices, nq=None, seg=None, sensitive=True):
    return dict(name=name, n=n, k=k, slices=slices, nq=nq, seg=seg, self_first=nq is None, sensitive=sensitive)


DIFF_CASES = (
    [_diff("n300-k%d-s%d" % (k, s), 300, k, s, nq=300 if k == 1 else None, sensitive=s == 32)
     for k in (1, 33, 64) for s in (2, 32)]
    + [_diff("n200-k%d-s2" % k, 200, k, 2, nq=200 if k == 1 else None) for k in (1, 33, 64)]
    + [_diff("q5-n300-k33-s32", 300, 33, 32, nq=5),
       # segments of 100, 100 and 400 rows: rows 0 .. 191 meet one candidate tile, which slice 2 takes (slices 0 and 1 are empty
       # for them), but no (row, slice) pair holds 1 .. k - 1 candidates; under the second set of segments rows 100 .. 127
       # find 44 candidates of their segment [100, 300) in slice 2
       _diff("seg-0-100-200-600", 600, 64, 3, seg=(0, 100, 200, 600)),
       _diff("seg-0-100-300-600", 600, 64, 3, seg=(0, 100, 300, 600)),
       _diff("one-slice-null-workspace", 300, 10, 1, sensitive=False)])
DIFF_BY_NAME = {c["name"]: c for c in DIFF_CASES}


@functools.lru_cache(maxsize=None)
def diff_inputs(name):
    """(X, Q or None, D float64 [nq, n])."""
    c = DIFF_BY_NAME[name]
    X = ints(c["n"], F_DIFF, 7000 + c["n"] + c["k"])
    if c["seg"] is not None:
        X[250] = X[210]  # two identical rows of one segment: self_first puts 250 before 210 in row 250
    Q = None if c["nq"] is None else ints(c["nq"], F_DIFF, 7500 + c["k"])
    return X, Q, kr.distances(X if Q is None else Q, X)


@functools.lru_cache(maxsize=None)
def diff_reference(name):
    """(idx int32, dist float64, mean float64) of tests/_knn_ref.knn."""
    c = DIFF_BY_NAME[name]
    X, Q, D = diff_inputs(name)
    return kr.knn(X, c["k"], queries=Q, segments=c["seg"], self_first=c["self_first"], D=D)


def diff_lists(name):
    """The case's slice lists with correct sentinels (ld, lj, used) and its slice ranges (a, b)."""
    c = DIFF_BY_NAME[name]
    X, Q, D = diff_inputs(name)
    nq = c["n"] if Q is None else c["nq"]
    a, b = kr.slice_ranges(nq, c["n"], c["slices"], c["seg"])
    return kr.slice_lists(D, c["k"], a, b, c["self_first"]) + (a, b)


# ---- the dot form ----------------------------------------------------------------------------------------------------------

def _dot(name, n, k, cand_slices, F, nq=None, kind="ints", short=False):
    return dict(name=name, n=n, k=k, cand_slices=cand_slices, F=F, nq=nq, kind=kind, self_first=nq is None, short=short)


DOT_CASES = []
for _F in (3, 33):
    DOT_CASES += [
        _dot("n20-k10-F%d" % _F, 20, 10, 0, _F),                                    # kp = n = 20: one full list
        _dot("n257-q65-k10-cs1-F%d" % _F, 257, 10, 1, _F, nq=65),                   # one slice over three tiles
        _dot("n257-q65-k10-cs0-F%d" % _F, 257, 10, 0, _F, nq=65, short=True),       # three slices, the last of one row
        _dot("n257-q65-k10-cs32-F%d" % _F, 257, 10, 32, _F, nq=65, short=True),     # 32 slices clipped to 3
        _dot("n257-self-k10-cs0-F%d" % _F, 257, 10, 0, _F, short=True),             # the same with Q == X
        _dot("n300-k64-cs0-F%d" % _F, 300, 64, 0, _F, short=True),                  # kp = 96, the last tile has 44 rows
        _dot("n300-q70-k64-cs0-F%d" % _F, 300, 64, 0, _F, nq=70, short=True)]
DOT_CASES += [_dot("identical", dr.CASE_N, dr.CASE_K, 0, dr.CASE_F, kind="identical"),
              _dot("mixed", dr.CASE_N, dr.CASE_K, 0, dr.CASE_F, kind="mixed")]
DOT_BY_NAME = {c["name"]: c for c in DOT_CASES}


@functools.lru_cache(maxsize=None)
def dot_inputs(name):
    """(X, Q or None, D32 float32 [nq, n], est float32 [nq, n])."""
    c = DOT_BY_NAME[name]
    X = ints(c["n"], c["F"], 8000 + c["n"] + c["F"]) if c["kind"] == "ints" else dr.case(c["kind"])
    Q = None if c["nq"] is None else ints(c["nq"], c["F"], 8500 + c["F"])
    Qa = X if Q is None else Q
    return X, Q, dr.d2_f32(Qa, X), dr.estimates(Qa, X)


@functools.lru_cache(maxsize=None)
def dot_reference(name):
    """(idx int32, dist float32, fallback int32) of _knn_dot_ref.scheme on the kernels' estimates, and the float64 mean."""
    c = DOT_BY_NAME[name]
    X, Q, D32, est = dot_inputs(name)
    idx, dist, fb = dr.scheme(X, c["k"], est, Q, c["self_first"], D32=D32)
    mean = np.sqrt(kr.distances(X if Q is None else Q, X)).mean(1)
    return idx, dist, fb, mean


# ---- the transpose ---------------------------------------------------------------------------------------------------------

def _tables():
    rng = np.random.default_rng(9000)
    t = {}
    t["below-one-tile"] = (rng.integers(0, 50, (31, 64)).astype(np.int32), 50)   # 1984 entries
    t["one-tile"] = (rng.integers(0, 50, (32, 64)).astype(np.int32), 50)         # 2048
    t["one-tile-and-one"] = (rng.integers(0, 50, (2049, 1)).astype(np.int32), 50)
    # n = 1: every valid entry has the digit 0, whose first tile starts at 0 whatever the counters held -- so two tiles, the
    # second of which starts where the first one's count says; and two ignored entries, whose key is n itself
    one = np.zeros((700, 3), np.int32)
    one[1, 2], one[699, 0] = -1, 1
    t["n1"] = (one, 1)
    n = 2 ** 20 + 3
    wide = rng.integers(0, n, (65, 2)).astype(np.int32)  # 130 entries, keys of 21 bits: three passes
    wide[0, 0], wide[64, 1], wide[3, 1] = n - 1, 0, wide[2, 0]
    t["wide-keys"] = (wide, n)
    ign = rng.integers(-1, 8, (40, 5)).astype(np.int32)  # -1 and 7 = n are ignored
    ign[0, 0], ign[39, 4], ign[7, 2] = -1, 7, 2 ** 31 - 1
    t["ignored-entries"] = (ign, 7)
    return t


TABLES = _tables()
