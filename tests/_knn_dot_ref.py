"""The scheme of ops.knn(form="dot") in numpy: CPU, test infrastructure only (include/hg_aggr.h, hg_knn_dot_f32).

    shortlist   the kp = min(n, k + slack) smallest candidates of row i under (estimate(i, j), j); with self_first row i itself
                is ranked before everything
    rerank      the shortlist's float32 difference-form distances (d2_f32: q - x, then one fma per column into one
                accumulator), the k smallest under (d2, j)
    certify     T = the largest shortlisted estimate, E1 = bound(Q, X)[i], Ei = E1 + (F + 4) u max(T, 0), all in float32 as
                the kernel computes them: certified iff n <= kp or the k-th d2 < T - Ei, strictly
    fall back   a row that is not certified selects from all n candidates by d2_f32

`estimate` is injectable: whatever it returns, the output must be the exhaustive selection on d2_f32 as long as
|estimate - d2_f64| <= E1 -- that is the certificate's claim, and tests hand it the truth perturbed adversarially.

float32 fma chains are emulated as float32(float64(a) * float64(b) + float64(acc)): the product is exact in float64; the sum
is rounded twice, which differs from one rounding only where the float64 sum falls on a float32 tie -- never on
integer-valued rows, where every value is exact."""
import numpy as np

import _knn_ref as kr

U = np.float32(2.0 ** -24)
F_MAX = 65536
F32 = np.float32


def slots(k):
    return (k + 16 + 31) // 32


def default_slack(k):
    """32 slots(k) - k, 16 .. 47: the shortlist fills whole 32-slot register rows and keeps at least 16 spare."""
    return 32 * slots(k) - k


def _fma32(a, b, acc):
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(F32)


def norms(X):
    """n2[j] = sum_c X[j, c]^2 in float32, one fma per column in column order."""
    X = np.asarray(X, F32)
    acc = np.zeros(X.shape[0], F32)
    for c in range(X.shape[1]):
        acc = _fma32(X[:, c], X[:, c], acc)
    return acc


def d2_f32(Q, X):
    """The difference-form distances [nq, n] in float32 as knn_kernel computes them."""
    Q, X = np.asarray(Q, F32), np.asarray(X, F32)
    acc = np.zeros((Q.shape[0], X.shape[0]), F32)
    for c in range(X.shape[1]):
        d = (Q[:, c][:, None] - X[:, c][None, :]).astype(F32)
        acc = _fma32(d, d, acc)
    return acc


def bound(Q, X):
    """E1 [nq] float32, as the kernel computes it: |d~(i, j) - d2_f64(i, j)| <= E1[i] for every candidate j."""
    return _bound(Q, X)[0]


def _bound(Q, X):
    """(E1, n2q + n2max), both float32 [nq]."""
    F = np.asarray(X).shape[1]
    assert 1 <= F <= F_MAX
    total = (norms(Q) + norms(X).max()).astype(F32)
    c2 = 2 * F + 4
    C = F32(c2 + (c2 >> 6) + 1) * U
    return (C * total + F32(F + 2) * F32(2.0 ** -146)).astype(F32), total


def _lower(T, E1, F):
    """T - Ei in float32."""
    T = F32(T)
    Ei = F32(E1 + (F32(F + 4) * U) * max(T, F32(0)))
    return F32(T - Ei)


def _select(key, k):
    j = np.arange(key.shape[0])
    return np.lexsort((j, key))[:k]


def scheme(X, k, estimate, queries=None, self_first=None, slack=None, D32=None):
    """(idx int32 [nq, k], dist float32 [nq, k], fallback int32 [nq]).  estimate: [nq, n] array of d~."""
    X = np.asarray(X, F32)
    Q = X if queries is None else np.asarray(queries, F32)
    if self_first is None:
        self_first = queries is None
    nq, n, F = Q.shape[0], X.shape[0], X.shape[1]
    kp = min(n, k + (default_slack(k) if slack is None else slack))
    if D32 is None:
        D32 = d2_f32(Q, X)
    E1, total = _bound(Q, X)
    idx = np.empty((nq, k), np.int32)
    dist = np.empty((nq, k), F32)
    fallback = np.zeros(nq, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(nq):
            est = np.asarray(estimate[i], np.float64).copy()
            if self_first:
                est[i] = -np.inf
            short = _select(est, kp)
            exact = D32[i].astype(np.float64)
            if self_first:
                exact[i] = -1.0
            pick = short[np.lexsort((short, exact[short]))[:k]]
            certified = n <= kp
            if not certified:
                certified = bool(total[i] < F32(1e37)) and bool(exact[pick[-1]] < _lower(est[short[-1]], E1[i], F))
            if not certified:
                fallback[i] = 1
                pick = _select(exact, k)
            idx[i] = pick
            dist[i] = np.maximum(D32[i, pick], 0)
    return idx, dist, fallback


def exhaustive(X, k, queries=None, self_first=None, D32=None):
    """The selection on d2_f32 over all candidates: what form="difference" returns."""
    Q = X if queries is None else queries
    n = np.asarray(X).shape[0]
    est = np.zeros((np.asarray(Q).shape[0], n))
    return scheme(X, k, est, queries, self_first, slack=n, D32=D32)[:2]


def perturbed(D64, E1, D_true_rank_k, mode, rng):
    """The float64 truth moved by up to E1 per row, as float32 values that still lie within E1 of it.  mode 'exclude':
    the k true neighbours of every row up, everything else down; 'random': uniform in the bound."""
    E = E1.astype(np.float64)[:, None]
    if mode == "exclude":
        sign = np.where(D_true_rank_k, 1.0, -1.0)
    else:
        sign = rng.uniform(-1.0, 1.0, D64.shape)
    est = (D64 + sign * E).astype(F32)
    off = np.abs(est.astype(np.float64) - D64) > E  # the rounding to float32 stepped outside: one step back
    est[off] = np.nextafter(est[off], D64.astype(F32)[off])
    assert (np.abs(est.astype(np.float64) - D64) <= E).all()
    return est


def _sorted_truth(Q, X, self_first):
    D64 = kr.distances(Q, X)
    D32 = d2_f32(Q, X).astype(np.float64)
    if self_first:
        i = np.arange(D64.shape[0])
        D64[i, i] = -np.inf  # always shortlisted, never the threshold
        D32[i, i] = -1.0
    return np.sort(D64, axis=1), np.sort(D32, axis=1)


def _setup(Q, X, k, slack, self_first):
    X = np.asarray(X, F32)
    same = Q is None
    Q = X if same else np.asarray(Q, F32)
    if self_first is None:
        self_first = same
    n, F = X.shape
    kp = min(n, k + (default_slack(k) if slack is None else slack))
    return Q, X, self_first, n, F, kp


def certifiable(Q, X, k, slack=None, self_first=None):
    """True iff every row is certified whatever the estimates, as long as each is within E1 of the float64 truth.  A row is
    surely certified when n <= kp, or when (a) its k true neighbours cannot be pushed out of the shortlist,
    d2_(k) + E1 < d2_(kp + 1) - E1 in float64, and (b) its k-th d2_f32 is below T - Ei for the smallest T the estimates can
    give, T = d2_(kp) - E1 (T - Ei grows with T).  Q None: the rows of X themselves."""
    Q, X, self_first, n, F, kp = _setup(Q, X, k, slack, self_first)
    if n <= kp:
        return True
    S64, S32 = _sorted_truth(Q, X, self_first)
    E1, total = _bound(Q, X)
    for i in range(Q.shape[0]):
        E = float(E1[i])
        if not total[i] < F32(1e37) or not S64[i, k - 1] + E < S64[i, kp] - E:
            return False
        t_min = np.nextafter(F32(S64[i, kp - 1] - E), F32(-np.inf))
        if not S32[i, k - 1] < _lower(t_min, E1[i], F):
            return False
    return True


def never_certifiable(Q, X, k, slack=None, self_first=None):
    """True iff no row can be certified whatever the estimates within E1 of the truth: every shortlist's k-th d2_f32 is at
    least the true k-th, and T is at most d2_(kp) + E1."""
    Q, X, self_first, n, F, kp = _setup(Q, X, k, slack, self_first)
    if n <= kp:
        return False
    S64, S32 = _sorted_truth(Q, X, self_first)
    E1, total = _bound(Q, X)
    for i in range(Q.shape[0]):
        t_max = np.nextafter(F32(S64[i, kp - 1] + float(E1[i])), F32(np.inf))
        if total[i] < F32(1e37) and S32[i, k - 1] < _lower(t_max, E1[i], F):
            return False
    return True


CASE_N, CASE_F, CASE_K = 300, 64, 10


def case(name):
    """The inputs [300, 64] the device tests run at k = 10 and the host tests classify, by name.
    certified    randn rows: the 10th and the 33rd neighbour are about 13 apart, E1 is about 1e-3
    identical    all rows the same: every d2 is 0 and no T can exceed E1
    pairs        150 rows, each present twice (row 150 + i = row i), over 5 distinct integer rows: every row has 59 others at
                 exactly 0, more than the shortlist holds, so again no T exceeds E1 -- and every row's duplicates tie
    offset       1000 + 1e-3 randn: d2 is about 1e-4 and E1 about 1e3
    mixed        240 randn rows and a cluster of 60 rows at 10 + 1e-3 randn: the cluster's rows are 1e-4 apart under an E1 of
                 0.1, the others keep their gaps of about 13 under an E1 of 0.06"""
    rng = np.random.default_rng({"certified": 1, "identical": 2, "pairs": 3, "offset": 4, "mixed": 5}[name])
    n, F = CASE_N, CASE_F
    if name == "certified":
        X = rng.standard_normal((n, F))
    elif name == "identical":
        X = np.repeat(rng.standard_normal((1, F)), n, axis=0)
    elif name == "pairs":
        base = rng.integers(-4, 5, (5, F))[rng.permutation(np.repeat(np.arange(5), 30))]
        X = np.concatenate([base, base])
    elif name == "offset":
        X = 1000.0 + 1e-3 * rng.standard_normal((n, F))
    else:
        X = rng.standard_normal((n, F))
        X[240:] = 10.0 + 1e-3 * rng.standard_normal((60, F))
    return np.ascontiguousarray(X, F32)


# ---- the prefilter's slices, their shortlists and the rerank over them (csrc/hg_knn_dot.hip), as a host model ---------------

def estimates(Q, X):
    """d~ = (n2q + n2x) - 2 s~ in float32 as the kernels form it: float32 norms and an fma chain over the columns for q.x.
    Exact on integer-valued rows."""
    Q, X = np.asarray(Q, F32), np.asarray(X, F32)
    s = np.zeros((Q.shape[0], X.shape[0]), F32)
    for c in range(X.shape[1]):
        s = _fma32(np.broadcast_to(Q[:, c][:, None], s.shape), np.broadcast_to(X[:, c][None, :], s.shape), s)
    return ((norms(Q)[:, None] + norms(X)[None, :]).astype(F32) - F32(2) * s).astype(F32)


def dot_kp(n, k):
    return min(n, 32 * slots(k))


def dot_slices(nq, n, cand_slices):
    """knn_dot_slices: 0 asks for about 512 workgroups; every value is clipped to 32 and to the candidate tiles."""
    groups, tiles = -(-nq // kr.DOT_TQ), -(-n // kr.DOT_TC)
    s = cand_slices if cand_slices else 512 // groups
    return max(1, min(s, kr.KNN_MAX_SLICES, tiles))


def dot_workspace_bytes(nq, n, k, slices):
    """knn_dot_layout's total: the norms, the block maxima and their maximum, the slices' shortlists and partial means, each
    piece rounded up to 256 bytes."""
    def up(b):
        return (b + 255) // 256 * 256
    lists = slices * nq * dot_kp(n, k) * 4
    return up(n * 4) + up(nq * 4) + up(-(-n // kr.DOT_NORM_ROWS) * 4) + 256 + 2 * up(lists) + up(slices * nq * 4)


def shortlists(est, k, slices, self_first):
    """The slices' shortlists as the prefilter leaves them: (ld float32, lj int32, used bool), each [nq, slices, kp].  Slice s
    owns the candidate tiles [tiles s / slices, tiles (s + 1) / slices) of DOT_TC rows and lists its kp smallest candidates
    under (d~, j), the row itself at -inf under self_first; a slot past them holds (+inf, INT_MAX)."""
    est = np.asarray(est, F32)
    nq, n = est.shape
    kp = dot_kp(n, k)
    tiles = -(-n // kr.DOT_TC)
    ld = np.full((nq, slices, kp), np.inf, F32)
    lj = np.full((nq, slices, kp), kr.INT_MAX, np.int32)
    used = np.zeros((nq, slices, kp), bool)
    for s in range(slices):
        a, b = min(n, (tiles * s // slices) * kr.DOT_TC), min(n, (tiles * (s + 1) // slices) * kr.DOT_TC)
        j = np.arange(a, b)
        for i in range(nq):
            key = est[i, a:b].copy()
            if self_first and a <= i < b:
                key[i - a] = -np.inf
            order = np.lexsort((j, key))[:kp]
            m = order.shape[0]
            ld[i, s, :m], lj[i, s, :m], used[i, s, :m] = key[order], j[order], True
    return ld, lj, used


def rerank(X, k, ld, lj, queries=None, self_first=None, D32=None):
    """The model of knn_dot_rerank_kernel over given shortlists: (idx, dist, fallback) as `scheme` returns them.  The lists are
    merged with the rank search of knn_merge_kernel (the same code in both kernels); the first kp entries are the row's
    shortlist, a slot no entry ranked into holds no candidate; an entry outside 0 .. n - 1 makes the row fall back; the
    others are ranked by d2_f32 with every copy of a repeated index offered; then the certificate as in `scheme`."""
    X = np.asarray(X, F32)
    Q = X if queries is None else np.asarray(queries, F32)
    if self_first is None:
        self_first = queries is None
    nq, n, F = Q.shape[0], X.shape[0], X.shape[1]
    kp = ld.shape[2]
    if D32 is None:
        D32 = d2_f32(Q, X)
    E1, total = _bound(Q, X)
    idx = np.empty((nq, k), np.int32)
    dist = np.empty((nq, k), F32)
    fallback = np.zeros(nq, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(nq):
            rank = kr.merge_ranks(ld[i], lj[i])
            cd, cj = np.full(kp, np.nan, F32), np.full(kp, -1, np.int64)
            w = rank < kp
            cd[rank[w]], cj[rank[w]] = ld[i].reshape(-1)[w], lj[i].reshape(-1)[w]
            exact = D32[i].astype(np.float64)
            if self_first:
                exact[i] = -1.0
            ok = (cj >= 0) & (cj < n)
            short = cj[ok]
            pick = short[np.lexsort((short, exact[short]))[:k]]
            certified = bool(ok.all()) and pick.shape[0] == k
            if certified and n > kp:
                certified = bool(total[i] < F32(1e37)) and bool(exact[pick[-1]] < _lower(cd[kp - 1], E1[i], F))
            if not certified:
                fallback[i] = 1
                pick = _select(exact, k)
            idx[i] = pick
            dist[i] = np.maximum(D32[i, pick], 0)
    return idx, dist, fallback
