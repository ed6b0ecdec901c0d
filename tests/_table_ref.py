"""numpy references for the neighbour-table operators (include/hg_aggr.h, hg_table_*): test infrastructure, numpy only.

transpose: the stable argsort of the valid positions by vertex.  gather / gather_t: float32 loops in the contract's order
for rows one lane group sums (every row of gather; rows of gather_t up to HG_TABLE_SEQ_MAX entries).  gather_t_ordered:
gather_t with the longer rows in the pieces and the tree of the header's ORDER paragraph, written from that paragraph
alone, so float32 and bit for bit on every row; hub_table builds the tables that put such rows in every place of a
workgroup.  aggr / aggr_grad: the whole operator Y = degV . H_w (degE . (H_w^T X)) and its X-gradient in float64."""
import numpy as np

# (F, src and dst on 16-byte boundaries, P): the widths at which the long-row path takes another shape -- 64 lane groups a
# wave (F = 1; F = 4 aligned), P below its power of two (F = 3, 5, 12), the scalar columns of a width divisible by 4 on rows
# off a 16-byte boundary, and more than one column pass (F = 130; F = 260 aligned).  P is the header's 4 * (64 / L).
LONG_ROW_WIDTHS = ((1, True, 256), (3, True, 84), (4, True, 256), (4, False, 64), (5, True, 48), (12, True, 84),
                   (130, True, 4), (260, True, 4))


def transpose(idx, n=None):
    """(ptr_v [n + 1], pos_v [valid entries]) of a table idx [rows, k]: the positions p = i k + s with idx[p] == v, ascending,
    for v = 0 .. n - 1; entries outside 0 .. n - 1 are counted nowhere."""
    idx = np.asarray(idx)
    n = idx.shape[0] if n is None else n
    flat = idx.reshape(-1).astype(np.int64)
    valid = np.flatnonzero((flat >= 0) & (flat < n))
    order = valid[np.argsort(flat[valid], kind="stable")]
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, flat[valid] + 1, 1)
    return np.cumsum(ptr).astype(np.int32), order.astype(np.int32)


def transpose_loops(idx, n=None):
    """The definition written out: for every vertex, every position in ascending order."""
    idx = np.asarray(idx)
    n = idx.shape[0] if n is None else n
    flat = idx.reshape(-1)
    ptr, pos = [0], []
    for v in range(n):
        for p in range(flat.shape[0]):
            if flat[p] == v:
                pos.append(p)
        ptr.append(len(pos))
    return np.asarray(ptr, np.int32), np.asarray(pos, np.int32)


def _term(src, j, p, w, src_scale):
    t = src[j].astype(np.float32)
    if src_scale is not None:
        t = (t * np.float32(src_scale[j])).astype(np.float32)
    if w is not None:
        t = (t * np.float32(w[p])).astype(np.float32)
    return t


def gather(idx, src, w=None, src_scale=None, dst_scale=None):
    """dst[i] = dst_scale[i] * sum_s term(i k + s, idx[i, s]) in float32, ascending s, one rounded add a term."""
    idx = np.asarray(idx)
    rows, k = idx.shape
    n, F = src.shape
    out = np.zeros((rows, F), np.float32)
    for i in range(rows):
        acc = np.zeros(F, np.float32)
        for s in range(k):
            j = int(idx[i, s])
            if 0 <= j < n:
                acc = (acc + _term(src, j, i * k + s, w, src_scale)).astype(np.float32)
        if dst_scale is not None:
            acc = (np.float32(dst_scale[i]) * acc).astype(np.float32)
        out[i] = acc
    return out


def gather_t(ptr_v, pos_v, k, src, w=None, src_scale=None, dst_scale=None):
    """dst[v] = dst_scale[v] * sum_q term(pos_v[q], pos_v[q] // k) in float32, ascending q; an empty row is +0.0."""
    n = len(ptr_v) - 1
    F = src.shape[1]
    out = np.zeros((n, F), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in range(n):
            acc = np.zeros(F, np.float32)
            for q in range(int(ptr_v[v]), int(ptr_v[v + 1])):
                p = int(pos_v[q])
                acc = (acc + _term(src, p // k, p, w, src_scale)).astype(np.float32)
            if dst_scale is not None and ptr_v[v + 1] > ptr_v[v]:
                acc = (np.float32(dst_scale[v]) * acc).astype(np.float32)
            out[v] = acc
    return out


def long_row_shape(F, aligned16=True):
    """(c, L, R, P, P') of the header's ORDER paragraph: c columns a lane, L lanes a row, R = 64 // L rows a wave, P = 4 R
    pieces of a long row, P' the power of two at or above P."""
    c = 4 if F % 4 == 0 and aligned16 else 1
    L = min(-(-F // c), 64)
    R = 64 // L
    P = 4 * R
    P2 = 1
    while P2 < P:
        P2 *= 2
    return c, L, R, P, P2


def long_row_sum(terms, live, P, first_stride=None):
    """The sum of one long row in the header's order, float32 [F].  terms [len, F] float32 are the row's rounded terms in
    ascending q and live [len] says which entries count: the row is cut into P consecutive pieces of ceil(len / P) entries
    (the last ones may be short or empty), each summed in ascending q from +0.0 with one rounded add a term, and the P
    partial rows are added in the tree part[g] += part[g + s], s = P' / 2, P' / 4 .. 1, for g < s and g + s < P.
    first_stride: where the tree starts, P' / 2 unless a test wants to see that another tree gives other bits."""
    length, F = terms.shape
    chunk = -(-length // P)
    part = np.zeros((P, F), np.float32)
    for g in range(P):
        for q in range(min(g * chunk, length), min((g + 1) * chunk, length)):
            if live[q]:
                part[g] = (part[g] + terms[q]).astype(np.float32)
    P2 = 1
    while P2 < P:
        P2 *= 2
    s = P2 // 2 if first_stride is None else first_stride
    while s >= 1:
        for g in range(max(0, min(s, P - s))):  # g < s and g + s < P; a stride reads no row it writes
            part[g] = (part[g] + part[g + s]).astype(np.float32)
        s //= 2
    return part[0]


def gather_t_ordered(ptr_v, pos_v, k, src, w=None, src_scale=None, dst_scale=None, aligned16=True, seq_max=128):
    """gather_t with every row in the order include/hg_aggr.h documents, float32 [n, F]: a row of at most seq_max entries
    as gather_t sums it, a longer one as long_row_sum does with P = long_row_shape(F, aligned16)[3]; dst_scale once at the
    end.  aligned16: whether src and dst stand on 16-byte boundaries on the device (it picks c, and so P).
    An entry of pos_v outside 0 .. rows k - 1 is ignored the way the kernel ignores it: it keeps its place -- it counts in the
    row's length, which decides between the two orders and sets the pieces' size, and it occupies its slot of its piece --
    and adds nothing.  A row that holds only such entries is not empty: dst_scale is applied to its +0.0."""
    src = np.asarray(src, np.float32)
    rows, F = src.shape
    n = len(ptr_v) - 1
    P = long_row_shape(F, aligned16)[3]
    pos = np.asarray(pos_v).astype(np.int64)
    live_all = (pos >= 0) & (pos < rows * k)
    out = np.zeros((n, F), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in range(n):
            beg, end = int(ptr_v[v]), int(ptr_v[v + 1])
            live = live_all[beg:end]
            terms = np.zeros((end - beg, F), np.float32)
            for q in np.flatnonzero(live):
                p = int(pos[beg + q])
                terms[q] = _term(src, p // k, p, w, src_scale)
            if end - beg > seq_max:
                acc = long_row_sum(terms, live, P)
            else:
                acc = np.zeros(F, np.float32)
                for q in np.flatnonzero(live):
                    acc = (acc + terms[q]).astype(np.float32)
            if dst_scale is not None and end > beg:
                acc = (np.float32(dst_scale[v]) * acc).astype(np.float32)
            out[v] = acc
    return out


def hub_table(F, aligned16=True, seq_max=128, seed=0, lengths=None):
    """A table [rows, 2] over n vertices whose vertex rows reach every place of the long-row path at width F.  Slot 0 of
    every row names a hub, slot 1 a vertex that is no hub.  With R rows a wave (long_row_shape), n = max(8 R + 3, 43) is no
    multiple of the 4 R rows of a workgroup, and the hubs are the vertices {0, 1, R, 4 R - 1, 4 R, n - 1}: two lane groups
    of one wave, the next wave, the last row of workgroup 0, the first of workgroup 1, the last vertex of a partial tile.
    Their lengths cycle through `lengths` (seq_max + 1, seq_max + 2, 4 seq_max + 3, 1000).  Of the other vertices the first
    has exactly seq_max entries, the second none, the rest share what is left in turn (short rows); the rows are shuffled.
    Returns a dict: idx, n, hubs, lens, full, empty, and R, P of the width."""
    _, _, R, P, _ = long_row_shape(F, aligned16)
    rng = np.random.default_rng(seed)
    n = max(8 * R + 3, 43)
    assert n % (4 * R)
    hubs = sorted({0, 1, R, 4 * R - 1, 4 * R, n - 1})
    if lengths is None:
        lengths = (seq_max + 1, seq_max + 2, 4 * seq_max + 3, max(1000, 4 * seq_max + 7))
    lens = [lengths[i % len(lengths)] for i in range(len(hubs))]
    others = [v for v in range(n) if v not in hubs]
    full, empty, rest = others[0], others[1], others[2:]
    rows = sum(lens)
    slot0 = np.repeat(hubs, lens)
    slot1 = np.concatenate([np.full(seq_max, full), np.asarray(rest)[np.arange(rows - seq_max) % len(rest)]])
    assert -(-(rows - seq_max) // len(rest)) <= seq_max
    idx = np.stack([rng.permutation(slot0), rng.permutation(slot1)], axis=1).astype(np.int32)
    return dict(idx=idx, n=n, hubs=hubs, lens=lens, full=full, empty=empty, R=R, P=P)


def hub_operator_case(F, seq_max=128, seed=70):
    """hub_table(F) with what ops.knn_aggr takes: randn X and output gradient G [n, F], weights in [0.5, 1.5), degE = 1 / k
    and degV = in-degree^-1/2 (1 for a vertex with no entry), the scales of the kNN hypergraph."""
    t = hub_table(F, True, seq_max, seed)
    rng = np.random.default_rng(seed + F)
    idx, n = t["idx"], t["n"]
    rows, k = idx.shape
    deg = np.bincount(idx.reshape(-1), minlength=n).astype(np.float64)
    t.update(X=rng.standard_normal((n, F)).astype(np.float32), G=rng.standard_normal((n, F)).astype(np.float32),
             w=(rng.random(rows * k) + 0.5).astype(np.float32), degE=np.full(rows, 1.0 / k, np.float32),
             degV=np.where(deg > 0, np.maximum(deg, 1) ** -0.5, 1.0).astype(np.float32))
    return t


TABLE_TILE, TABLE_RADIX_BITS = 2048, 8  # csrc/hg_table.h: kTableTile = kTableBlock * kTableItems, kTableRadixBits


def radix_passes(n):
    """The passes of the transpose's sort: the keys 0 .. n (n itself: an ignored entry) have ceil(log2(n + 1)) bits."""
    bits = 0
    while (1 << bits) <= n:
        bits += 1
    return -(-bits // TABLE_RADIX_BITS)


def transpose_workspace_bytes(rows, k, n):
    """hg_table_transpose_workspace_bytes: the second position buffer rounded up to 256 bytes, then 256 counters a tile."""
    entries = rows * k
    return (entries * 4 + 255) // 256 * 256 + (1 << TABLE_RADIX_BITS) * -(-entries // TABLE_TILE) * 4


def _wrap32(a):
    return ((np.asarray(a, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def radix_model(idx, n, hist0=0, fill=0):
    """The transpose's sort as hg_table.hip runs it, with every tile counter starting at the int32 `hist0` instead of 0 and the
    position buffers holding `fill` before a pass writes them: per pass and per tile of TABLE_TILE positions a count of each
    digit, one exclusive scan over [digit, tile], and a stable scatter that drops what lands outside the buffer.  Returns the
    final positions int64 [rows k], or None where a pass read a position outside the table (the kernel would have read
    idx out of bounds).  hist0 = 0 is the stable sort by key."""
    flat = np.asarray(idx).reshape(-1).astype(np.int64)
    entries = flat.shape[0]
    key = np.where((flat >= 0) & (flat < n), flat, n)
    bins = 1 << TABLE_RADIX_BITS
    tiles = -(-entries // TABLE_TILE)
    order = np.arange(entries)
    for p in range(radix_passes(n)):
        if ((order < 0) | (order >= entries)).any():
            return None
        digit = (key[order] >> (p * TABLE_RADIX_BITS)) & (bins - 1)
        hist = np.full((bins, tiles), hist0, np.int64)
        for t in range(tiles):
            hist[:, t] += np.bincount(digit[t * TABLE_TILE:(t + 1) * TABLE_TILE], minlength=bins)
        hist = _wrap32(hist)
        start = _wrap32(np.concatenate([[0], np.cumsum(hist.reshape(-1))[:-1]])).reshape(bins, tiles)
        out = np.full(entries, fill, np.int64)
        for t in range(tiles):
            d = digit[t * TABLE_TILE:(t + 1) * TABLE_TILE]
            within = np.zeros(d.shape[0], np.int64)
            for b in np.unique(d):
                m = d == b
                within[m] = np.arange(int(m.sum()))
            at = _wrap32(start[d, t] + within)
            w = (at >= 0) & (at < entries)
            out[at[w]] = order[t * TABLE_TILE:(t + 1) * TABLE_TILE][w]
        order = out
    return order


def _dense64(idx, n, w):
    """H_w^T as a dense float64 [rows, n] matrix (duplicates within a row add up)."""
    idx = np.asarray(idx)
    rows, k = idx.shape
    Ht = np.zeros((rows, n), np.float64)
    wf = np.ones(rows * k) if w is None else np.asarray(w, np.float64).reshape(-1)
    for i in range(rows):
        for s in range(k):
            j = int(idx[i, s])
            if 0 <= j < n:
                Ht[i, j] += wf[i * k + s]
    return Ht


def _col64(t, count):
    return np.ones((count, 1)) if t is None else np.asarray(t, np.float64).reshape(count, 1)


def aggr(idx, X, w=None, degE=None, degV=None):
    """Y = degV . H_w (degE . (H_w^T X)) in float64."""
    n = X.shape[0]
    Ht = _dense64(idx, n, w)
    return _col64(degV, n) * (Ht.T @ (_col64(degE, Ht.shape[0]) * (Ht @ X.astype(np.float64))))


def aggr_grad(idx, dY, w=None, degE=None, degV=None):
    """dX of aggr for the output gradient dY, in float64: the operator is symmetric up to where the scales sit."""
    n = dY.shape[0]
    Ht = _dense64(idx, n, w)
    return Ht.T @ (_col64(degE, Ht.shape[0]) * (Ht @ (_col64(degV, n) * dY.astype(np.float64))))
