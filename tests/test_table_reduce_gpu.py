"""Max, min and mean over a kNN neighbour table (ops.knn_gather, hg_table_reduce_* / hg_table_select_*) against a brute-force
numpy loop: (dst, arg) and the gradient bit for bit on inputs where nearly every column ties, then the compositions."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _table_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
ROWS, N = 77, 53
WIDTHS = ((1, False), (4, False), (20, False), (260, False), (12, True))  # (F, rows off the 16-byte boundary: V = 1 at F % 4 == 0)
KS = (1, 3, 8, 9, 64)


def small_table(k, seed=1):
    """[ROWS, k] over N vertices with entries out of range, and: row 5 names vertex N - 1 alone and nobody else does (the -inf
    source either way, and a duplicated entry), row 7 alternates 3, 4 and rows 10, 11 alone name N - 2 (-0.0 before +0.0,
    hop 0 and hop 1), row 20 is out of range throughout and nobody names vertex N - 3."""
    rng = np.random.default_rng(seed + k)
    idx = rng.integers(0, N - 3, (ROWS, k))
    bad = rng.random(idx.shape)
    idx[bad < 0.08], idx[bad > 0.92] = -1, N
    idx[5], idx[7], idx[20] = N - 1, np.resize([3, 4], k), np.resize([-1, N], k)
    idx[10, 0] = idx[11, 0] = N - 2
    return idx.astype(np.int32), N


def table_of(name, F, view):
    if name == "hub":
        t = tr.hub_table(F, aligned16=not view)
        return t["idx"], t["n"]
    return small_table(name)


def source(nsrc, F, to, seed=2):
    """Integers in -3 .. 3, the -inf row and the two zeros of small_table's rows."""
    src = np.random.default_rng(seed + F).integers(-3, 4, (nsrc, F)).astype(np.float32)
    inf_row, neg0, pos0 = (nsrc - 1, 3, 4) if to == "hyperedge" else (5, 10, 11)
    src[inf_row], src[neg0, 0], src[pos0, 0] = -np.inf, -0.0, 0.0
    return src


def entries_of(idx, n, to):
    """Per destination row the valid (position, source row) pairs in ascending position; and the source row of every position."""
    rows, k = idx.shape
    flat = idx.reshape(-1).astype(np.int64)
    if to == "hyperedge":
        return [[(i * k + s, int(idx[i, s])) for s in range(k) if 0 <= idx[i, s] < n] for i in range(rows)], flat
    ptr, pos = tr.transpose(idx, n)
    return [[(int(p), int(p) // k) for p in pos[ptr[v]:ptr[v + 1]]] for v in range(n)], np.arange(rows * k) // k


def ref_reduce(entries, src, op):
    F = src.shape[1]
    val, arg = np.zeros((len(entries), F), np.float32), np.full((len(entries), F), -1, np.int32)
    for r, ent in enumerate(entries):
        for t, (p, j) in enumerate(ent):
            m = np.ones(F, bool) if t == 0 else (src[j] > val[r] if op == "max" else src[j] < val[r])  # strict: the first wins
            val[r], arg[r] = np.where(m, src[j], val[r]), np.where(m, p, arg[r])
    return val, arg


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def on_device(a, view=False):
    """The array on the GPU; view: as a contiguous view 4 bytes past a 16-byte boundary."""
    t = torch.from_numpy(a).cuda()
    if not view:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


def case(to, table, F, view):
    idx, n = table_of(table, F, view)
    src = source(n if to == "hyperedge" else idx.shape[0], F, to)
    entries, src_row = entries_of(idx, n, to)
    scale = (2.0 ** np.random.default_rng(3).integers(-2, 3, len(entries))).astype(np.float32)
    return idx, n, src, entries, src_row, scale


@pytest.mark.parametrize("op", ("max", "min"))
@pytest.mark.parametrize("to,table", [(to, t) for to in ("hyperedge", "vertex") for t in KS + (("hub",) if to == "vertex" else ())])
@pytest.mark.parametrize("F,view", WIDTHS)
def test_forward_bits(hg, op, to, table, F, view):
    idx, n, src, entries, _, scale = case(to, table, F, view)
    val, arg = ref_reduce(entries, src, op)
    assert (arg < 0).all(1).any() and (table == "hub" or np.isneginf(val).all(1).any())  # no candidate; -inf alone
    d_idx, d_src = torch.from_numpy(idx).cuda(), on_device(src, view)
    for sc in (None, scale):
        want = val if sc is None else val * sc[:, None]
        kw = dict(to=to, reduce=op, scale=None if sc is None else torch.from_numpy(sc).cuda(), num_nodes=n)
        dst, got = hg.ops.knn_gather(d_idx, d_src, return_index=True, **kw)
        assert np.array_equal(got.cpu().numpy(), arg)
        assert np.array_equal(bits(dst), want.view(np.int32))
        again = hg.ops.knn_gather(d_idx, d_src, return_index=True, **kw)
        assert torch.equal(again[1], got) and np.array_equal(bits(again[0]), bits(dst))
        assert np.array_equal(bits(hg.ops.knn_gather(d_idx, d_src, **kw)), bits(dst))  # the kernel without the position store


@pytest.mark.parametrize("op", ("max", "min"))
@pytest.mark.parametrize("to", ("hyperedge", "vertex"))
@pytest.mark.parametrize("table", (3, 9, "hub"))
@pytest.mark.parametrize("F", (4, 20))
def test_gradient_bits(hg, op, to, table, F):
    idx, n, src, entries, src_row, scale = case(to, table, F, False)
    _, arg = ref_reduce(entries, src, op)
    dY = np.random.default_rng(4).integers(-2, 3, arg.shape).astype(np.float32)
    dY[0, 0] = np.inf  # goes to one winner; a product with 0 in place of the select would spread NaN
    want = np.zeros(src.shape, np.float64)
    r, c = np.nonzero(arg >= 0)
    np.add.at(want, (src_row[arg[r, c]], c), dY[r, c].astype(np.float64) * scale[r])
    x = torch.from_numpy(src).cuda().requires_grad_(True)
    dst = hg.ops.knn_gather(torch.from_numpy(idx).cuda(), x, to=to, reduce=op, scale=torch.from_numpy(scale).cuda(), num_nodes=n)
    dst.backward(torch.from_numpy(dY).cuda())
    assert np.array_equal(bits(x.grad), want.astype(np.float32).view(np.int32))


def test_compositions(hg):
    ops = hg.ops
    idx, n = small_table(3)
    rng = np.random.default_rng(5)
    X = rng.integers(-3, 4, (n, 20)).astype(np.float32)
    degE, degV = ((2.0 ** rng.integers(-2, 3, c)).astype(np.float32) for c in (ROWS, n))
    d_idx, dE, dV = (torch.from_numpy(a).cuda() for a in (idx, degE, degV))
    # max into sum, exact on integers
    Xe = ref_reduce(entries_of(idx, n, "hyperedge")[0], X, "max")[0] * degE[:, None]
    want = np.stack([sum((Xe[j].astype(np.float64) for _, j in ent), np.zeros(20)) for ent in entries_of(idx, n, "vertex")[0]])
    got = ops.knn_aggr(d_idx, torch.from_numpy(X).cuda(), degE=dE, degV=dV, first="max", second="sum")
    assert np.array_equal(got.cpu().numpy(), (want * degV[:, None]).astype(np.float32))
    # the mean of either hop against float64
    for to, nsrc in (("hyperedge", n), ("vertex", ROWS)):
        src = rng.standard_normal((nsrc, 20)).astype(np.float32)
        ref = np.stack([sum((src[j].astype(np.float64) for _, j in ent), np.zeros(20)) / (3 if to == "hyperedge" else max(len(ent), 1))
                        for ent in entries_of(idx, n, to)[0]])  # a hyperedge's length is k, ignored entries included
        got = ops.knn_gather(d_idx, torch.from_numpy(src).cuda(), to=to, reduce="mean", num_nodes=n).cpu().numpy()
        assert (np.abs(got - ref) <= 1e-5 * np.maximum(1, np.abs(ref))).all()
    # the two sums are the call without the arguments
    Xd = torch.from_numpy(rng.standard_normal((n, 20)).astype(np.float32)).cuda()
    assert torch.equal(ops.knn_aggr(d_idx, Xd, degE=dE, degV=dV, first="sum", second="sum"), ops.knn_aggr(d_idx, Xd, degE=dE, degV=dV))


def test_layer_on_the_table_matches_the_planned_layer(hg):
    torch.manual_seed(6)
    host = hg.DynamicHypergraphConv(12, 32, k=10, first_aggr="max", second_aggr="mean").cuda()
    table = hg.DynamicHypergraphConv(12, 32, k=10, first_aggr="max", second_aggr="mean", device_graph=True).cuda()
    table.load_state_dict(host.state_dict())
    X0 = torch.randn(300, 12, device="cuda")
    G = torch.randn(300, 32, device="cuda")
    out = []
    for layer in (host, table):
        X = X0.clone().requires_grad_(True)
        Y = layer(X)
        Y.backward(G)
        out.append((Y.detach().double(), X.grad.double()))
    for ref, got in zip(*out):
        assert ((got - ref).abs() <= 1e-5 * ref.abs().clamp(min=1)).all()
