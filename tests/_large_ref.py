"""What test_large_offsets_gpu.py shares: the base hypergraph, its block-diagonal batch, guard-banded buffers and the choice
of the replicas that are checked.  Test infrastructure only.

The batch is K independent copies of one small hypergraph (synth.replicate_block_diagonal), so every copy is a problem of
its own: its slice of the inputs, the float64 reference of the operator's own _*_ref module on the base graph, and that
module's bound.  An offset computed in 32 bits reads or writes another copy's rows; the copies hold independent random
values, so such an error is of the size of the values themselves.
"""
import numpy as np
import torch

import _grad_ref as gr
from hypergef_amd import synth

DEV = "cuda:0"
E31 = 2 ** 31          # the element threshold `E`; in bytes the threshold `B`
SENTINEL = -12288.0    # what every output is prefilled with (exact in bf16 too): no sum of the random inputs gives it
ARG_SENTINEL = -7      # the same for int32 positions (a valid one is >= -1)
GUARD = 4096           # elements of the band on either side of an output (16 KiB of fp32: keeps 16-byte alignment)

N0, M0 = 2050, 2061    # no powers of two: the element 2^31 falls inside a replica, not between two
LONG = 700             # one hyperedge of LONG members, one vertex in LONG hyperedges: beyond split_len = 512 and kSegLong
MID = 100              # one row of MID entries per side: beyond short_max = 32, a wave task that owns its whole row
EMPTY, BIG, HUB, ISOLATED, MID_EDGE, MID_VERTEX = 5, 11, 7, N0 - 1, 13, 9


def base():
    """The base incidence: ragged short hyperedges (1 .. 40 members), hyperedge BIG of LONG members, vertex HUB in LONG
    hyperedges, MID_EDGE and MID_VERTEX with MID entries, hyperedge EMPTY without members (degE = inf) and vertex ISOLATED
    in none."""
    rng = np.random.default_rng(2031)
    sizes = np.minimum(rng.geometric(1.0 / 3.2, M0), 40)
    sizes[EMPTY], sizes[BIG], sizes[MID_EDGE] = 0, LONG, MID
    member = {}
    for v, count in ((HUB, LONG), (MID_VERTEX, MID)):
        member[v] = np.zeros(M0, bool)
        member[v][rng.choice(np.setdiff1d(np.arange(M0), [EMPTY]), count, replace=False)] = True
    rows = []
    for e in range(M0):
        mem = rng.choice(N0 - 1, int(sizes[e]), replace=False)  # never ISOLATED = N0 - 1
        mem = mem[(mem != HUB) & (mem != MID_VERTEX)]
        rows.append(np.sort(np.concatenate([mem, [v for v in member if member[v][e]]]).astype(np.int64)))
    rows[EMPTY] = np.zeros(0, np.int64)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return synth.Incidence(N0, M0, ptr.astype(np.int32), np.concatenate(rows).astype(np.int32), name="large-base")


def replicas_for(one):
    """K such that [N, 512] and [M, 512] reach 2^31 elements and [nnz, 128] does too, with some forty replicas beyond the
    one in which that element falls (so the straddling replica is not the last)."""
    need = max(-(-E31 // (512 * one.N)), -(-E31 // (512 * one.M)), -(-E31 // (128 * one.nnz)))
    return need + 40


def picked(K, per_replica, threshold=E31):
    """The replicas a test checks: the first, the middle, the one in which element (or byte) `threshold` of an array of
    `per_replica` elements (bytes) a replica falls, and the last."""
    r = threshold // per_replica
    assert 0 < r < K - 1, (r, K)
    return sorted({0, K // 2, r, K - 1})


class Guarded:
    """A contiguous output of `shape` inside one allocation, a band of GUARD elements of `fill` on either side of it."""

    def __init__(self, shape, dtype=torch.float32, fill=SENTINEL):
        self.n = int(np.prod(shape))
        self.fill = fill
        self.buf = torch.full((self.n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)

    def refill(self):
        self.t.fill_(self.fill)

    def check(self, what, written=True):
        """The bands are intact and (written) no element of the output still holds the fill: both decided on the device
        over the whole array."""
        assert bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all()), \
            "guard band overwritten: " + what
        if written:
            assert not bool((self.t == self.fill).any()), "an element was not written: " + what


class Batch:
    """The batch on the device: the plan over K replicas of base(), the scale vectors (independent per replica) and the
    views a test needs of one replica."""

    def __init__(self):
        from hypergef_amd.plan import Plan
        self.one = one = base()
        self.K = K = replicas_for(one)
        self.inc = inc = synth.replicate_block_diagonal(one, K)
        self.N, self.M, self.nnz = inc.N, inc.M, inc.nnz
        self.ptr = torch.from_numpy(inc.csrptr).to(DEV)
        self.ind = torch.from_numpy(inc.colind).to(DEV)
        self.plan = Plan.from_tensors(inc.N, self.ptr, self.ind)
        sizes = np.diff(one.csrptr).astype(np.float32)
        with np.errstate(divide="ignore"):
            self.degE = torch.from_numpy(np.tile(np.float32(1) / sizes, K)).to(DEV)  # inf on the empty hyperedges
        g = torch.Generator(device=DEV).manual_seed(31)
        self.degV = torch.rand(inc.N, device=DEV, generator=g) + 0.5
        self.W = torch.rand(inc.M, device=DEV, generator=g) + 0.5
        self.L = {"hyperedge": int(sizes.max()), "vertex": int(np.bincount(one.colind, minlength=one.N).max())}
        self.index = gr.Graph(one)  # V, E alone: the softmax and dot references

    def rows(self, r, side):
        """Replica r's rows of an [N, .] (side 'vertex' / 1) or [M, .] ('hyperedge' / 0) array, or its H_T positions
        ('nnz')."""
        n = {"vertex": self.one.N, 1: self.one.N, "hyperedge": self.one.M, 0: self.one.M, "nnz": self.one.nnz}[side]
        return slice(r * n, (r + 1) * n)

    def graph(self, r, scales=True):
        """Replica r as a _grad_ref.Graph with its own degE, degV, W."""
        if not scales:
            return self.index
        return gr.Graph(self.one, self.degE[self.rows(r, 0)], self.degV[self.rows(r, 1)], self.W[self.rows(r, 0)])


def randn(*shape, seed, dtype=torch.float32):
    """Independent normal values over the whole array, drawn on the device: no two replicas share a row."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g, dtype=dtype)


def rand_weights(*shape, seed):
    """Incidence weights in [0.25, 1.25)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(*shape, device=DEV, generator=g).add_(0.25)


def scores(*shape, seed):
    """Attention scores with |s| <= 2: |sv + se| <= 4 (and <= 6 with an entry logit), inside the bound's Smax = 8."""
    return randn(*shape, seed=seed).mul_(0.5).clamp_(-2.0, 2.0)
