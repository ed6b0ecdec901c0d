"""The attention dropout's mask, restated in numpy from the published definition: test infrastructure only.

Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11; Random123): with M0 = 0xD2511F53, M1 = 0xCD9E8D57, ten times
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  (k0, k1) += (0x9E3779B9, 0xBB67AE85).
The mask of include/hg_aggr.h: keep[p, h] = philox(counter (p, h, sid_lo, sid_hi), key (key_lo, key_hi))[0] >= T,
T = floor(float32(p_drop) * 2^32).
"""
import ctypes

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

# Random123's known-answer vectors (counter, key, output)
KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32_10(counter, key):
    """The four output words for arrays (or scalars) of counter words c0..c3 and key words k0, k1: uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & np.uint64(MASK32) for c in counter)
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # < 2^64: no wrap
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & np.uint64(MASK32),
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & np.uint64(MASK32))
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return tuple(np.asarray(c).astype(np.uint32) for c in (c0, c1, c2, c3))


def threshold(p_drop):
    return int(np.floor(np.float64(np.float32(p_drop)) * 4294967296.0))


def scale(p_drop):
    """1 / (1 - p) as the library forms it: in float32."""
    return np.float32(1) / (np.float32(1) - np.float32(p_drop))


def keep(key, sid, p_drop, nnz, heads):
    """bool [nnz, heads]; key, sid: the two words of the state as unsigned 64-bit integers."""
    key, sid = int(key) & (2 ** 64 - 1), int(sid) & (2 ** 64 - 1)
    p, h = np.meshgrid(np.arange(nnz, dtype=np.uint64), np.arange(heads, dtype=np.uint64), indexing="ij")
    w = philox4x32_10((p, h, np.full_like(p, sid & MASK32), np.full_like(p, sid >> 32)), (key & MASK32, key >> 32))[0]
    return w.astype(np.uint64) >= np.uint64(threshold(p_drop))


def keep_host(key, sid, p_drop, nnz, heads):
    """The same from the library's own host statement (hg_dropout_keep_host): bool [nnz, heads]."""
    from hypergef_amd import _lib
    out = np.empty((nnz, heads), np.uint8)
    _lib.check(_lib.lib().hg_dropout_keep_host(int(key) & (2 ** 64 - 1), int(sid) & (2 ** 64 - 1), float(np.float32(p_drop)),
                                               nnz, heads, out.ctypes.data_as(ctypes.c_void_p)))
    return out.astype(bool)


def keep_of_state(rng_state, p_drop, nnz, heads):
    """keep_host for an int64 [2] state tensor as ops.incidence_softmax takes it."""
    key, sid = (int(x) for x in rng_state.cpu().tolist())
    return keep_host(key, sid, p_drop, nnz, heads)
