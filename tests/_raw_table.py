"""The C entries of the kNN search and the neighbour-table operators (include/hg_aggr.h) on caller-owned device tensors, and the
guarded, poisoned buffers the tests hand them.  Test infrastructure: ctypes over hypergef_amd._lib.lib(), nothing computed here.

hypergef_amd/knn_graph.py allocates every output and workspace itself; these wrappers take them from the caller, so that a
test can put each one between guard bands, fill it with a poison word, give the workspace exactly the queried size and start it
one word past a 256-byte boundary."""
import ctypes
import functools

import numpy as np
import torch

from hypergef_amd import _lib

GUARD = 64               # words of guard band before and after a view
GUARD_WORD = 0x5A5A5A5A  # no poison is this word
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _lib_checked():
    """The library with the argument types of the eight entries set (as _lib sets them; set here too so that this module
    does not depend on it)."""
    L = _lib.lib()
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_size_t
    for name, res, args in (
            ("hg_knn_workspace_bytes", sz, [i32] * 5),
            ("hg_knn_f32", ctypes.c_int, [vp, i32, vp, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
            ("hg_knn_dot_workspace_bytes", sz, [i32] * 5),
            ("hg_knn_dot_f32", ctypes.c_int, [vp, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
            ("hg_table_transpose_workspace_bytes", sz, [i32] * 3),
            ("hg_table_transpose", ctypes.c_int, [vp, i32, i32, i32, vp, vp, vp, sz, vp]),
            ("hg_table_gather_f32", ctypes.c_int, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
            ("hg_table_gather_t_f32", ctypes.c_int, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def signed(word):
    """The 32-bit word as the int32 torch fills with."""
    return word - (1 << 32) if word >= 1 << 31 else word


def guarded(nwords, poison_word, offset_words=0):
    """(buffer, view): an int32 view of `nwords` words filled with `poison_word`, GUARD words inside a buffer otherwise filled
    with GUARD_WORD, starting `offset_words` words past a 256-byte boundary."""
    assert poison_word != GUARD_WORD and 0 <= offset_words < 64
    buf = torch.full((GUARD + offset_words + nwords + GUARD,), signed(GUARD_WORD), dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 256 == 0
    view = buf[GUARD + offset_words:GUARD + offset_words + nwords]
    view.fill_(signed(poison_word))
    assert view.data_ptr() % 256 == 4 * offset_words and view.numel() == nwords
    return buf, view


def guards_intact(buf, view):
    start = (view.data_ptr() - buf.data_ptr()) // 4
    g = signed(GUARD_WORD)
    return bool((buf[:start] == g).all()) and bool((buf[start + view.numel():] == g).all())


def guarded_bytes(nbytes, poison_word, offset_words=0):
    """A workspace of exactly `nbytes` bytes (a multiple of 4, never rounded up); (None, None) for 0 bytes."""
    assert nbytes % 4 == 0
    return guarded(nbytes // 4, poison_word, offset_words) if nbytes else (None, None)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bytes(t):
    return 0 if t is None else t.numel() * t.element_size()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def knn_workspace_bytes(nq, n, F, k, cand_slices):
    return int(_lib_checked().hg_knn_workspace_bytes(nq, n, F, k, cand_slices))


def knn(Q, X, k, idx, dist, mean=None, seg=None, self_first=False, cand_slices=0, workspace=None):
    """hg_knn_f32.  Q, X: float32 [nq, F], [n, F] (the same tensor for Q == X); seg: host offsets or None."""
    seg_np = None if seg is None else np.ascontiguousarray(seg, np.int32)
    seg_ptr = None if seg_np is None else seg_np.ctypes.data_as(ctypes.c_void_p)
    with torch.cuda.device(DEV):
        _lib.check(_lib_checked().hg_knn_f32(_p(Q), Q.shape[0], _p(X), X.shape[0], X.shape[1], k, seg_ptr,
                                             0 if seg_np is None else seg_np.shape[0] - 1, 1 if self_first else 0, cand_slices,
                                             _p(idx), _p(dist), _p(mean), _p(workspace), _bytes(workspace), _stream()))


def knn_dot_workspace_bytes(nq, n, F, k, cand_slices):
    return int(_lib_checked().hg_knn_dot_workspace_bytes(nq, n, F, k, cand_slices))


def knn_dot(Q, X, k, idx, dist, mean=None, fallback=None, self_first=False, cand_slices=0, workspace=None):
    with torch.cuda.device(DEV):
        _lib.check(_lib_checked().hg_knn_dot_f32(_p(Q), Q.shape[0], _p(X), X.shape[0], X.shape[1], k, 1 if self_first else 0,
                                                 cand_slices, _p(idx), _p(dist), _p(mean), _p(fallback), _p(workspace),
                                                 _bytes(workspace), _stream()))


def transpose_workspace_bytes(rows, k, n):
    return int(_lib_checked().hg_table_transpose_workspace_bytes(rows, k, n))


def transpose(idx, n, ptr_v, pos_v, workspace):
    rows, k = idx.shape
    with torch.cuda.device(DEV):
        _lib.check(_lib_checked().hg_table_transpose(_p(idx), rows, k, n, _p(ptr_v), _p(pos_v), _p(workspace), _bytes(workspace),
                                                     _stream()))


def gather(idx, n, src, dst, w=None, src_scale=None, dst_scale=None):
    rows, k = idx.shape
    with torch.cuda.device(DEV):
        _lib.check(_lib_checked().hg_table_gather_f32(_p(idx), rows, k, n, src.shape[1], _p(src), _p(w), _p(src_scale),
                                                      _p(dst_scale), _p(dst), _stream()))


def gather_t(ptr_v, pos_v, k, src, dst, w=None, src_scale=None, dst_scale=None):
    rows, F = src.shape
    with torch.cuda.device(DEV):
        _lib.check(_lib_checked().hg_table_gather_t_f32(_p(ptr_v), _p(pos_v), rows, k, ptr_v.shape[0] - 1, F, _p(src), _p(w),
                                                        _p(src_scale), _p(dst_scale), _p(dst), _stream()))
