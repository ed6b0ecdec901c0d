"""Plan objects: this backend's schedule for one hypergraph (include/hg_aggr.h).

The plan plays the role the reference's `group_key/group_row/group_start/
group_end` tensors play for its kernels (HyperGsys/hypergraph.py:96-101): it is
built once per hypergraph from `H_T_csrptr` / `H_T_colind` and reused by every
aggregation call.  The reference operators receive those two tensors on every
call, so a small cache keyed on them keeps the call signature unchanged.
"""
import collections
import ctypes
import threading

import numpy as np
import torch

from . import _lib


_CACHE_LOCK = threading.Lock()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream_handle(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def make_opts(short_max=0, split_len=0, panel_rows=0, panel_nnz=0, xcd_remap=True, host_only=False,
              t_big=0, fused_tile_bytes=0, dfs_order=False, hub_pass=True, fused_steps=0,
              row_stream=True):
    flags = 0
    if dfs_order:
        flags |= _lib.HG_PLAN_DFS_ORDER
    if not hub_pass:
        flags |= _lib.HG_PLAN_NO_HUB_PASS
    if not row_stream:
        flags |= _lib.HG_PLAN_NO_ROW_STREAM
    if host_only:
        flags |= _lib.HG_PLAN_HOST_ONLY
    if not xcd_remap:
        flags |= _lib.HG_PLAN_NO_XCD_REMAP
    return _lib.PlanOpts(short_max, split_len, panel_rows, panel_nnz, flags, t_big, fused_tile_bytes, fused_steps)


class Plan:
    """Owns an `hg_plan*`."""

    def __init__(self, handle, device=None):
        self._h = handle
        self.device = device
        info = _lib.PlanInfo()
        _lib.check(_lib.lib().hg_plan_get_info(self._h, ctypes.byref(info)))
        self.info = info.as_dict()
        self.N, self.M, self.nnz = info.N, info.M, info.nnz
        self._nonempty = None  # nonempty_edges' mask

    @classmethod
    def from_host(cls, N, M, csrptr_t, colind_t, opts=None, device=None):
        """csrptr_t / colind_t: host int32 arrays of H_T.  With a host-only
        `opts` nothing touches the GPU (used by the CPU tests)."""
        csrptr_t = np.ascontiguousarray(csrptr_t, dtype=np.int32)
        colind_t = np.ascontiguousarray(colind_t, dtype=np.int32)
        if csrptr_t.shape[0] != M + 1:
            raise ValueError("csrptr_t must have M + 1 entries")
        if int(csrptr_t[-1]) != colind_t.shape[0]:
            raise ValueError("csrptr_t[M] must equal len(colind_t)")
        h = ctypes.c_void_p()
        ctx = torch.cuda.device(device) if device is not None else _NullCtx()
        with ctx:
            _lib.check(_lib.lib().hg_plan_create_host(
                ctypes.byref(h), N, M, csrptr_t.ctypes.data_as(ctypes.c_void_p),
                colind_t.ctypes.data_as(ctypes.c_void_p),
                ctypes.byref(opts) if opts is not None else None))
        return cls(h, device)

    @classmethod
    def from_tensors(cls, N, csrptr_t, colind_t, opts=None):
        """csrptr_t / colind_t: int32 device tensors (the reference's
        `hyperg.H_T_csrptr` / `hyperg.H_T_colind`)."""
        _check_index(csrptr_t, "csrptr_t")
        _check_index(colind_t, "indices_t")
        M = csrptr_t.numel() - 1
        h = ctypes.c_void_p()
        with torch.cuda.device(csrptr_t.device):
            _lib.check(_lib.lib().hg_plan_create_device(
                ctypes.byref(h), N, M, colind_t.numel(), _ptr(csrptr_t), _ptr(colind_t),
                ctypes.byref(opts) if opts is not None else None, _stream_handle(csrptr_t.device)))
        return cls(h, csrptr_t.device)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().hg_plan_destroy(h)
            except Exception:
                pass

    def vertex_csr(self):
        """Host copy of the derived H CSR: (ptr_v [N+1], ind_v [nnz])."""
        ptr_v = np.empty(self.N + 1, np.int32)
        ind_v = np.empty(self.nnz, np.int32)
        _lib.check(_lib.lib().hg_plan_get_vertex_csr(
            self._h, ptr_v.ctypes.data_as(ctypes.c_void_p), ind_v.ctypes.data_as(ctypes.c_void_p)))
        return ptr_v, ind_v

    def schedule(self, hop):
        """Host copy of hop's schedule: dict of int32 [n,4] arrays (see hg_aggr.h)."""
        out = {k: np.zeros((self.info[k][hop], 4), np.int32) for k in ("panels", "tasks", "fixups")}
        _lib.check(_lib.lib().hg_plan_get_schedule(
            self._h, hop, *(out[k].ctypes.data_as(ctypes.c_void_p) for k in ("panels", "tasks", "fixups"))))
        return out

    def prepare(self, F):
        """Build the feature-width dependent (fused) schedule now; returns its shape."""
        info = _lib.FusedInfo()
        _lib.check(_lib.lib().hg_plan_prepare(self._h, F, ctypes.byref(info)))
        self._drop_ws_cache(F)
        return info.as_dict()

    def auto_variant(self, F):
        """Name of the kernel family `variant="auto"` runs for feature width F."""
        v = _lib.lib().hg_plan_auto_variant(self._h, F)
        if v < 0:
            _lib.check(v)
        return {code: name for name, code in _lib.VARIANTS.items()}[v]

    def tune(self, csrptr_t, colind_t, X, degE=None, degV=None, W=None, iters=20, out=None):
        """Timed choice of what variant="auto" runs for X's width (hg_plan_tune_f32): the fused schedule and the
        pull variant with each of its kernels per hop (three on launch-bound graphs) are run `iters` times each on these tensors and the fastest is
        pinned -- the counterpart of the reference's tuner (HyperGAggr_tune, hgnnAgg.cuh:1115-1157), worth calling
        for a single dataset-sized hypergraph.  Returns {"variant", "pull_hop_kernels", "us": {...}}; `pin` takes the first
        two.  out ([N, F] float32, optional) receives what the winner computed, the result the call leaves behind."""
        _check_feat(X, "node_feat")
        F = X.shape[1]
        self.prepare(F)
        flat = lambda t: None if t is None else t.reshape(-1)
        degE, degV, W = flat(degE), flat(degV), flat(W)
        if out is not None:
            _check_feat(out, "out", device=X.device)
            if tuple(out.shape) != (self.N, F):
                raise ValueError("out must be [%d, %d]" % (self.N, F))
        Y = out if out is not None else torch.empty((self.N, F), dtype=torch.float32, device=X.device)
        workspace, nbytes = self._workspace(F, X.device)
        info = _lib.TuneInfo()
        with torch.cuda.device(X.device):
            _lib.check(_lib.lib().hg_plan_tune_f32(
                self._h, F, _ptr(csrptr_t), _ptr(colind_t), _ptr(X), _ptr(degE), _ptr(degV), _ptr(W), _ptr(Y),
                _ptr(workspace), nbytes, int(iters), _stream_handle(X.device), ctypes.byref(info)))
        if hasattr(self, "_auto"):
            self._auto.pop(F, None)  # the cached answer of auto_variant may have changed
        self._drop_ws_cache(F)
        names ={code: name for name, code in _lib.VARIANTS.items()}
        kinds = ("stream", "panels", "tasks")  # per hop: streaming row gather, row panels + wave tasks, latency schedule
        labels = ("fused", "pull") + tuple("pull/%s+%s" % (kinds[c % 3], kinds[c // 3]) for c in range(1, 9))
        return {"variant": names[info.variant], "pull_hop_kernels": info.pull_hop_kernels,
                "us": {l: float(u) for l, u in zip(labels, info.us) if u >= 0}}

    def pin(self, F, variant, pull_hop_kernels=0):
        """Set what variant="auto" runs for feature width F, and the kernel of each pull hop, without timing anything
        (hg_plan_set_choice): variant 'fused' or 'pull', pull_hop_kernels = k0 + 3 * k1 with k = 0 streaming row gather,
        1 row panels + wave tasks, 2 the latency schedule (has_latency_schedule()) -- the two values `tune` returns, so
        plan.pin(F, **{k: tuned[k] for k in ("variant", "pull_hop_kernels")}) repeats a tuned choice and its bits.
        A forced variant="pull", gather_rows and the bf16 call use the pinned hop kernels too.  'auto' removes the pin
        (see unpin).  Launches and allocates nothing; works on host-only plans."""
        if variant not in _lib.VARIANTS:
            raise ValueError("variant must be one of %s, got %r" % (sorted(_lib.VARIANTS), variant))
        _lib.check(_lib.lib().hg_plan_set_choice(self._h, int(F), _lib.VARIANTS[variant], int(pull_hop_kernels)))
        if hasattr(self, "_auto"):
            self._auto.pop(F, None)  # the cached answer of auto_variant may have changed
        self._drop_ws_cache(F)

    def unpin(self, F):
        """Remove width F's pinned or tuned choice: the static rule decides again, and the pull hops run their default
        kernel."""
        self.pin(F, "auto")

    def has_latency_schedule(self):
        """Whether the plan carries the latency schedule hop kernel 2 runs on (hg_plan_has_latency_schedule): graphs of
        at most 2^18 incidences whose short_max is above the latency cut."""
        v = _lib.lib().hg_plan_has_latency_schedule(self._h)
        if v < 0:
            _lib.check(v)
        return bool(v)

    def _ensure_fused(self, F):
        if not hasattr(self, "_prepared"):
            self._prepared = set()
        if F not in self._prepared:
            self.prepare(F)
            self._prepared.add(F)

    def workspace_bytes(self, F):
        # cached per width: asking costs a library call per aggregation otherwise; prepare / tune, which can build a
        # larger layout for the width, drop the entry
        cache = self.__dict__.setdefault("_ws_bytes", {})
        n = cache.get(F)
        if n is None:
            n = cache[F] = int(_lib.lib().hg_plan_workspace_bytes(self._h, F))
        return n

    def linear_workspace_bytes(self, F_in):
        """hg_aggr_linear_workspace_bytes, cached per width like workspace_bytes (the query runs the AUTO rule under the
        plan's locks and may build a schedule: not something to pay per launch-bound layer call)."""
        cache = self.__dict__.setdefault("_ws_bytes", {})
        n = cache.get(("lin", F_in))
        if n is None:
            n = cache[("lin", F_in)] = int(_lib.lib().hg_aggr_linear_workspace_bytes(self._h, F_in))
        return n

    def _workspace(self, F, device):
        nbytes = self.workspace_bytes(F)
        # torch's caching allocator returns 512-byte aligned blocks and is stream-ordered
        return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device), nbytes

    def _drop_ws_cache(self, F):
        """Forget width F's cached workspace sizes: something may have built a larger layout for it."""
        for k in (F, ("lin", F)):
            self.__dict__.setdefault("_ws_bytes", {}).pop(k, None)

    def _run_with_workspace(self, entry, head, tail, F, workspace, device, size):
        """Call entry(*head, workspace, bytes, *tail) on the caller's workspace, or on an own one of size(F) bytes
        (workspace_bytes or linear_workspace_bytes, both cached), and raise on a bad status.  HG_ERR_WORKSPACE on an own
        one means the cached size is stale: the call itself built a layout for this width that needs more (e.g. AUTO on an
        unaligned view of X with N >= 2^24 takes another schedule than the one the size was asked for).  Nothing was
        written; ask again and retry once.  No closure and no tensor method on the own path: this runs once per
        launch-bound call."""
        own = workspace is None
        if own:
            nbytes = size(F)
            workspace = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        else:
            nbytes = workspace.numel() * workspace.element_size()
        st = entry(*head, _ptr(workspace), nbytes, *tail)
        if st == _lib.HG_ERR_WORKSPACE and own:
            self._drop_ws_cache(F)
            nbytes = size(F)
            workspace = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
            st = entry(*head, _ptr(workspace), nbytes, *tail)
        _lib.check(st)

    def aggregate(self, csrptr_t, colind_t, X, degE=None, degV=None, W=None, variant="auto",
                  out=None, workspace=None, bind_scales=True, trainable_scales=False):
        """Y = degV . H (degE . W . (H^T X)) on X's device, current stream.
        bind_scales: see _bind_scales; pass False for scale vectors whose contents change
        without torch noticing (numpy / DLPack aliases, `.data` writes, other libraries).
        X may be float32 or bfloat16; Y has X's dtype (so must `out`).  The scale vectors are float32 either way.  A bf16
        call (hg_aggr_fused_bf16) accumulates in fp32 in the fp32 call's order and rounds once: for F % 4 == 0 its result
        equals aggregate(X.float(), ...).to(torch.bfloat16) bit for bit.  bf16 rows of other widths are padded with zero
        columns to the next multiple of 4 and the result sliced back -- that path copies X and Y, and runs at the padded
        width F4: a caller's workspace is used there if it holds workspace_bytes(F4), else the call takes its own.  A
        bf16 X or out whose data is not 8-byte aligned is copied too.
        trainable_scales: one of the scale vectors is being trained although the tensor passed does not say so (a view made
        with grad mode off, as inside an autograd Function): the set is treated as one that requires a gradient -- never
        bound, W not tested for all ones."""
        bf16 = isinstance(X, torch.Tensor) and X.dtype == torch.bfloat16
        _check_feat(X, "node_feat", bf16_ok=True)
        if X.shape[0] != self.N:
            raise ValueError("node_feat has %d rows, hypergraph has %d vertices" % (X.shape[0], self.N))
        F = X.shape[1]
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != X.dtype):
            raise TypeError("out must have node_feat's dtype %s, got %s" % (X.dtype, getattr(out, "dtype", type(out))))
        if bf16 and (F % 4 != 0 or X.data_ptr() % 8 != 0 or (out is not None and out.data_ptr() % 8 != 0)):
            # hg_aggr_fused_bf16 takes whole four-column lanes at 8-byte alignment: pad / copy, aggregate, slice back
            F4 = (F + 3) // 4 * 4
            if F4 == F:
                Xp = X if X.data_ptr() % 8 == 0 else X.clone()
            else:
                Xp = torch.zeros((self.N, F4), dtype=X.dtype, device=X.device)
                Xp[:, :F] = X
            if workspace is not None and workspace.numel() * workspace.element_size() < self.workspace_bytes(F4):
                workspace = None  # sized for F, not for the padded width: this path copies anyway, take an own one
            Yp = self.aggregate(csrptr_t, colind_t, Xp, degE, degV, W, variant, None, workspace, bind_scales,
                                trainable_scales)
            if out is None:
                return Yp[:, :F].contiguous() if F4 != F else Yp
            out.copy_(Yp[:, :F])
            return out
        _check_scales((("degE", degE, self.M), ("degV", degV, self.N), ("W", W, self.M)), X.device)
        W = self._drop_unit_weights(W, bind_scales and not trainable_scales)
        stream = torch.cuda.current_stream(X.device)  # looked up once per call: it is a measurable share of a launch-bound call
        if (degE is not None or degV is not None or W is not None) and variant in ("auto", "fused"):
            self._bind_scales(F, degE, degV, W, X.device, bind_scales, stream, trainable_scales)
        Y = out if out is not None else torch.empty((self.N, F), dtype=X.dtype, device=X.device)
        if variant == "fused":  # hg_plan_workspace_bytes sizes for what AUTO runs; a forced fused call needs its schedule first
            self._ensure_fused(F)
        with torch.cuda.device(X.device):
            args = (self._h, F, _ptr(csrptr_t), _ptr(colind_t), _ptr(X), _ptr(degE), _ptr(degV), _ptr(W), _ptr(Y))
            entry = _lib.lib().hg_aggr_fused_bf16 if bf16 else _lib.lib().hg_aggr_fused_f32
            self._run_with_workspace(entry, args, (_lib.VARIANTS[variant], ctypes.c_void_p(stream.cuda_stream)), F, workspace,
                                     X.device, self.workspace_bytes)
        return Y

    def aggregate_linear(self, csrptr_t, colind_t, X, weight, degE=None, degV=None, W=None,
                         variant="auto", out=None, workspace=None, packed=None, residual=None, ca=1.0,
                         cb=0.0, relu=False, t_out=None, bind_scales=True, math="f32", trainable_scales=False):
        """Y[N, F_out] = Aggr(X) . weight^T in one pass (hg_aggr_linear_f32); weight = nn.Linear.weight,
        [F_out, F_in]; packed = pack_linear(weight) if the caller keeps it across calls.
        With residual / ca / cb / relu / t_out: Y = act((ca * Aggr(X) + cb * residual) . weight^T) and
        t_out receives the bracket (hg_aggr_linear_res_f32: one UniGCNII / UniGIN layer per pass).  cb may be a
        one-element float32 device tensor (a learned scalar such as UniGIN's 1 + eps): the kernel then reads it from
        device memory (hg_aggr_linear_res_dev_f32) -- no read-back to the host, and a captured hipGraph sees its updates.
        math = 'bf16x6': at F_in = 128 the fused panels' matrix phase computes each fp32 product as six bf16 products
        (HG_LIN_BF16X6, include/hg_aggr.h: fp32-equivalent error, 3/8 of the matrix-pipe cycles); 'f32': fp32 MFMA.
        Raises HgError(unsupported) for widths the MFMA epilogue does not take."""
        _check_feat(X, "node_feat")
        _check_feat(weight, "weight", device=X.device)
        if X.shape[0] != self.N:
            raise ValueError("node_feat has %d rows, hypergraph has %d vertices" % (X.shape[0], self.N))
        F_in = X.shape[1]
        if weight.dim() != 2 or weight.shape[1] != F_in:
            raise ValueError("weight must be [F_out, F_in = %d]" % F_in)
        F_out = weight.shape[0]
        if packed is None:
            packed = packed_linear_cached(weight, math == "bf16x6")
        elif packed.numel() not in (weight.numel(), _lib.lib().hg_linear_pack_floats(F_out, F_in, LIN_BF16X6)):
            raise ValueError("packed does not belong to this weight")
        if math not in ("f32", "bf16x6"):
            raise ValueError("math must be 'f32' or 'bf16x6', got %r" % (math,))
        flags = (LIN_RELU if relu else 0)
        if math == "bf16x6" and F_in == 128 and packed.numel() == _lib.lib().hg_linear_pack_floats(F_out, F_in, LIN_BF16X6):
            flags |= LIN_BF16X6
        weight = packed
        _check_scales((("degE", degE, self.M), ("degV", degV, self.N), ("W", W, self.M)), X.device)
        W = self._drop_unit_weights(W, bind_scales and not trainable_scales)  # trainable_scales: as in aggregate()
        if (degE is not None or degV is not None or W is not None) and variant in ("auto", "fused"):
            self._bind_scales(F_in, degE, degV, W, X.device, bind_scales, trainable=trainable_scales)
        Y = out if out is not None else torch.empty((self.N, F_out), dtype=torch.float32, device=X.device)
        if variant == "fused":
            self._ensure_fused(F_in)
        with torch.cuda.device(X.device):
            for name, t in (("residual", residual), ("t_out", t_out)):
                if t is not None:
                    _check_feat(t, name, device=X.device)
                    if tuple(t.shape) != (self.N, F_in):
                        raise ValueError("%s must be [N, F_in]" % name)
            if isinstance(cb, torch.Tensor):
                _check_feat(cb, "cb", device=X.device)
                if cb.numel() != 1:
                    raise ValueError("a tensor cb must hold one element")
                fn, cb_arg = _lib.lib().hg_aggr_linear_res_dev_f32, _ptr(cb)
            else:
                fn, cb_arg = _lib.lib().hg_aggr_linear_res_f32, float(cb)
            head = (self._h, F_in, F_out, _ptr(csrptr_t), _ptr(colind_t), _ptr(X), _ptr(degE), _ptr(degV),
                    _ptr(W), _ptr(weight), _ptr(residual), float(ca), cb_arg, flags, _ptr(t_out), _ptr(Y))
            self._run_with_workspace(fn, head, (_lib.VARIANTS[variant], _stream_handle(X.device)), F_in, workspace, X.device,
                                     self.linear_workspace_bytes)
        return Y

    def linear_bf16_path(self, F_in, F_out, variant="auto"):
        """hg_aggr_linear_bf16_path: which kernels aggregate_linear_bf16 runs for these widths, as a bit mask -- 1: the
        fused panels run the bf16 epilogue themselves, 2: some or all rows go through the bf16 rows kernel."""
        v = _lib.lib().hg_aggr_linear_bf16_path(self._h, F_in, F_out, _lib.VARIANTS[variant])
        if v < 0:
            _lib.check(v)
        return v

    def aggregate_linear_bf16(self, csrptr_t, colind_t, X, weight, degE=None, degV=None, W=None,
                              variant="auto", out=None, workspace=None, packed=None, residual=None, ca=1.0,
                              cb=0.0, relu=False, t_out=None, bind_scales=True, trainable_scales=False):
        """aggregate_linear on bfloat16 rows with the linear on the bf16 MFMA (hg_aggr_linear_res_bf16): X, weight,
        residual, t_out and the result are bfloat16, degE / degV / W float32, accumulation fp32.  t_out receives
        (ca * Aggr(X) + cb * residual) of the fp32 call on the widened operands, rounded to bf16 once -- bit for bit
        aggregate_linear(X.float(), ..., t_out=).to(bfloat16) -- and Y = round_bf16(act(t_out . weight^T)) (include/hg_aggr.h).
        (Both calls must run the same pull hop kernels for that: X.float() beyond 2^31 bytes leaves the streaming row gather
        while a bfloat16 X of half the size stays on it, and a long hyperedge is then summed in another order; pin them.)
        cb may be a one-element float32 device tensor.  packed = pack_linear_bf16(weight) if the caller keeps it.
        Dtypes and shapes are refused (TypeError, ValueError) before any device is touched."""
        for name, t in (("node_feat", X), ("weight", weight), ("residual", residual), ("t_out", t_out), ("out", out)):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16):
                raise TypeError("%s must be a bfloat16 tensor, got %s" % (name, getattr(t, "dtype", type(t))))
        if isinstance(cb, torch.Tensor) and cb.dtype != torch.float32:
            raise TypeError("a tensor cb must be float32, got %s" % cb.dtype)
        if X.dim() != 2 or X.shape[0] != self.N:
            raise ValueError("node_feat must be [N = %d, F_in], got %s" % (self.N, tuple(X.shape)))
        F_in = X.shape[1]
        if weight.dim() != 2 or weight.shape[1] != F_in:
            raise ValueError("weight must be [F_out, F_in = %d]" % F_in)
        F_out = weight.shape[0]
        if not linear_supported(F_in, F_out):
            raise ValueError("aggregate_linear_bf16 takes F_in in {32, 64, 128} and F_out a positive multiple of 16, got %d -> %d"
                             % (F_in, F_out))
        for name, t in (("residual", residual), ("t_out", t_out)):
            if t is not None and tuple(t.shape) != (self.N, F_in):
                raise ValueError("%s must be [N, F_in]" % name)
        if out is not None and tuple(out.shape) != (self.N, F_out):
            raise ValueError("out must be [N, F_out]")
        if isinstance(cb, torch.Tensor) and cb.numel() != 1:
            raise ValueError("a tensor cb must hold one element")
        if packed is not None and packed.numel() * packed.element_size() != 2 * F_out * F_in:
            raise ValueError("packed does not belong to this weight")
        _check_feat(X, "node_feat", bf16_ok=True)
        for name, t in (("weight", weight), ("residual", residual), ("t_out", t_out), ("out", out)):
            if t is not None:
                _check_feat(t, name, device=X.device, bf16_ok=True)
        _check_scales((("degE", degE, self.M), ("degV", degV, self.N), ("W", W, self.M)), X.device)
        if X.data_ptr() % 8 != 0:  # the entry takes 8-byte aligned rows (torch's own allocations are; views need not be)
            X = X.clone()
        if residual is not None and residual.data_ptr() % 8 != 0:
            residual = residual.clone()
        if packed is None:
            packed = packed_linear_bf16_cached(weight)
        W = self._drop_unit_weights(W, bind_scales and not trainable_scales)
        if (degE is not None or degV is not None or W is not None) and variant in ("auto", "fused"):
            self._bind_scales(F_in, degE, degV, W, X.device, bind_scales, trainable=trainable_scales)
        Y = out if out is not None else torch.empty((self.N, F_out), dtype=torch.bfloat16, device=X.device)
        if variant == "fused":
            self._ensure_fused(F_in)
        with torch.cuda.device(X.device):
            if isinstance(cb, torch.Tensor):
                _check_feat(cb, "cb", device=X.device)
                cb_host, cb_dev = 0.0, _ptr(cb)
            else:
                cb_host, cb_dev = float(cb), None
            head = (self._h, F_in, F_out, _ptr(csrptr_t), _ptr(colind_t), _ptr(X), _ptr(degE), _ptr(degV), _ptr(W),
                    _ptr(packed), _ptr(residual), float(ca), cb_host, cb_dev, LIN_RELU if relu else 0, _ptr(t_out), _ptr(Y))
            fn = _lib.lib().hg_aggr_linear_res_bf16
            self._run_with_workspace(fn, head, (_lib.VARIANTS[variant], _stream_handle(X.device)), F_in, workspace, X.device,
                                     self.linear_workspace_bytes)
        return Y

    def _drop_unit_weights(self, W, enable=True):
        """The reference's layers each carry their own all-ones `Wdiag` (model/ugsys/hgnn.py:12): multiplying by
        exactly 1.0f is the identity, so such a W is not passed on at all -- same bits, no multiply, and the
        layers of a model then share ONE bound scale set instead of re-binding at every call.  Checked once
        per tensor (address, torch version counter); `bind_scales=False` skips the shortcut as it skips binding."""
        if W is None or not enable or W.requires_grad:
            return W
        if not hasattr(self, "_unit_w"):
            self._unit_w, self._unit_w_misses = {}, 0
        key = (W.data_ptr(), W._version, W.numel())
        hit = self._unit_w.get(key)
        if hit is None:
            if self._unit_w_misses >= 16:  # weights that keep changing and are never all ones: stop looking
                return W                   # (the check reads one flag back from the device)
            if len(self._unit_w) > 64:
                self._unit_w.clear()
            hit = self._unit_w[key] = (bool((W == 1).all().item()), W)  # keeps W (and its address) alive
            self._unit_w_misses = 0 if hit[0] else self._unit_w_misses + 1
        return None if hit[0] else W

    def _bind_scales(self, F, degE, degV, W, device, enable=True, stream=None, trainable=False):
        """Degree / weight vectors are graph constants: pre-gather them into the fused
        schedule's panel order once (hg_plan_bind_scales) and again only when a tensor is
        replaced or modified in place (data_ptr / torch version counter).

        The rule for callers: the library compares addresses, this layer adds torch's version
        counter.  A write that bumps neither (`t.data.mul_()`, a numpy or DLPack alias, another
        library writing in place) is invisible -- call `plan.unbind()` after such a write, or
        pass `bind_scales=False` for vectors that change that way; the kernel then gathers
        degE / W / degV itself on every call (a few percent slower, always current).

        The gather kernel runs on the stream current at binding time; a later call on another
        stream waits for it through an event."""
        if not hasattr(self, "_bound"):
            self._bound, self._auto, self._bind_stats = {}, {}, {}
        if F not in self._auto:
            self._auto[F] = self.auto_variant(F)
        if self._auto[F] != "fused":
            return
        if not enable:
            self.unbind(F)
            return
        if trainable or any(t is not None and t.requires_grad for t in (degE, degV, W)):
            # A trainable scale changes at every optimizer step: binding it would re-gather, and synchronise, on every
            # call.  Such a set is never bound -- the kernels gather it themselves -- and a binding of other tensors
            # stays as it is (the library matches a binding by address).  Only a binding of these very addresses, made
            # before the tensor was marked trainable, is dropped.
            hit = self._bound.get(F)
            if hit is not None and tuple(None if k is None else k[0] for k in hit[0]) == \
                    tuple(None if t is None else t.data_ptr() for t in (degE, degV, W)):
                self.unbind(F)
            return
        key = tuple(None if t is None else (t.data_ptr(), t._version) for t in (degE, degV, W))
        if stream is None:
            stream = torch.cuda.current_stream(device)
        hit = self._bound.get(F)
        if hit is not None and hit[0] == key:
            if hit[2] != stream.cuda_stream:
                stream.wait_event(hit[3])
            self._bind_stats[F][0] += 1
            return
        # Callers that alternate between scale sets at one width (layers with different W, an adjoint backward)
        # would re-gather at every call: after a few re-binds that were not followed by reuse, stop binding this
        # width -- the kernels then gather degE / W / degV themselves (a few percent, not a gather + a sync).
        st = self._bind_stats.setdefault(F, [0, 0])  # [reuses, binds]
        if st[1] >= 8 and st[0] < st[1]:
            if hit is not None:
                self.unbind(F)
            return
        st[1] += 1
        with torch.cuda.device(device):
            _lib.check(_lib.lib().hg_plan_bind_scales(self._h, F, _ptr(degE), _ptr(degV), _ptr(W),
                                                      _stream_handle(device)))
            ev = torch.cuda.Event()
            ev.record(stream)
        # keep the tensors (and so their addresses) alive; remember where the gather was enqueued
        self._bound[F] = (key, (degE, degV, W), stream.cuda_stream, ev)

    def unbind(self, F=None):
        """Forget the pre-gathered scale vectors (of feature width F, or all): the next call either
        binds afresh or, with bind_scales=False, reads degE / W / degV directly."""
        bound = getattr(self, "_bound", {})
        for f in ([F] if F is not None else list(bound)):
            if f in bound:
                dev = next((t.device for t in bound[f][1] if t is not None), self.device)
                with torch.cuda.device(dev):
                    _lib.check(_lib.lib().hg_plan_bind_scales(self._h, f, None, None, None, _stream_handle(dev)))
                del bound[f]

    def gather_rows(self, hop, csrptr_t, colind_t, src, scaleA=None, scaleB=None):
        """One hop: hop 0 = H^T src (rows = hyperedges), hop 1 = H src."""
        _check_feat(src, "src")
        F = src.shape[1]
        nrows = self.M if hop == 0 else self.N
        dst = torch.empty((nrows, F), dtype=torch.float32, device=src.device)
        workspace, nbytes = self._workspace(F, src.device)
        with torch.cuda.device(src.device):
            _lib.check(_lib.lib().hg_gather_rows_f32(
                self._h, hop, F, _ptr(csrptr_t), _ptr(colind_t), _ptr(src), _ptr(scaleA), _ptr(scaleB),
                _ptr(dst), _ptr(workspace), nbytes, _stream_handle(src.device)))
        return dst

    def gather_rows_incidence(self, hop, csrptr_t, colind_t, src, w=None, scaleA=None, scaleB=None, heads=1, out=None,
                              workspace=None):
        """One hop of aggregate_incidence as a call of its own (hg_gather_rows_incidence_heads_f32): hop 0 / 'hyperedge',
        dst[e] = ((sum_{p=(e,u)} w[p] src[u]) * scaleA[e]) * scaleB[e] with src [N, F] and dst [M, F]; hop 1 / 'vertex' the
        mirror, src [M, F] and dst [N, F].  w: float32 [nnz] in H_T order ([nnz, H] with heads = H, column h weighing head
        h's columns), or None (unit weights); the scales have one factor per row of dst.  The schedule, kernels and bits
        are those of aggregate_incidence's hop.  The first hop-1 call with w uploads the plan's permutation: not capturable.
        src and out may each be float32 or bfloat16 (hg_gather_rows_incidence_heads_bf16); dst has src's dtype unless out says
        otherwise.  w and the scales stay float32.  Sums are fp32 in the float32 call's order and a bfloat16 dst is rounded once:
        the result equals the float32 call on src.float(), rounded where dst is bfloat16, bit for bit.  Where the bf16 lanes do
        not exist (F % 4 or (F / heads) % 4 != 0, or data not 8- / 16-byte aligned) exactly that is run: widen, float32 call, round."""
        heads = _heads(heads)
        hop = _side(hop)
        _check_feat(src, "src", bf16_ok=True)
        nsrc, ndst = (self.N, self.M) if hop == 0 else (self.M, self.N)
        if src.dim() != 2 or src.shape[0] != nsrc:
            raise ValueError("src must be [%d, F]" % nsrc)
        F = src.shape[1]
        if F % heads:
            raise ValueError("F = %d is no multiple of heads = %d" % (F, heads))
        _check_scales((("w", w, self.nnz * heads), ("scaleA", scaleA, ndst), ("scaleB", scaleB, ndst)), src.device)
        if out is not None:
            _check_feat(out, "out", device=src.device, bf16_ok=True)
            if tuple(out.shape) != (ndst, F):
                raise ValueError("out must be [%d, %d]" % (ndst, F))
        dst = out if out is not None else torch.empty((ndst, F), dtype=src.dtype, device=src.device)
        io = (_lib.HG_ROWS_SRC_BF16 if src.dtype == torch.bfloat16 else 0) | (_lib.HG_ROWS_DST_BF16 if dst.dtype == torch.bfloat16 else 0)
        if io and not _bf16_lanes(F, heads, src, dst):
            got = self.gather_rows_incidence(hop, csrptr_t, colind_t, src.float(), w, scaleA, scaleB, heads,
                                             dst if dst.dtype == torch.float32 else None, workspace)
            return got if got is dst else dst.copy_(got)  # copy_ rounds to nearest even, as the kernel's store does
        workspace, nbytes = self._incidence_workspace(F, workspace, src.device)
        with torch.cuda.device(src.device):
            if io:
                _lib.check(_lib.lib().hg_gather_rows_incidence_heads_bf16(
                    self._h, hop, F, heads, _ptr(csrptr_t), _ptr(colind_t), _ptr(src), _ptr(w), _ptr(scaleA), _ptr(scaleB),
                    _ptr(dst), _ptr(workspace), nbytes, io, _stream_handle(src.device)))
            else:
                _lib.check(_lib.lib().hg_gather_rows_incidence_heads_f32(
                    self._h, hop, F, heads, _ptr(csrptr_t), _ptr(colind_t), _ptr(src), _ptr(w), _ptr(scaleA), _ptr(scaleB),
                    _ptr(dst), _ptr(workspace), nbytes, _stream_handle(src.device)))
        return dst

    def reduce_workspace_bytes(self, F):
        return int(_lib.lib().hg_gather_rows_reduce_workspace_bytes(self._h, F))

    def _reduce_args(self, hop, rows, arg, out, F=None):
        """Checks gather_rows_reduce and gather_rows_select share: rows [nsrc, F] float32 on a GPU, the int32 table beside
        it, the result's shape.  Returns (hop, nsrc, ndst, F)."""
        hop = _side(hop)
        _check_feat(rows, "src")
        nsrc, ndst = (self.N, self.M) if hop == 0 else (self.M, self.N)
        if rows.dim() != 2:
            raise ValueError("src must be [rows, F]")
        F = rows.shape[1]
        if arg is not None:
            if not isinstance(arg, torch.Tensor) or arg.dtype != torch.int32:
                raise TypeError("arg must be an int32 tensor")
            if not arg.is_cuda or arg.device != rows.device or not arg.is_contiguous():
                raise RuntimeError("arg must be contiguous and on %s" % rows.device)
        if out is not None:
            _check_feat(out, "out", device=rows.device)
        return hop, nsrc, ndst, F

    def gather_rows_reduce(self, hop, csrptr_t, colind_t, src, op, scaleA=None, scaleB=None, out=None, arg_out=None,
                           workspace=None):
        """One hop with max or min in place of the sum (hg_gather_rows_reduce_f32): hop 0 / 'hyperedge',
        dst[e, c] = ((op over the members u of e of src[u, c]) * scaleA[e]) * scaleB[e] with src [N, F] and dst [M, F]; hop 1 /
        'vertex' the mirror.  op: 'max' or 'min'.  Returns (dst, arg): arg int32 [rows of dst, F] holds the winning
        incidence's position in colind_t -- the greatest (smallest) value under > (<), the smallest position among ties, so
        -0.0 ties +0.0 -- and dst is src[colind[arg]] scaled, bit for bit.  An empty row gets +0.0 and arg = -1 whatever its
        scale.  NaN inputs: unspecified.  float32 only; every schedule and every call give the same bits.  The first hop-1
        call uploads the plan's permutation: not capturable."""
        if op not in ("max", "min"):
            raise ValueError("op must be 'max' or 'min', got %r" % (op,))
        hop, nsrc, ndst, F = self._reduce_args(hop, src, arg_out, out)
        if src.shape[0] != nsrc:
            raise ValueError("src must be [%d, F]" % nsrc)
        _check_scales((("scaleA", scaleA, ndst), ("scaleB", scaleB, ndst)), src.device)
        for name, t in (("out", out), ("arg_out", arg_out)):
            if t is not None and tuple(t.shape) != (ndst, F):
                raise ValueError("%s must be [%d, %d]" % (name, ndst, F))
        dst = out if out is not None else torch.empty((ndst, F), dtype=torch.float32, device=src.device)
        arg = arg_out if arg_out is not None else torch.empty((ndst, F), dtype=torch.int32, device=src.device)
        nbytes = self.reduce_workspace_bytes(F)
        if workspace is None:
            workspace = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
        with torch.cuda.device(src.device):
            _lib.check(_lib.lib().hg_gather_rows_reduce_f32(
                self._h, hop, F, _lib.HG_REDUCE_MAX if op == "max" else _lib.HG_REDUCE_MIN, _ptr(csrptr_t), _ptr(colind_t),
                _ptr(src), _ptr(scaleA), _ptr(scaleB), _ptr(dst), _ptr(arg), _ptr(workspace),
                workspace.numel() * workspace.element_size(), _stream_handle(src.device)))
        return dst, arg

    def gather_rows_select(self, hop, csrptr_t, colind_t, gs, arg, out=None, workspace=None):
        """The gradient of gather_rows_reduce's src (hg_gather_rows_select_f32).  hop names the hop being differentiated;
        gs (the incoming gradient times the hop's scales) and arg (its winners) are [rows of that hop's dst, F].  Every row
        of the result gathers, over the other hop's CSR and in the sum gather's order, the gs of the rows it won:
        dsrc[u, c] = sum_q (arg[r_q, c] == pos(q)) ? gs[r_q, c] : 0.  No atomics: two calls give the same bits."""
        hop, nsrc, ndst, F = self._reduce_args(hop, gs, arg, out)
        if arg is None or tuple(gs.shape) != (ndst, F) or tuple(arg.shape) != (ndst, F):
            raise ValueError("gs and arg must be [%d, F]" % ndst)
        if out is not None and tuple(out.shape) != (nsrc, F):
            raise ValueError("out must be [%d, %d]" % (nsrc, F))
        dsrc = out if out is not None else torch.empty((nsrc, F), dtype=torch.float32, device=gs.device)
        if workspace is None:
            workspace = torch.empty(self.reduce_workspace_bytes(F), dtype=torch.uint8, device=gs.device)
        with torch.cuda.device(gs.device):
            _lib.check(_lib.lib().hg_gather_rows_select_f32(
                self._h, hop, F, _ptr(csrptr_t), _ptr(colind_t), _ptr(gs), _ptr(arg), _ptr(dsrc), _ptr(workspace),
                workspace.numel() * workspace.element_size(), _stream_handle(gs.device)))
        return dsrc

    def row_recip(self, hop, csrptr_t):
        """float32 device tensor of 1 / (row length) of one side -- [M], 1 / |e|, for hop 0 / 'hyperedge'; [N], one over a
        vertex's number of incidences, for hop 1 / 'vertex' -- with 0 for an empty row: the mean's scale.  Built by the
        first call outside a stream capture and kept with the plan (nonempty_edges' rule inside one)."""
        hop = _side(hop)
        cache = self.__dict__.setdefault("_row_recip", {})
        key = (hop, str(csrptr_t.device))
        hit = cache.get(key)
        if hit is not None:
            return hit
        if hop == 0:
            length = (csrptr_t[1:] - csrptr_t[:-1]).to(torch.float32)
        else:
            ptr_v = torch.from_numpy(self.vertex_csr()[0]).to(csrptr_t.device)
            length = (ptr_v[1:] - ptr_v[:-1]).to(torch.float32)
        recip = torch.where(length > 0, 1.0 / length, torch.zeros_like(length))
        if not torch.cuda.is_current_stream_capturing():
            cache[key] = recip
        return recip

    def incidence_perm(self):
        """Host copy (numpy int32 [nnz]) of perm[q] = the H_T position of H entry q: the stable transpose behind
        vertex_csr(), by which hop 2 of aggregate_incidence reads e2v.  Works on host-only plans too."""
        perm = np.empty(self.nnz, np.int32)
        _lib.check(_lib.lib().hg_plan_get_incidence_perm(self._h, perm.ctypes.data_as(ctypes.c_void_p)))
        return perm

    def incidence_workspace_bytes(self, F):
        return int(_lib.lib().hg_aggr_incidence_workspace_bytes(self._h, F))

    def _incidence_workspace(self, F, workspace, device):
        """(workspace, the bytes of it to pass on) of an incidence call at width F: the caller's with its own size, or a new
        one of incidence_workspace_bytes(F)."""
        if workspace is not None:
            return workspace, workspace.numel() * workspace.element_size()
        nbytes = self.incidence_workspace_bytes(F)
        return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device), nbytes

    def aggregate_incidence(self, csrptr_t, colind_t, X, v2e=None, e2v=None, degE=None, degV=None, W=None,
                            xe_out=None, out=None, workspace=None, heads=1):
        """Y = degV . H_e2v (degE . W . (H_v2e^T X)) with a weight per incidence (hg_aggr_incidence_f32): v2e / e2v are
        float32 [nnz] aligned with colind_t, or None (unit weights).  xe_out ([M, F] float32) receives hop 1's table.
        heads = H > 1 (hg_aggr_incidence_heads_f32): v2e / e2v are [nnz, H] and head h weighs columns h F/H .. (h+1) F/H - 1.
        The first call with e2v builds and uploads the plan's permutation: not capturable (make one call before a
        hipGraph capture).
        X may be bfloat16 (hg_aggr_incidence_heads_bf16): Y (and out) are then bfloat16, the weights, the scales and xe_out
        stay float32.  Hop 1's table and every sum are fp32 in the float32 call's order, Y is rounded once: Y equals
        aggregate_incidence(X.float(), ...).to(bfloat16) and xe_out the float32 call's, bit for bit.  Where the bf16 lanes do
        not exist (F % 4 or (F / heads) % 4 != 0, data not 8- / 16-byte aligned) exactly that is run."""
        heads = _heads(heads)
        bf16 = isinstance(X, torch.Tensor) and X.dtype == torch.bfloat16
        _check_feat(X, "node_feat", bf16_ok=True)
        if X.dim() != 2 or X.shape[0] != self.N:
            raise ValueError("node_feat must be [N = %d, F]" % self.N)
        F = X.shape[1]
        if F % heads:
            raise ValueError("F = %d is no multiple of heads = %d" % (F, heads))
        _check_scales((("v2e", v2e, self.nnz * heads), ("e2v", e2v, self.nnz * heads), ("degE", degE, self.M),
                       ("degV", degV, self.N), ("W", W, self.M)), X.device)
        for name, t, rows in (("xe_out", xe_out, self.M), ("out", out, self.N)):
            if t is not None:
                _check_feat(t, name, device=X.device, bf16_ok=bf16 and name == "out")
                if tuple(t.shape) != (rows, F):
                    raise ValueError("%s must be [%d, %d]" % (name, rows, F))
        if out is not None and out.dtype != X.dtype:
            raise TypeError("out must have node_feat's dtype %s, got %s" % (X.dtype, out.dtype))
        if bf16 and not _bf16_lanes(F, heads, X, out, xe_out):
            Y32 = self.aggregate_incidence(csrptr_t, colind_t, X.float(), v2e, e2v, degE, degV, W, xe_out, None, workspace, heads)
            return Y32.to(torch.bfloat16) if out is None else out.copy_(Y32)
        Y = out if out is not None else torch.empty((self.N, F), dtype=X.dtype, device=X.device)
        workspace, nbytes = self._incidence_workspace(F, workspace, X.device)
        with torch.cuda.device(X.device):
            if bf16:
                _lib.check(_lib.lib().hg_aggr_incidence_heads_bf16(
                    self._h, F, heads, _ptr(csrptr_t), _ptr(colind_t), _ptr(X), _ptr(v2e), _ptr(e2v), _ptr(degE),
                    _ptr(degV), _ptr(W), _ptr(xe_out), _ptr(Y), _ptr(workspace), nbytes, _stream_handle(X.device)))
            elif heads == 1:
                _lib.check(_lib.lib().hg_aggr_incidence_f32(
                    self._h, F, _ptr(csrptr_t), _ptr(colind_t), _ptr(X), _ptr(v2e), _ptr(e2v), _ptr(degE), _ptr(degV),
                    _ptr(W), _ptr(xe_out), _ptr(Y), _ptr(workspace), nbytes, _stream_handle(X.device)))
            else:
                _lib.check(_lib.lib().hg_aggr_incidence_heads_f32(
                    self._h, F, heads, _ptr(csrptr_t), _ptr(colind_t), _ptr(X), _ptr(v2e), _ptr(e2v), _ptr(degE),
                    _ptr(degV), _ptr(W), _ptr(xe_out), _ptr(Y), _ptr(workspace), nbytes, _stream_handle(X.device)))
        return Y

    def incidence_dot(self, csrptr_t, colind_t, A, B, out=None, heads=1):
        """out[p] = <A[u], B[e]> for every H_T entry p = (e, u) (hg_incidence_dot_f32): A [N, F], B [M, F].  heads = H > 1
        (hg_incidence_dot_heads_f32): out [nnz, H], out[p, h] the product over head h's columns h F/H .. (h+1) F/H - 1.
        A and B may each be float32 or bfloat16 (hg_incidence_dot_heads_bf16); out is float32 and equals the float32 call on
        A.float(), B.float() bit for bit (that call is what runs where F % 4, (F / heads) % 4 or the alignment rule out the
        bf16 lanes)."""
        heads = _heads(heads)
        _check_feat(A, "A", bf16_ok=True)
        _check_feat(B, "B", device=A.device, bf16_ok=True)
        if A.dim() != 2 or B.dim() != 2 or A.shape[0] != self.N or B.shape[0] != self.M or A.shape[1] != B.shape[1]:
            raise ValueError("A must be [N = %d, F] and B [M = %d, F]" % (self.N, self.M))
        if A.shape[1] % heads:
            raise ValueError("F = %d is no multiple of heads = %d" % (A.shape[1], heads))
        if out is None:
            out = torch.empty(_per_head(self.nnz, heads), dtype=torch.float32, device=A.device)
        else:
            _check_feat(out, "out", device=A.device)
            if out.numel() != self.nnz * heads:
                raise ValueError("out must have nnz * heads = %d elements" % (self.nnz * heads))
        io = (_lib.HG_DOT_A_BF16 if A.dtype == torch.bfloat16 else 0) | (_lib.HG_DOT_B_BF16 if B.dtype == torch.bfloat16 else 0)
        if io and not _bf16_lanes(A.shape[1], heads, A, B):
            return self.incidence_dot(csrptr_t, colind_t, A.float(), B.float(), out, heads)
        with torch.cuda.device(A.device):
            if io:
                _lib.check(_lib.lib().hg_incidence_dot_heads_bf16(self._h, A.shape[1], heads, _ptr(csrptr_t), _ptr(colind_t),
                                                                  _ptr(A), _ptr(B), _ptr(out), io, _stream_handle(A.device)))
            elif heads == 1:
                _lib.check(_lib.lib().hg_incidence_dot_f32(self._h, A.shape[1], _ptr(csrptr_t), _ptr(colind_t), _ptr(A),
                                                           _ptr(B), _ptr(out), _stream_handle(A.device)))
            else:
                _lib.check(_lib.lib().hg_incidence_dot_heads_f32(self._h, A.shape[1], heads, _ptr(csrptr_t),
                                                                 _ptr(colind_t), _ptr(A), _ptr(B), _ptr(out),
                                                                 _stream_handle(A.device)))
        return out

    def hyperedge_dot(self, csrptr_t, colind_t, A, B, a_weight=None, b_weight=None, heads=1):
        """out[e] = sum_c (sum_{p=(e,u)} a_weight[p, c/C] A[u, c]) * (sum_{p=(e,u)} b_weight[p, c/C] B[u, c]), float32 [M]
        (hg_hyperedge_dot_heads_f32): the product of two hyperedge sums without either [M, F] table -- q of the degE / W
        gradients with (A, a_weight) = (X, v2e) and (B, b_weight) = (degV * dY, e2v).  A, B: float32 [N, F]; the weights:
        float32 with nnz * heads elements in H_T order (head fastest), or None (unit weights); C = F / heads.  A plain
        kernel call, no autograd.  Refusals are decided in ops._incidence_args' order, before a device is touched.  The
        first call on a plan uploads the long-row list the segment kernels share: not capturable."""
        heads = _heads(heads)
        floats = (("A", A), ("B", B), ("a_weight", a_weight), ("b_weight", b_weight))
        for name, t in floats:
            if (t is not None or name in ("A", "B")) and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32):
                raise TypeError("%s must be a float32 tensor (hyperedge_dot has no bfloat16 form), got %s"
                                % (name, getattr(t, "dtype", type(t))))
        if A.dim() != 2 or B.dim() != 2 or A.shape[0] != self.N or tuple(B.shape) != tuple(A.shape):
            raise ValueError("A and B must both be [N = %d, F], got %s and %s" % (self.N, tuple(A.shape), tuple(B.shape)))
        F = A.shape[1]
        if F < 1:
            raise ValueError("the feature width must be at least 1")
        if F % heads:
            raise ValueError("F = %d is no multiple of heads = %d" % (F, heads))
        for name, t in floats[2:]:
            if t is not None and t.numel() != self.nnz * heads:
                raise ValueError("%s must have nnz * heads = %d elements, got %d" % (name, self.nnz * heads, t.numel()))
        _check_index(csrptr_t, "csrptr_t")
        _check_index(colind_t, "indices_t")
        _check_feat(A, "A")
        for name, t in floats[1:]:
            if t is not None:
                _check_feat(t, name, device=A.device)
        out = torch.empty(self.M, dtype=torch.float32, device=A.device)
        with torch.cuda.device(A.device):
            _lib.check(_lib.lib().hg_hyperedge_dot_heads_f32(
                self._h, F, heads, _ptr(csrptr_t), _ptr(colind_t), _ptr(A), _ptr(a_weight), _ptr(B), _ptr(b_weight),
                _ptr(out), _stream_handle(A.device)))
        return out

    def rows_dot(self, A, B):
        """out[r] = <A[r, :], B[r, :]>, float32 [rows], for two float32 [rows, F] tensors (hg_rows_dot_f32): the last step
        of the degV gradient, <dY[v], Z[v]>.  One lane group per row, fixed order.  A plain kernel call, no autograd."""
        for name, t in (("A", A), ("B", B)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise TypeError("%s must be a float32 tensor (rows_dot has no bfloat16 form), got %s"
                                % (name, getattr(t, "dtype", type(t))))
        if A.dim() != 2 or tuple(B.shape) != tuple(A.shape) or A.shape[1] < 1:
            raise ValueError("A and B must be [rows, F] of one shape with F >= 1, got %s and %s"
                             % (tuple(A.shape), tuple(B.shape)))
        _check_feat(A, "A")
        _check_feat(B, "B", device=A.device)
        out = torch.empty(A.shape[0], dtype=torch.float32, device=A.device)
        with torch.cuda.device(A.device):
            _lib.check(_lib.lib().hg_rows_dot_f32(A.shape[0], A.shape[1], _ptr(A), _ptr(B), _ptr(out),
                                                  _stream_handle(A.device)))
        return out

    def nonempty_edges(self, csrptr_t):
        """bool [M] device tensor: the hyperedges with at least one member (their scales take part in the result; an
        empty one's degE may be inf).  Built by the first call outside a stream capture and kept with the plan; a call
        inside a capture before that builds one for that graph alone (it would lie in the graph's private pool)."""
        mask = self._nonempty
        if mask is None or mask.device != csrptr_t.device:
            mask = csrptr_t[1:] != csrptr_t[:-1]
            # a mask made during a stream capture lives in that graph's private pool: it serves the capture and is not kept
            if not torch.cuda.is_current_stream_capturing():
                self._nonempty = mask
        return mask

    def segment_info(self, side):
        """How the segment kernels cut one side ('hyperedge' / 'vertex', or 0 / 1): {"width": lanes per group, "keep":
        entries a lane keeps in registers, "long": the longest row a lane group takes, "long_rows": int32 ids of the
        longer rows, which get a workgroup each} (hg_plan_get_segment_info).  Works on host-only plans."""
        side = _side(side)
        info = (ctypes.c_int32 * 4)()
        _lib.check(_lib.lib().hg_plan_get_segment_info(self._h, side, info, None))
        rows = np.empty(info[3], np.int32)
        _lib.check(_lib.lib().hg_plan_get_segment_info(self._h, side, info, rows.ctypes.data_as(ctypes.c_void_p)))
        return {"width": info[0], "keep": info[1], "long": info[2], "long_rows": rows}

    def _scores(self, sv, se, device=None, heads=1, entry=None):
        for name, t, n in (("node_score", sv, self.N * heads), ("edge_score", se, self.M * heads),
                           ("incidence_score", entry, self.nnz * heads)):
            if t is not None:
                _check_feat(t, name, device=device)
                device = t.device
                if t.numel() != n:
                    raise ValueError("%s must have %d elements, got %d" % (name, n, t.numel()))
        return device

    def _rng_ptr(self, rng_state, device):
        _rng_state_dtype(rng_state)
        _rng_state_length(rng_state)
        _rng_state_device(rng_state, device)
        return _ptr(rng_state)

    def _softmax_entry(self, bwd, group, heads, csrptr_t, colind_t, sv, se, entry, slope, p_drop, rng):
        """(the softmax's C entry for a form, its leading arguments).  The eight entries, named by the four methods below,
        differ in their argument lists only by entry after se and (p_drop, rng) after slope; the arrays follow."""
        if entry is not None and self.nnz == 0:
            entry = None  # nothing to add it to (and an empty tensor has no address to pass)
        fn = getattr(_lib.lib(), _SOFTMAX_ENTRIES[entry is not None, rng is not None, bwd])
        head = (self._h, group, heads, _ptr(csrptr_t), _ptr(colind_t), _ptr(sv), _ptr(se))
        if rng is None:
            return fn, head + ((float(slope),) if entry is None else (_ptr(entry), float(slope)))
        return fn, head + ((float(slope), float(p_drop), rng) if entry is None else (_ptr(entry), float(slope), float(p_drop), rng))

    def _softmax(self, csrptr_t, colind_t, sv, se, group, slope, heads, entry=None, p_drop=None, rng_state=None, out=None):
        """incidence_attention (p_drop None: alpha, written to `out` where one is given) and incidence_attention_dropout
        ((alpha, alpha_drop)): the checks in their one order, the allocations, the launch."""
        heads = _heads(heads)
        group = _side(group)
        _check_index(csrptr_t, "csrptr_t")
        _check_index(colind_t, "indices_t")
        device = self._scores(sv, se, csrptr_t.device, heads, entry)
        rng = None if p_drop is None else self._rng_ptr(rng_state, device)
        if out is None:
            out = torch.empty(_per_head(self.nnz, heads), dtype=torch.float32, device=device)
        else:
            _check_feat(out, "out", device=device)
            if out.numel() != self.nnz * heads:
                raise ValueError("out must have nnz * heads = %d elements" % (self.nnz * heads))
        fn, args = self._softmax_entry(False, group, heads, csrptr_t, colind_t, sv, se, entry, slope, p_drop, rng)
        with torch.cuda.device(device):
            if rng is None:
                _lib.check(fn(*args, _ptr(out), _stream_handle(device)))
                return out
            alpha_drop = torch.empty_like(out)
            _lib.check(fn(*args, _ptr(out), _ptr(alpha_drop), _stream_handle(device)))
        return out, alpha_drop

    def _softmax_backward(self, csrptr_t, colind_t, alpha, grad, grad_name, sv, se, group, slope, need_sv, need_se, heads,
                          entry=None, p_drop=None, rng_state=None):
        """incidence_attention_backward (p_drop None) and incidence_attention_dropout_backward: (ds, dsv or None, dse or
        None).  grad_name: the name under which the incoming gradient is refused, 'dalpha' or 'dout'."""
        heads = _heads(heads)
        group = _side(group)
        _check_index(csrptr_t, "csrptr_t")
        _check_index(colind_t, "indices_t")
        _check_feat(alpha, "alpha")
        _check_feat(grad, grad_name, device=alpha.device)
        for name, t in (("alpha", alpha), (grad_name, grad)):
            if t.numel() != self.nnz * heads:
                raise ValueError("%s must have nnz%s = %d elements, got %d" % (name, " * heads" if heads > 1 else "",
                                                                              self.nnz * heads, t.numel()))
        device = self._scores(sv, se, alpha.device, heads, entry)
        rng = None if p_drop is None else self._rng_ptr(rng_state, device)
        ds = torch.empty(_per_head(self.nnz, heads), dtype=torch.float32, device=device)
        dsv = torch.empty(_per_head(self.N, heads), dtype=torch.float32, device=device) if need_sv else None
        dse = torch.empty(_per_head(self.M, heads), dtype=torch.float32, device=device) if need_se else None
        fn, args = self._softmax_entry(True, group, heads, csrptr_t, colind_t, sv, se, entry, slope, p_drop, rng)
        with torch.cuda.device(device):
            _lib.check(fn(*args, _ptr(alpha), _ptr(grad), _ptr(ds), _ptr(dsv), _ptr(dse), _stream_handle(device)))
        return ds, dsv, dse

    def incidence_attention(self, csrptr_t, colind_t, sv=None, se=None, group="hyperedge", slope=0.2, out=None, heads=1,
                            entry=None):
        """alpha [nnz] in H_T order: the softmax over each hyperedge's members (group 'hyperedge') or each vertex's
        hyperedges ('vertex') of leaky_relu(sv[u] + se[e], slope) (hg_incidence_attention_f32).  sv [N], se [M]: float32,
        or None (0).  heads = H > 1 (hg_incidence_attention_heads_f32): sv [N, H], se [M, H], alpha [nnz, H], a softmax
        per head.  The first call of a form builds and uploads what it needs from the plan: not capturable.
        entry: float32 [nnz] / [nnz, H] in H_T order, a logit per incidence added to the score, raw = (sv[u] + se[e]) +
        entry[p] (hg_incidence_attention_entry_heads_f32); None is the call without one."""
        return self._softmax(csrptr_t, colind_t, sv, se, group, slope, heads, entry, out=out)

    def incidence_attention_backward(self, csrptr_t, colind_t, alpha, dalpha, sv=None, se=None, group="hyperedge",
                                     slope=0.2, need_sv=True, need_se=True, heads=1, entry=None):
        """(ds [nnz], dsv [N] or None, dse [M] or None) for alpha = incidence_attention(...) and its gradient dalpha
        (hg_incidence_attention_bwd_f32); sv / se as in the forward (they decide the leaky branch).  heads = H > 1
        (hg_incidence_attention_heads_bwd_f32): every array has a trailing dimension H.  entry: the forward's logit per
        incidence (hg_incidence_attention_entry_heads_bwd_f32); ds is then its gradient."""
        return self._softmax_backward(csrptr_t, colind_t, alpha, dalpha, "dalpha", sv, se, group, slope, need_sv, need_se, heads,
                                      entry)

    def incidence_attention_stats(self, csrptr_t, colind_t, sv=None, se=None, group="hyperedge", slope=0.2, heads=1,
                                  out=None):
        """(seg_max, seg_inv) of incidence_attention's softmax, one pair per segment and head: the maximum of
        leaky_relu(sv[u] + se[e], slope) over the segment and the reciprocal of its sum of exponentials, float32 [M] /
        [M, H] for group 'hyperedge', [N] / [N, H] for 'vertex'; (0, 0) for an empty segment
        (hg_incidence_attention_stats_heads_f32).  alpha[p] = exp(leaky(raw[p]) - seg_max[g]) * seg_inv[g] has
        incidence_attention's bits; aggregate_incidence_attention forms it in the gather.  out: a pair of such tensors.
        The first call on a side uploads the long-row list the segment kernels share: not capturable."""
        heads = _heads(heads)
        group = _side(group)
        _check_index(csrptr_t, "csrptr_t")
        _check_index(colind_t, "indices_t")
        device = self._scores(sv, se, csrptr_t.device, heads)
        nseg = self.M if group == 0 else self.N
        if out is None:
            out = tuple(torch.empty(_per_head(nseg, heads), dtype=torch.float32, device=device) for _ in range(2))
        else:
            for t in out:
                _check_feat(t, "out", device=device)
                if t.numel() != nseg * heads:
                    raise ValueError("out must be two tensors of %d elements" % (nseg * heads))
        seg_max, seg_inv = out
        with torch.cuda.device(device):
            _lib.check(_lib.lib().hg_incidence_attention_stats_heads_f32(
                self._h, group, heads, _ptr(csrptr_t), _ptr(colind_t), _ptr(sv), _ptr(se), float(slope), _ptr(seg_max),
                _ptr(seg_inv), _stream_handle(device)))
        return seg_max, seg_inv

    def _attention_args(self, X, nrows, sv, se, seg_max, seg_inv, group, heads):
        _check_feat(X, "node_feat")
        if X.dim() != 2 or X.shape[0] != nrows:
            raise ValueError("the feature rows must be [%d, F]" % nrows)
        F = X.shape[1]
        if F % heads:
            raise ValueError("F = %d is no multiple of heads = %d" % (F, heads))
        self._scores(sv, se, X.device, heads)
        nseg = self.M if group == 0 else self.N
        for name, t in (("seg_max", seg_max), ("seg_inv", seg_inv)):
            _check_feat(t, name, device=X.device)
            if t.numel() != nseg * heads:
                raise ValueError("%s must have %d elements, got %d" % (name, nseg * heads, t.numel()))
        return F

    def aggregate_incidence_attention(self, csrptr_t, colind_t, X, sv=None, se=None, group="hyperedge", slope=0.2,
                                      seg_max=None, seg_inv=None, degE=None, degV=None, W=None, xe_out=None, out=None,
                                      workspace=None, heads=1):
        """aggregate_incidence(X, alpha, alpha, degE, degV, W) for alpha = incidence_attention(sv, se, group, slope), bit
        for bit, without alpha: each gathering lane forms its coefficient from the two scores and the segment's
        statistics (hg_aggr_incidence_attention_heads_f32).  seg_max / seg_inv: incidence_attention_stats' pair for the
        same scores; None computes them here.  No [nnz, H] array exists and the plan's permutation is not used."""
        heads = _heads(heads)
        group = _side(group)
        if seg_max is None or seg_inv is None:
            seg_max, seg_inv = self.incidence_attention_stats(csrptr_t, colind_t, sv, se, group, slope, heads=heads)
        F = self._attention_args(X, self.N, sv, se, seg_max, seg_inv, group, heads)
        _check_scales((("degE", degE, self.M), ("degV", degV, self.N), ("W", W, self.M)), X.device)
        for name, t, rows in (("xe_out", xe_out, self.M), ("out", out, self.N)):
            if t is not None:
                _check_feat(t, name, device=X.device)
                if tuple(t.shape) != (rows, F):
                    raise ValueError("%s must be [%d, %d]" % (name, rows, F))
        Y = out if out is not None else torch.empty((self.N, F), dtype=torch.float32, device=X.device)
        workspace, nbytes = self._incidence_workspace(F, workspace, X.device)
        with torch.cuda.device(X.device):
            _lib.check(_lib.lib().hg_aggr_incidence_attention_heads_f32(
                self._h, F, heads, group, _ptr(csrptr_t), _ptr(colind_t), _ptr(X), _ptr(sv), _ptr(se), float(slope),
                _ptr(seg_max), _ptr(seg_inv), _ptr(degE), _ptr(degV), _ptr(W), _ptr(xe_out), _ptr(Y), _ptr(workspace),
                nbytes, _stream_handle(X.device)))
        return Y

    def gather_rows_attention(self, hop, csrptr_t, colind_t, src, seg_max, seg_inv, sv=None, se=None, group="hyperedge",
                              slope=0.2, scaleA=None, scaleB=None, heads=1, out=None, workspace=None):
        """One hop of aggregate_incidence_attention as a call of its own (hg_gather_rows_attention_heads_f32), as
        gather_rows_incidence is of aggregate_incidence: hop 0 / 'hyperedge' with (degE, W) into hop 1 / 'vertex' with
        (degV, None) gives the two-hop call's bits."""
        heads = _heads(heads)
        hop = _side(hop)
        group = _side(group)
        nsrc, ndst = (self.N, self.M) if hop == 0 else (self.M, self.N)
        F = self._attention_args(src, nsrc, sv, se, seg_max, seg_inv, group, heads)
        _check_scales((("scaleA", scaleA, ndst), ("scaleB", scaleB, ndst)), src.device)
        if out is not None:
            _check_feat(out, "out", device=src.device)
            if tuple(out.shape) != (ndst, F):
                raise ValueError("out must be [%d, %d]" % (ndst, F))
        dst = out if out is not None else torch.empty((ndst, F), dtype=torch.float32, device=src.device)
        workspace, nbytes = self._incidence_workspace(F, workspace, src.device)
        with torch.cuda.device(src.device):
            _lib.check(_lib.lib().hg_gather_rows_attention_heads_f32(
                self._h, hop, group, F, heads, _ptr(csrptr_t), _ptr(colind_t), _ptr(src), _ptr(sv), _ptr(se), float(slope),
                _ptr(seg_max), _ptr(seg_inv), _ptr(scaleA), _ptr(scaleB), _ptr(dst), _ptr(workspace), nbytes,
                _stream_handle(src.device)))
        return dst

    def incidence_attention_dropout(self, csrptr_t, colind_t, sv=None, se=None, group="hyperedge", slope=0.2, p_drop=0.5,
                                    rng_state=None, heads=1, entry=None):
        """(alpha, alpha_drop): incidence_attention's coefficients and, from the same launch, the coefficients after dropout,
        alpha_drop = keep ? alpha / (1 - p_drop) : 0 (hg_incidence_attention_dropout_heads_f32).  rng_state: int64 [2] on
        the scores' device, {key, sid} of the Philox mask; the kernel reads it when it runs.  keep depends on (rng_state,
        H_T position, head) alone; no mask is stored.  [nnz], or [nnz, heads].  entry: as in incidence_attention
        (hg_incidence_attention_entry_dropout_heads_f32)."""
        return self._softmax(csrptr_t, colind_t, sv, se, group, slope, heads, entry, p_drop, rng_state)

    def incidence_attention_dropout_backward(self, csrptr_t, colind_t, alpha, dout, sv=None, se=None, group="hyperedge",
                                             slope=0.2, p_drop=0.5, rng_state=None, need_sv=True, need_se=True, heads=1,
                                             entry=None):
        """(ds, dsv or None, dse or None) for (alpha, alpha_drop) = incidence_attention_dropout(...) and dout, the gradient
        of alpha_drop: incidence_attention_backward on dalpha = keep ? dout / (1 - p_drop) : 0, the mask regenerated from
        rng_state (hg_incidence_attention_dropout_heads_bwd_f32)."""
        return self._softmax_backward(csrptr_t, colind_t, alpha, dout, "dout", sv, se, group, slope, need_sv, need_se, heads,
                                      entry, p_drop, rng_state)

    def incidence_sum(self, csrptr_t, colind_t, val, side="hyperedge", out=None, heads=1):
        """out[e] = sum of val over hyperedge e's incidences (side 'hyperedge', [M]) or out[v] = sum over vertex v's
        (side 'vertex', [N]); val float32 [nnz] in H_T order (hg_incidence_sum_f32).  heads = H > 1
        (hg_incidence_sum_heads_f32): val [nnz, H], out [M, H] / [N, H].  Deterministic, no atomics."""
        heads = _heads(heads)
        side = _side(side)
        _check_index(csrptr_t, "csrptr_t")
        _check_index(colind_t, "indices_t")
        _check_feat(val, "val", device=csrptr_t.device)
        if val.numel() != self.nnz * heads:
            raise ValueError("val must have nnz%s = %d elements, got %d" % (" * heads" if heads > 1 else "",
                                                                            self.nnz * heads, val.numel()))
        n = self.M if side == 0 else self.N
        if out is None:
            out = torch.empty(_per_head(n, heads), dtype=torch.float32, device=val.device)
        else:
            _check_feat(out, "out", device=val.device)
            if out.numel() != n * heads:
                raise ValueError("out must have %d elements" % (n * heads))
        with torch.cuda.device(val.device):
            _lib.check(_lib.lib().hg_incidence_sum_heads_f32(self._h, side, heads, _ptr(csrptr_t), _ptr(colind_t), _ptr(val),
                                                             _ptr(out), _stream_handle(val.device)))
        return out

    def segment_ids(self, csrptr_t, colind_t, side):
        """int64 [nnz] device tensor: the hyperedge (side 'hyperedge') or vertex ('vertex') of every H_T entry -- the gather
        index of incidence_sum's backward.  Built once per side and kept with the plan."""
        side = _side(side)
        cache = self.__dict__.setdefault("_seg_ids", {})
        ids = cache.get(side)
        if ids is None:
            if side == 0:
                sizes = (csrptr_t[1:] - csrptr_t[:-1]).long()
                ids = torch.repeat_interleave(torch.arange(self.M, device=csrptr_t.device), sizes, output_size=self.nnz)
            else:
                ids = colind_t.long()
            cache[side] = ids
        return ids


SIDES = {"hyperedge": 0, "vertex": 1}
# (entry logit, dropout, backward) -> hg_incidence_attention_[entry_][dropout_]heads_[bwd_]f32
_SOFTMAX_ENTRIES = {(e, d, b): "hg_incidence_attention_%s%sheads_%sf32" % ("entry_" * e, "dropout_" * d, "bwd_" * b)
                    for e in (False, True) for d in (False, True) for b in (False, True)}


def _side(side):
    if side in (0, 1):
        return int(side)
    if side not in SIDES:
        raise ValueError("group / side must be 'hyperedge' or 'vertex', got %r" % (side,))
    return SIDES[side]


def _heads(heads):
    """The `heads` argument as an int >= 1 (ValueError otherwise; decided before any tensor is looked at)."""
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError("heads must be an integer >= 1, got %r" % (heads,))
    return heads


def _per_head(n, heads):
    """Shape of a per-item array: [n] for a single head (today's layout), [n, heads] otherwise."""
    return (n,) if heads == 1 else (n, heads)


def linear_supported(F_in, F_out):
    """Widths hg_aggr_linear_f32 takes (MFMA tiles: K in {32, 64, 128}, 16-column output tiles)."""
    return F_in in (32, 64, 128) and F_out > 0 and F_out % 16 == 0


def linear_fusion_pays(F_in, F_out):
    """Measured on MI355X (profiles/r01_linear_epilogue.md): folding the projection into the
    aggregation beats linear-then-aggregate 1.5-1.8x at 32 -> 32 / 64 -> 64, still 1.1x at 64 -> 16
    and 128 -> 128, and loses (0.86x) at 128 -> 64, where the aggregation would run at twice the
    width it needs.  The operator layer fuses only where it wins."""
    return linear_supported(F_in, F_out) and (F_in <= 64 or F_out >= F_in)


def linear_bf16_fusion_pays(F_in, F_out):
    """The 'auto' rule of Options.linear_bf16 = 'mfma': linear_fusion_pays' rule, taken over unmeasured.  What decides
    it is which width the aggregation runs at -- folded it gathers F_in-wide rows, unfolded F_out-wide ones -- and that
    ratio is the same at two bytes per element as at four; the table of tools/bf16_linear_probe.py
    (profiles/r12_bf16_linear.md) is what a later change of this rule should be taken from."""
    return linear_fusion_pays(F_in, F_out)


LIN_RELU, LIN_BF16X6 = 1, 2  # include/hg_aggr.h: flags of the linear epilogue


def pack_linear(weight, bf16x6=False):
    """nn.Linear.weight [F_out, F_in] -> the MFMA fragment order hg_aggr_linear_f32 reads
    (hg_linear_pack_ex_f32; one tiny kernel, two with the planes).  Re-pack after every weight update.
    bf16x6: at F_in = 128 the buffer also carries the weight's three bf16 planes (HG_LIN_BF16X6); such a packing serves
    both forms of the matrix phase (aggregate_linear(..., math=)), one without them the fp32 form only."""
    _check_feat(weight, "weight")
    F_out, F_in = weight.shape
    L = _lib.lib()
    flags = LIN_BF16X6 if bf16x6 else 0
    wfrag = torch.empty(max(L.hg_linear_pack_floats(F_out, F_in, flags), F_out * F_in), dtype=torch.float32,
                        device=weight.device)
    with torch.cuda.device(weight.device):
        _lib.check(L.hg_linear_pack_ex_f32(F_out, F_in, _ptr(weight), _ptr(wfrag), flags, _stream_handle(weight.device)))
    return wfrag


_PACK_CACHE = collections.OrderedDict()
_PACK_CACHE_MAX = 64


def packed_linear_cached(weight, bf16x6=False):
    """pack_linear(weight), kept until the weight is replaced or modified in place (data_ptr /
    torch version counter: an optimizer step bumps it): inference re-uses one packing per layer
    instead of launching the pack kernel on every forward."""
    bf16x6 = bool(bf16x6) and weight.shape[1] == 128  # other widths carry no planes: one entry
    key = (weight.data_ptr(), weight._version, tuple(weight.shape), str(weight.device), bf16x6)
    stream = torch.cuda.current_stream(weight.device)
    with _CACHE_LOCK:
        hit = _PACK_CACHE.get(key)
        if hit is not None:
            _PACK_CACHE.move_to_end(key)
    if hit is not None:
        if hit[2] != stream.cuda_stream:  # packed on another stream: order this one behind the pack kernel
            stream.wait_event(hit[3])
        return hit[0]
    packed = pack_linear(weight, bf16x6)
    with torch.cuda.device(weight.device):
        ev = torch.cuda.Event()
        ev.record(stream)
    with _CACHE_LOCK:
        # the weight stays alive: its address cannot be recycled under the key
        _PACK_CACHE[key] = (packed, weight, stream.cuda_stream, ev)
        while len(_PACK_CACHE) > _PACK_CACHE_MAX:
            _PACK_CACHE.popitem(last=False)
    return packed


def clear_pack_cache():
    """Forget every cached packing.  Needed around hipGraph captures that update weights: a replay rewrites the
    weights in place behind torch's version counter, which is part of the cache key."""
    with _CACHE_LOCK:
        _PACK_CACHE.clear()


def linear_rows(X, weight, packed=None, out=None):
    """X . weight^T on the library's own fp32-MFMA rows kernel (hg_linear_rows_f32): for the
    tall-skinny products of this path it is 1.1-1.5x rocBLAS at K <= 64 and on par at K = 128."""
    _check_feat(X, "X")
    _check_feat(weight, "weight", device=X.device)
    F_out, F_in = weight.shape
    if X.dim() != 2 or X.shape[1] != F_in:
        raise ValueError("X must be [rows, F_in = %d]" % F_in)
    if packed is None:
        packed = packed_linear_cached(weight)
    Y = out if out is not None else torch.empty((X.shape[0], F_out), dtype=torch.float32, device=X.device)
    with torch.cuda.device(X.device):
        _lib.check(_lib.lib().hg_linear_rows_f32(X.shape[0], F_in, F_out, _ptr(X), _ptr(packed), _ptr(Y),
                                                 _stream_handle(X.device)))
    return Y


def _check_bf16_weight(weight):
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.bfloat16:
        raise TypeError("weight must be a bfloat16 tensor, got %s" % getattr(weight, "dtype", type(weight)))
    if weight.dim() != 2 or not linear_supported(weight.shape[1], weight.shape[0]):
        raise ValueError("weight must be [F_out, F_in] with F_in in {32, 64, 128} and F_out a positive multiple of 16")
    _check_feat(weight, "weight", bf16_ok=True)


def pack_linear_bf16(weight):
    """A bfloat16 nn.Linear.weight [F_out, F_in] -> the fragment order of the bf16 MFMA (hg_linear_pack_bf16; one tiny
    kernel): what aggregate_linear_bf16 and linear_rows_bf16 read.  Re-pack after every weight update."""
    _check_bf16_weight(weight)
    F_out, F_in = weight.shape
    L = _lib.lib()
    wfrag = torch.empty(max(int(L.hg_linear_pack_bf16_bytes(F_out, F_in)) // 2, 8), dtype=torch.bfloat16, device=weight.device)
    with torch.cuda.device(weight.device):
        _lib.check(L.hg_linear_pack_bf16(F_out, F_in, _ptr(weight), _ptr(wfrag), _stream_handle(weight.device)))
    return wfrag


def packed_linear_bf16_cached(weight):
    """pack_linear_bf16(weight), cached as packed_linear_cached caches the fp32 packings (same key, same cache)."""
    _check_bf16_weight(weight)
    key = (weight.data_ptr(), weight._version, tuple(weight.shape), str(weight.device), "bf16")
    stream = torch.cuda.current_stream(weight.device)
    with _CACHE_LOCK:
        hit = _PACK_CACHE.get(key)
        if hit is not None:
            _PACK_CACHE.move_to_end(key)
    if hit is not None:
        if hit[2] != stream.cuda_stream:  # packed on another stream: order this one behind the pack kernel
            stream.wait_event(hit[3])
        return hit[0]
    packed = pack_linear_bf16(weight)
    with torch.cuda.device(weight.device):
        ev = torch.cuda.Event()
        ev.record(stream)
    with _CACHE_LOCK:
        _PACK_CACHE[key] = (packed, weight, stream.cuda_stream, ev)
        while len(_PACK_CACHE) > _PACK_CACHE_MAX:
            _PACK_CACHE.popitem(last=False)
    return packed


def linear_rows_bf16(X, weight, packed=None, out=None):
    """round_bf16(X . weight^T) for bfloat16 X [rows, F_in] and weight [F_out, F_in] on the library's bf16-MFMA rows kernel
    (hg_linear_rows_bf16): exact products, fp32 accumulation, one rounding."""
    if not isinstance(X, torch.Tensor) or X.dtype != torch.bfloat16:
        raise TypeError("X must be a bfloat16 tensor, got %s" % getattr(X, "dtype", type(X)))
    _check_bf16_weight(weight)
    _check_feat(X, "X", device=weight.device, bf16_ok=True)
    F_out, F_in = weight.shape
    if X.dim() != 2 or X.shape[1] != F_in:
        raise ValueError("X must be [rows, F_in = %d]" % F_in)
    if packed is None:
        packed = packed_linear_bf16_cached(weight)
    if X.data_ptr() % 8 != 0:
        X = X.clone()
    Y = out if out is not None else torch.empty((X.shape[0], F_out), dtype=torch.bfloat16, device=X.device)
    with torch.cuda.device(X.device):
        _lib.check(_lib.lib().hg_linear_rows_bf16(X.shape[0], F_in, F_out, _ptr(X), _ptr(packed), _ptr(Y),
                                                  _stream_handle(X.device)))
    return Y


def wgrad_supported(F_a, F_b):
    """hg_linear_wgrad_f32's shapes: at most sixteen 16 x 16 tiles (one workgroup's accumulators), or both widths
    multiples of 64 up to 512 (64 x 64 blocks of the output)."""
    if F_a <= 0 or F_b <= 0 or F_a % 16 or F_b % 16:
        return False
    if (F_a // 16) * (F_b // 16) <= 16:
        return True
    return F_a % 64 == 0 and F_b % 64 == 0 and F_a <= 512 and F_b <= 512


def linear_wgrad(A, B):
    """A^T . B for A [N, F_a], B [N, F_b] (the linear's weight gradient, hg_linear_wgrad_f32)."""
    _check_feat(A, "A")
    _check_feat(B, "B", device=A.device)
    if A.dim() != 2 or B.dim() != 2 or A.shape[0] != B.shape[0]:
        raise ValueError("A and B must be [N, F_a] and [N, F_b]")
    N, F_a = A.shape
    F_b = B.shape[1]
    nbytes = int(_lib.lib().hg_linear_wgrad_workspace_bytes(N, F_a, F_b))
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=A.device)
    C = torch.empty((F_a, F_b), dtype=torch.float32, device=A.device)
    with torch.cuda.device(A.device):
        _lib.check(_lib.lib().hg_linear_wgrad_f32(N, F_a, F_b, _ptr(A), _ptr(B), _ptr(C), _ptr(ws), nbytes,
                                                  _stream_handle(A.device)))
    return C


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _check_index(t, name):
    # reference: assertTensor(..., torch::kInt32), hgnnaggr_cuda.cu:8-12 -- but raising, not aborting
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise TypeError("%s must be an int32 tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must be on a GPU (no CPU fallback in this backend)" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)


def _bf16_lanes(F, heads, *rows):
    """Whether the bf16 entries of the incidence path take these row arrays (None: absent): whole four-column lanes inside one
    head, bfloat16 data 8-byte and float32 data 16-byte aligned (include/hg_aggr.h)."""
    if F % 4 or (F // heads) % 4:
        return False
    return all(t is None or t.data_ptr() % (8 if t.dtype == torch.bfloat16 else 16) == 0 for t in rows)


def _check_scales(pairs, device):
    """pairs of (name, tensor or None, elements): every tensor given is a float32 feature tensor on `device` of that size."""
    for name, t, n in pairs:
        if t is not None:
            _check_feat(t, name, device=device)
            if t.numel() != n:
                raise ValueError("%s must have %d elements, got %d" % (name, n, t.numel()))


def _check_feat(t, name, device=None, bf16_ok=False):
    if not isinstance(t, torch.Tensor) or not (t.dtype == torch.float32 or (bf16_ok and t.dtype == torch.bfloat16)):
        raise TypeError("%s must be a float32%s tensor" % (name, " or bfloat16" if bf16_ok else ""))
    if not t.is_cuda:
        raise RuntimeError("%s must be on a GPU (no CPU fallback in this backend)" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    if device is not None and t.device != device:
        raise RuntimeError("%s is on %s, expected %s" % (name, t.device, device))


# The attention dropout's state, int64 [2] = {key, sid}: the three refusals in the order every layer makes them (ops.
# _segment_args interleaves them with those of the other arguments).
def _rng_state_dtype(t):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
        raise TypeError("rng_state must be an int64 tensor of 2 elements {key, sid}, got %s" % (getattr(t, "dtype", type(t)),))


def _rng_state_length(t):
    if t.numel() != 2:
        raise ValueError("rng_state must have 2 elements {key, sid}, got %d" % t.numel())


def _rng_state_device(t, device=None):
    if not t.is_cuda:
        raise RuntimeError("rng_state must be on a GPU (no CPU fallback in this backend)")
    if not t.is_contiguous():
        raise RuntimeError("rng_state must be contiguous")
    if device is not None and t.device != device:
        raise RuntimeError("rng_state is on %s, expected %s" % (t.device, device))


# ------------------------------------------------------------------ plan cache
_CACHE = collections.OrderedDict()
_CACHE_MAX = 32
_DEFAULT_OPTS = None


def set_default_opts(opts):
    """Plan options used by plans created through the cache; clears the cache."""
    global _DEFAULT_OPTS
    with _CACHE_LOCK:
        _DEFAULT_OPTS = opts
        _CACHE.clear()


def cached_plan(N, csrptr_t, colind_t):
    """Plan for the hypergraph held in these two device tensors.  The key pins
    storage address, length, device and torch's in-place version counter; the
    entry keeps the tensors alive so an address cannot be recycled under it."""
    key = (N, csrptr_t.data_ptr(), csrptr_t.numel(), csrptr_t._version,
           colind_t.data_ptr(), colind_t.numel(), colind_t._version, str(csrptr_t.device))
    with _CACHE_LOCK:
        hit = _CACHE.get(key)
        if hit is not None:
            _CACHE.move_to_end(key)
            return hit[0]
    plan = Plan.from_tensors(N, csrptr_t, colind_t, _DEFAULT_OPTS)
    with _CACHE_LOCK:
        _CACHE[key] = (plan, csrptr_t, colind_t)
        while len(_CACHE) > _CACHE_MAX:
            _CACHE.popitem(last=False)
    return plan


def clear_plan_cache():
    with _CACHE_LOCK:
        _CACHE.clear()
