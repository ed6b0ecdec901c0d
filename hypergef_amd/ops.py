"""Operator surface of the reference, on the MI355X backend.

Mirrors, name for name and argument for argument:
  * the pybind modules `hgnnaggr` (HyperGsys/source/hgnnaggr/hgnnaggr.cc:122-151)
    and `unignnaggr` (HyperGsys/source/unignnaggr/unignnaggr.cc:81-102) --
    exposed as `hypergef_amd.hgnnaggr` / `hypergef_amd.unignnaggr` and, after
    `hypergef_amd.install_dropin()`, as top-level `hgnnaggr` / `unignnaggr`;
  * the Python wrappers `HGNNAggr`, `UniGNNConvdeg`, `UniGNNConv`
    (HyperGsys/source/python/hgnnaggr.py:6-7, unignnconv.py:6-10).

The four schedule tensors (`balan_key, balan_row, group_st, group_ed`) stay in
the signatures.  The default kernels derive their own wave64 schedule from
`csrptr_t` / `indices_t` (cached per hypergraph); with
`set_variant("push_groups")` the reference's own scheme runs on exactly the
tasks those tensors describe.

Backward: the reference returns `forward(grad_out)` for every sum operator
(hgnnaggr.cc:51-64, unignnaggr.cc:36-49, 65-78).  That equals the true adjoint
only when degV is absent; `set_backward("adjoint")` selects
H diag(degE W) H^T diag(degV) grad instead.  Default: "reference".
"""
import torch

from . import _lib
from .knn_graph import knn, knn_incidence_weights  # noqa: F401  (ops.knn / ops.knn_incidence_weights)
from .knn_graph import knn_aggr, knn_dist, knn_transpose  # noqa: F401  (ops.knn_aggr / ops.knn_transpose: no plan, no host step)
from .plan import (cached_plan, linear_bf16_fusion_pays, linear_fusion_pays, linear_rows, linear_supported, linear_wgrad,
                   wgrad_supported, _check_feat, _check_index, _ptr, _rng_state_device, _rng_state_dtype,
                   _rng_state_length, _stream_handle)

import contextlib
import numbers
import dataclasses
import os as _os
import threading


@dataclasses.dataclass(frozen=True)
class Options:
    """How one operator call runs: kernel family, backward rule, linear folding.

    variant:     'auto' | 'pull' | 'fused' | 'push_atomic' (one task per hyperedge) | 'push_groups'
                 (the caller's group_* tensors drive the push kernel).
    backward:    'reference' (forward(grad_out), hgnnaggr.cc:51-64) | 'adjoint' (the exact transpose).
    fuse_linear: 'auto' folds a layer's projection into the aggregation where that is faster
                 (plan.linear_fusion_pays), 'always' wherever the kernel takes the widths, 'never' not.
    linear_math: 'f32' = the folded projection on fp32 MFMA; 'bf16x6' = at F_in = 128 each fp32 product as six bf16
                 products on the bf16 MFMA (HG_LIN_BF16X6, include/hg_aggr.h): the same error bound, 3/8 of the matrix-pipe
                 cycles.  Forward of the fused layer only; every other width and kernel stays fp32 MFMA.
    linear_bf16: how a bfloat16 layer's linear runs.  'torch' = torch's GEMM around the bf16 aggregation; 'mfma' = folded
                 into the aggregation on the bf16 MFMA (hg_aggr_linear_res_bf16: fp32 accumulation, one rounding of the
                 combined row and one of the result) wherever fuse_linear folds -- 'always' at every supported width,
                 'auto' under plan.linear_bf16_fusion_pays; variants auto, pull and fused.  float32 layers ignore it.
    incidence_bf16: what the incidence operators do with bfloat16 feature rows.  'refuse' = the TypeError they always
                 raised; 'rows' = incidence_aggr / HGNNAggrIncidence, incidence_gather and incidence_dot take bfloat16
                 node_feat / src / A / B on the library's bf16-row kernels (hg_aggr_incidence_heads_bf16 and its
                 neighbours): fp32 sums in the float32 call's order, one rounding of a bfloat16 result.  The weights, scales
                 and the dot's result stay float32; incidence_softmax, incidence_sum, incidence_attention_aggr and
                 hyperedge_dot stay float32 only.

    Every operator resolves its options per call -- an explicit `options=` argument, else the innermost
    `with ops.options(...)` block of the calling thread, else the process defaults -- and an autograd node keeps
    the options of its forward for its backward, whichever thread runs it.  Two models in one process can
    therefore differ; nothing is shared but the defaults."""
    variant: str = "auto"
    backward: str = "reference"
    fuse_linear: str = "auto"
    linear_math: str = "f32"
    linear_bf16: str = "torch"
    incidence_bf16: str = "refuse"

    _CHOICES = {"variant": ("auto", "pull", "fused", "push_atomic", "push_groups"),
                "backward": ("reference", "adjoint"), "fuse_linear": ("auto", "always", "never"),
                "linear_math": ("f32", "bf16x6"), "linear_bf16": ("torch", "mfma"),
                "incidence_bf16": ("refuse", "rows")}

    def __post_init__(self):
        for k, allowed in Options._CHOICES.items():
            if getattr(self, k) not in allowed:
                raise ValueError("%s must be one of %s, got %r" % (k, ", ".join(allowed), getattr(self, k)))

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


_DEFAULTS_LOCK = threading.Lock()
_DEFAULTS = Options(fuse_linear=_os.environ["HG_FUSE_LINEAR"]
                    if _os.environ.get("HG_FUSE_LINEAR") in ("auto", "always", "never") else "auto",  # A/B runs of the drivers
                    linear_math=_os.environ["HG_LINEAR_MATH"]
                    if _os.environ.get("HG_LINEAR_MATH") in ("f32", "bf16x6") else "f32",
                    linear_bf16=_os.environ["HG_LINEAR_BF16"]
                    if _os.environ.get("HG_LINEAR_BF16") in ("torch", "mfma") else "torch",
                    incidence_bf16=_os.environ["HG_INCIDENCE_BF16"]
                    if _os.environ.get("HG_INCIDENCE_BF16") in ("refuse", "rows") else "refuse")
_TLS = threading.local()


def current_options():
    """The options a call made here, now, without an explicit `options=` would run with."""
    stack = getattr(_TLS, "stack", None)
    return stack[-1] if stack else _DEFAULTS


@contextlib.contextmanager
def options(**kw):
    """`with ops.options(variant="pull", backward="adjoint"):` -- per-thread, nestable overrides."""
    stack = getattr(_TLS, "stack", None)
    if stack is None:
        stack = _TLS.stack = []
    stack.append(current_options().replace(**kw))
    try:
        yield stack[-1]
    finally:
        stack.pop()


def _opt(o):
    if o is None:
        return current_options()
    if not isinstance(o, Options):
        raise TypeError("options must be an ops.Options")
    return o


def _set_default(**kw):
    global _DEFAULTS
    with _DEFAULTS_LOCK:
        _DEFAULTS = _DEFAULTS.replace(**kw)


def set_variant(name):
    """Process default of Options.variant (see there)."""
    _set_default(variant=name)


def set_backward(mode):
    """Process default of Options.backward."""
    _set_default(backward=mode)


def set_fuse_linear(mode):
    """Process default of Options.fuse_linear."""
    _set_default(fuse_linear=mode)


def set_linear_math(mode):
    """Process default of Options.linear_math."""
    _set_default(linear_math=mode)


def set_linear_bf16(mode):
    """Process default of Options.linear_bf16."""
    _set_default(linear_bf16=mode)


def set_incidence_bf16(mode):
    """Process default of Options.incidence_bf16."""
    _set_default(incidence_bf16=mode)


def _rows_dtype_ok(t, opt):
    """float32, or bfloat16 feature rows where Options.incidence_bf16 = 'rows' lets the incidence operators take them."""
    return isinstance(t, torch.Tensor) and (t.dtype == torch.float32 or
                                            (opt.incidence_bf16 == "rows" and t.dtype == torch.bfloat16))


def _flat(t):
    # degE / degV / W are read as flat arrays: [M] and [M,1] both valid
    return None if t is None else t.reshape(-1)


def _heads(heads):
    """The `heads` keyword as an int >= 1: ValueError otherwise, before any tensor is looked at."""
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError("heads must be an integer >= 1, got %r" % (heads,))
    return heads


def _per_head(t, heads):
    """A per-item array with `heads` columns as [*, heads] where its element count allows it (a wrong count is kept as it
    is and refused by the length checks)."""
    return t.reshape(-1, heads) if t.numel() % heads == 0 else t


def _times_degV(g, degV):
    """g * degV per row (the adjoint backward's input).  A bf16 g is multiplied in fp32 and rounded to bf16 once: torch
    would promote the product to fp32 and send the backward through the fp32 kernels."""
    if g.dtype == torch.bfloat16:
        return (g.float() * degV.reshape(-1, 1)).to(torch.bfloat16)
    return g * degV.reshape(-1, 1)


def _any_requires_grad(*tensors):
    return any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _forward(sched, csrptr_t, indices_t, node_feat, degE, degV, W, opt):
    # looked at before the scales are flattened: inside an autograd Function grad mode is off and a reshaped view of a
    # trainable tensor no longer says that it requires a gradient
    trainable = _any_requires_grad(degE, degV, W)
    _check_feat(node_feat, "node_feat", bf16_ok=True)
    _check_index(csrptr_t, "csrptr_t")
    _check_index(indices_t, "indices_t")
    if node_feat.dim() != 2:
        raise ValueError("node_feat must be [N, F]")
    N, F = node_feat.shape
    degE, degV, W = _flat(degE), _flat(degV), _flat(W)
    variant = opt.variant
    if node_feat.dtype == torch.bfloat16 and variant in ("push_atomic", "push_groups"):
        raise TypeError("bfloat16 node_feat: the %s kernels are fp32 only (use auto, fused or pull)" % variant)
    if variant == "push_groups":
        key, row, st, ed = sched
        for n, t in (("balan_key", key), ("balan_row", row), ("group_st", st), ("group_ed", ed)):
            _check_index(t, n)
        M = csrptr_t.numel() - 1
        for name, t, n in (("degE", degE, M), ("degV", degV, N), ("W", W, M)):
            if t is not None:
                _check_feat(t, name, device=node_feat.device)
                if t.numel() != n:
                    raise ValueError("%s must have %d elements" % (name, n))
        Y = torch.empty((N, F), dtype=torch.float32, device=node_feat.device)
        with torch.cuda.device(node_feat.device):
            _lib.check(_lib.lib().hg_aggr_push_groups_f32(
                N, M, F, row.numel(), _ptr(key), _ptr(row), _ptr(st), _ptr(ed),
                _ptr(csrptr_t), _ptr(indices_t), _ptr(node_feat), _ptr(degE), _ptr(degV), _ptr(W),
                _ptr(Y), _stream_handle(node_feat.device)))
        return Y
    plan = cached_plan(N, csrptr_t, indices_t)
    return plan.aggregate(csrptr_t, indices_t, node_feat, degE, degV, W, variant=variant, trainable_scales=trainable)


def _edge_scale_grads(plan, csrptr_t, q, degE, W, need_e, need_w):
    """(ddegE, dW) from q[e] = <S[e], Ge[e]> (Plan.hyperedge_dot): ddegE = q * W, dW = q * degE, the absent partner being
    the factor 1.  An empty hyperedge has q = +0 exactly and a partner that may be inf (degE = 1 / |e|): the partner is
    taken as 0 there, so no 0 * inf is formed and both gradients are exactly 0."""
    live = plan.nonempty_edges(csrptr_t)
    gE = gW = None
    if need_e:
        gE = (q if W is None else q * _flat(W).masked_fill(~live, 0.0)).view_as(degE)
    if need_w:
        gW = (q if degE is None else q * _flat(degE).masked_fill(~live, 0.0)).view_as(W)
    return gE, gW


def _sum_scale_grads(csrptr_t, indices_t, X, dY, degE, degV, W, need, opt):
    """Exact gradients (ddegE, ddegV, dW) of Y = degV . H (degE . W . (H^T X)) for its gradient dY, each where `need` asks:
    q[e] = <sum_{u in e} X[u], sum_{v in e} degV[v] dY[v]> in one kernel (Plan.hyperedge_dot; neither [M, F] table is
    written), ddegV[v] = <dY[v], Z[v]> with Z the aggregation without degV (Plan.rows_dot).  They run on the cached plan
    whatever variant the forward took.  bf16 rows are widened here (the two kernels are fp32); the results are fp32."""
    need_e, need_v, need_w = need
    plan = cached_plan(X.shape[0], csrptr_t, indices_t)
    dY32 = dY.float()
    gE = gV = gW = None
    if need_e or need_w:
        P = dY32 if degV is None else dY32 * _flat(degV).reshape(-1, 1)
        q = plan.hyperedge_dot(csrptr_t, indices_t, X.detach().float().contiguous(), P)
        gE, gW = _edge_scale_grads(plan, csrptr_t, q, degE, W, need_e, need_w)
    if need_v:
        variant = opt.variant if opt.variant in ("auto", "pull", "fused") else "auto"
        Z = plan.aggregate(csrptr_t, indices_t, X.detach(), _flat(degE), None, _flat(W), variant=variant,
                           trainable_scales=True)  # this code runs only where a scale is trainable
        gV = plan.rows_dot(dY32, Z.float()).view_as(degV)
    return gE, gV, gW


class _SumAggr(torch.autograd.Function):
    """One autograd node for all three sum operators (degE/degV/W optional).  degE, degV and W get their exact gradients
    where they require one (_sum_scale_grads), under both Options.backward rules: that option chooses dX's rule only."""

    @staticmethod
    def forward(ctx, balan_key, balan_row, group_st, group_ed, csrptr_t, indices_t, node_feat,
                degE, degV, W, opt=None):
        opt = ctx.opt = _opt(opt)
        out = _forward((balan_key, balan_row, group_st, group_ed), csrptr_t, indices_t, node_feat,
                       degE, degV, W, opt)
        # The reference saves its inputs the same way (hgnnaggr.cc:44-46); node_feat is not needed for dX
        # (the operator is linear) and is kept only where a scale wants a gradient.  save_for_backward makes
        # autograd raise if one of them is modified in place between forward and backward.
        keep_x = any(t is not None and ctx.needs_input_grad[i] for i, t in ((7, degE), (8, degV), (9, W)))
        ctx.save_for_backward(balan_key, balan_row, group_st, group_ed, csrptr_t, indices_t, degE, degV, W,
                              node_feat if keep_x else None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        grad_out = grad_out.contiguous()
        balan_key, balan_row, group_st, group_ed, csrptr_t, indices_t, degE, degV, W, X = ctx.saved_tensors
        sched = (balan_key, balan_row, group_st, group_ed)
        g = None
        if ctx.needs_input_grad[6]:
            if ctx.opt.backward == "reference" or degV is None:
                g = _forward(sched, csrptr_t, indices_t, grad_out, degE, degV, W, ctx.opt)
            else:
                g = _forward(sched, csrptr_t, indices_t, _times_degV(grad_out, degV), degE, None, W, ctx.opt)
        gE = gV = gW = None
        if X is not None:
            need = tuple(t is not None and ctx.needs_input_grad[i] for i, t in ((7, degE), (8, degV), (9, W)))
            gE, gV, gW = _sum_scale_grads(csrptr_t, indices_t, X, grad_out, degE, degV, W, need, ctx.opt)
        return (None,) * 6 + (g, gE, gV, gW, None)


def _rows_times(A, B, mode="auto"):
    """A . B for tall-skinny A [N, K], B [K, F]: the library's MFMA rows kernel where it takes the
    widths (1.4-1.5x rocBLAS at K <= 64), torch otherwise.  Backward-pass GEMMs use it."""
    K, F = B.shape
    if mode != "never" and A.is_cuda and A.dtype == B.dtype == torch.float32 and linear_supported(K, F) and A.shape[0] >= 4096:
        return linear_rows(A.contiguous(), B.t().contiguous())
    return A @ B


def _pad16(t):
    pad = (-t.shape[1]) % 16
    return t if pad == 0 else torch.nn.functional.pad(t, (0, pad))


def _wgrad(A, B, mode="auto"):
    """A^T . B over the vertices (the linear's weight gradient): the library's streaming MFMA kernel
    where it takes the widths -- rocBLAS needs 1.2 ms for [64 x 693 k] x [693 k x 64], 17x the time of
    reading the operands -- torch otherwise."""
    if mode != "never" and A.is_cuda and A.dtype == B.dtype == torch.float32 and A.shape[0] >= 4096:
        Fa, Fb = A.shape[1], B.shape[1]
        if wgrad_supported(Fa, Fb):
            return linear_wgrad(A.contiguous(), B.contiguous())
        Pa, Pb = Fa + (-Fa) % 16, Fb + (-Fb) % 16
        if wgrad_supported(Pa, Pb):  # e.g. the class-count layer: pad to the next 16 columns, cut the result
            return linear_wgrad(_pad16(A).contiguous(), _pad16(B).contiguous())[:Fa, :Fb]
    return A.t() @ B


class _LinearFn(torch.autograd.Function):
    """torch.nn.functional.linear with this library's weight-gradient kernel in the backward
    (x^T-style contraction over the vertices; see _wgrad)."""

    @staticmethod
    def forward(ctx, x, weight, bias, opt=None):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.mode = _opt(opt).fuse_linear  # the owning module's pinned Options, else the caller's (thread, process)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, grad):
        x, weight = ctx.saved_tensors
        grad = grad.contiguous()
        gx = _rows_times(grad, weight, ctx.mode) if ctx.needs_input_grad[0] else None
        gw = _wgrad(grad, x, ctx.mode) if ctx.needs_input_grad[1] else None
        gb = grad.sum(0) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return gx, gw, gb, None


class Linear(torch.nn.Linear):
    """Drop-in nn.Linear (same parameters, same state_dict) for the [N, F] activations of these
    models: identical forward, weight gradient on hg_linear_wgrad_f32.  `options` (an ops.Options, or None for the
    caller's) pins what the backward may use, like the conv modules' own: a model built with
    Options(fuse_linear="never") keeps its linears off the library's MFMA kernels too."""

    def __init__(self, in_features, out_features, bias=True, device=None, dtype=None, options=None):
        super().__init__(in_features, out_features, bias=bias, device=device, dtype=dtype)
        if options is not None and not isinstance(options, Options):
            raise TypeError("options must be an ops.Options")
        self.options = options

    def forward(self, x):
        if x.dim() == 2 and x.is_cuda and x.dtype == torch.float32:
            return _LinearFn.apply(x, self.weight, self.bias, self.options)
        return super().forward(x)


class _SumAggrLinear(torch.autograd.Function):
    """Aggr(X . Wlin^T) as one node: the layer's bias-free nn.Linear followed by the sum
    aggregation (HyperGsysHGNN.forward, model/ugsys/hgnn.py:22-23; HyperGsysUinGINConv.forward,
    unigin.py:20-21).  Forward runs hg_aggr_linear_f32 -- aggregate the F_in-wide rows, multiply
    each finished row by Wlin^T on the matrix cores -- when the widths allow, else the two steps.
    Backward is the two-step one: dZ = aggregation backward of grad_out (reference or adjoint
    mode, as _SumAggr), dX = dZ . Wlin, dWlin = dZ^T . X.  degE / degV / W get their exact gradients where they require
    one: _sum_scale_grads on (X, dT) at F_in, dT = dY . Wlin the gradient of the aggregated rows."""

    @staticmethod
    def forward(ctx, csrptr_t, indices_t, node_feat, weight, degE, degV, W, opt=None):
        opt = ctx.opt = _opt(opt)
        _check_feat(node_feat, "node_feat", bf16_ok=True)
        _check_feat(weight, "weight", device=node_feat.device, bf16_ok=True)
        _check_index(csrptr_t, "csrptr_t")
        _check_index(indices_t, "indices_t")
        if node_feat.dim() != 2 or weight.dim() != 2 or weight.shape[1] != node_feat.shape[1]:
            raise ValueError("node_feat must be [N, F_in] and weight [F_out, F_in]")
        if weight.dtype != node_feat.dtype:
            raise TypeError("weight must have node_feat's dtype %s, got %s" % (node_feat.dtype, weight.dtype))
        f32 = node_feat.dtype == torch.float32  # bf16: torch's GEMM, then the bf16 aggregation, unless linear_bf16 = 'mfma'
        mfma16 = not f32 and opt.linear_bf16 == "mfma"  # the linear folded in on the bf16 MFMA (hg_aggr_linear_res_bf16)
        ctx.scale_shapes = tuple(None if t is None else t.shape for t in (degE, degV, W))
        trainable = ctx.trainable = _any_requires_grad(degE, degV, W)  # before flattening: see _forward
        degE, degV, W = _flat(degE), _flat(degV), _flat(W)
        N, F_in = node_feat.shape
        F_out = weight.shape[0]
        variant = opt.variant
        plan = cached_plan(N, csrptr_t, indices_t)
        mode = opt.fuse_linear
        fuse = (f32 or mfma16) and ((mode == "always" and linear_supported(F_in, F_out)) or
                                    (mode == "auto" and (linear_fusion_pays if f32 else linear_bf16_fusion_pays)(F_in, F_out)))
        if fuse and mfma16 and variant in ("auto", "pull", "fused"):
            out = plan.aggregate_linear_bf16(csrptr_t, indices_t, node_feat.contiguous(), weight.detach().contiguous(),
                                             degE, degV, W, variant=variant, trainable_scales=trainable)
        elif fuse and variant in ("auto", "pull", "fused"):
            out = plan.aggregate_linear(csrptr_t, indices_t, node_feat, weight.detach().contiguous(),
                                        degE, degV, W, variant=variant, math=opt.linear_math, trainable_scales=trainable)
        else:  # project, then aggregate at F_out (own MFMA rows kernel where it takes the widths)
            wd = weight.detach().contiguous()
            Z = linear_rows(node_feat, wd) if f32 and linear_supported(F_in, F_out) and mode != "never" \
                else torch.nn.functional.linear(node_feat, wd)
            out = _SumAggrLinear._aggr(csrptr_t, indices_t, Z, degE, degV, W, opt, trainable)
        ctx.save_for_backward(node_feat, weight, csrptr_t, indices_t, degE, degV, W)
        return out

    @staticmethod
    def _aggr(csrptr_t, indices_t, feat, degE, degV, W, opt, trainable=False):
        # this operator has no group_* tensors: "push_groups" falls back to the plan's own schedule
        variant = opt.variant if opt.variant != "push_groups" else "auto"
        plan = cached_plan(feat.shape[0], csrptr_t, indices_t)
        return plan.aggregate(csrptr_t, indices_t, feat.contiguous(), degE, degV, W, variant=variant,
                              trainable_scales=trainable or _any_requires_grad(degE, degV, W))

    @staticmethod
    def backward(ctx, grad_out):
        grad_out = grad_out.contiguous()
        node_feat, weight, csrptr_t, indices_t, degE, degV, W = ctx.saved_tensors
        opt = ctx.opt
        if opt.backward == "reference" or degV is None:
            dZ = _SumAggrLinear._aggr(csrptr_t, indices_t, grad_out, degE, degV, W, opt, ctx.trainable)
        else:
            dZ = _SumAggrLinear._aggr(csrptr_t, indices_t, _times_degV(grad_out, degV), degE, None, W, opt, ctx.trainable)
        gx = _rows_times(dZ, weight, opt.fuse_linear) if ctx.needs_input_grad[2] else None
        gw = _wgrad(dZ, node_feat, opt.fuse_linear) if ctx.needs_input_grad[3] else None
        gE = gV = gW = None
        need = tuple(t is not None and ctx.needs_input_grad[i] for i, t in ((4, degE), (5, degV), (6, W)))
        if any(need):
            # Y = Aggr(X) . Wlin^T: with dT = dY . Wlin, the gradient of the aggregated rows, the scales see the plain
            # aggregation of X at F_in and its gradient dT
            dT = _rows_times(grad_out, weight.detach(), opt.fuse_linear)
            gE, gV, gW = (g if g is None else g.reshape(shape) for g, shape in zip(
                _sum_scale_grads(csrptr_t, indices_t, node_feat, dT.contiguous(), degE, degV, W, need, opt),
                ctx.scale_shapes))  # the saved scales are the flattened ones: give each gradient its input's shape
        return None, None, gx, gw, gE, gV, gW, None


# ca folds into M (backward of _AggrResLinear) only inside [2^-64, 2^64]: there M * ca and cb / ca stay far inside fp32's normal
# range (2^-126 .. 2^128) for weights and mixing factors of any ordinary size, so nothing flushes to zero or overflows
_FOLD_MIN, _FOLD_MAX = 2.0 ** -64, 2.0 ** 64


class _AggrResLinear(torch.autograd.Function):
    """Y = act((ca * Aggr(X) + cb * R) . M^T): a whole UniGNN layer as one node
    (hg_aggr_linear_res_f32).  UniGCNII (model/ugsys/unigcnii.py:19-21 + the relu of model/gnn.py:199):
    ca = 1 - alpha, cb = alpha, R = X0, M = (1 - beta) I + beta W.  UniGIN (unigin.py:20-22):
    ca = 1, cb = 1 + eps, R = X, M = W.  Falls back to the same formula in torch ops around the
    plain aggregation where the MFMA epilogue does not take the widths.  Backward: dP = dY (masked by
    the relu), dT = dP . M, dM = dP^T . T, dX = ca * (aggregation backward of dT), dR = cb * dT,
    dcb = <dT, R> (cb may be a tensor, e.g. 1 + eps).  degE / degV / W get no gradient from this node (the scale gradients
    of _SumAggr / _SumAggrLinear / _IncidenceAggr are not wired in here)."""

    @staticmethod
    def forward(ctx, csrptr_t, indices_t, node_feat, M, R, cb, degE, degV, W, ca, relu, need_t, opt=None):
        opt = ctx.opt = _opt(opt)
        _check_feat(node_feat, "node_feat", bf16_ok=True)
        _check_index(csrptr_t, "csrptr_t")
        _check_index(indices_t, "indices_t")
        degE, degV, W = _flat(degE), _flat(degV), _flat(W)
        N, F_in = node_feat.shape
        F_out = M.shape[0]
        f32 = node_feat.dtype == torch.float32  # bf16: the torch form around the bf16 aggregation, unless linear_bf16 = 'mfma'
        mfma16 = not f32 and opt.linear_bf16 == "mfma" and M.dtype == node_feat.dtype and (R is None or R.dtype == node_feat.dtype)
        # cb is a Python float except where it is learned (UniGIN's 1 + eps): then it stays on the device -- the
        # kernel reads it there (hg_aggr_linear_res_dev_f32), nothing is read back, and the step can be captured
        if R is None:
            cbf = 0.0
        elif isinstance(cb, torch.Tensor):
            cbf = cb.detach().to(torch.float32 if f32 else node_feat.dtype).reshape(1).contiguous()
        else:
            cbf = float(cb)
        variant = opt.variant if opt.variant != "push_groups" else "auto"
        Md = M.detach().contiguous()
        Rd = None if R is None else R.detach().contiguous()
        mode = opt.fuse_linear
        fuse = (f32 or mfma16) and ((mode == "always" and linear_supported(F_in, F_out)) or
                                    (mode == "auto" and (linear_fusion_pays if f32 else linear_bf16_fusion_pays)(F_in, F_out)))
        if fuse and mfma16 and variant in ("auto", "pull", "fused"):
            plan = cached_plan(N, csrptr_t, indices_t)
            T = torch.empty_like(node_feat, memory_format=torch.contiguous_format) if need_t else None  # bf16: the kernel's T_out
            # the kernel reads a learned cb as a float32 device scalar; the backward keeps cbf, the layer's own dtype, as the torch form
            cbk = cb.detach().to(torch.float32).reshape(1).contiguous() if (R is not None and isinstance(cb, torch.Tensor)) else cbf
            out = plan.aggregate_linear_bf16(csrptr_t, indices_t, node_feat.detach().contiguous(), Md, degE, degV, W,
                                             variant=variant, residual=Rd, ca=ca, cb=cbk, relu=relu, t_out=T)
        elif fuse and variant in ("auto", "pull", "fused"):
            plan = cached_plan(N, csrptr_t, indices_t)
            T = torch.empty_like(node_feat) if need_t else None
            out = plan.aggregate_linear(csrptr_t, indices_t, node_feat.detach(), Md, degE, degV, W, variant=variant,
                                        residual=Rd, ca=ca, cb=cbf, relu=relu, t_out=T, math=opt.linear_math)
        else:
            T = _SumAggrLinear._aggr(csrptr_t, indices_t, node_feat.detach(), degE, degV, W, opt) * ca
            if Rd is not None:
                T = T + Rd * cbf
            out = T @ Md.t()
            if relu:
                out = torch.relu(out)
        ctx.consts = (ca, cbf, relu)
        ctx.save_for_backward(M, R, T, out, csrptr_t, indices_t, degE, degV, W)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        M, R, T, out, csrptr_t, indices_t, degE, degV, W = ctx.saved_tensors
        ca, cbf, relu = ctx.consts
        dP = grad_out.contiguous()
        if relu:
            dP = torch.ops.aten.threshold_backward(dP, out, 0.0)  # relu's own backward: one vectorised kernel
        opt = ctx.opt
        need_gcb = R is not None and ctx.needs_input_grad[5]
        # dX wants ca * (dP . M): the factor rides in the [F_out, F_in] matrix (one tiny kernel) instead of an [N, F] pass over
        # the product, unless the unscaled product is needed for d cb (UniGIN, where ca = 1 anyway) or ca cannot be divided
        # out again for dR (zero, or so small that M * ca or cb / ca leaves fp32's normal range)
        fold = ctx.needs_input_grad[2] and not need_gcb and ca != 1.0 and _FOLD_MIN <= abs(ca) <= _FOLD_MAX
        dT = _rows_times(dP, M * ca if fold else M, opt.fuse_linear)
        gM = _wgrad(dP, T, opt.fuse_linear) if ctx.needs_input_grad[3] else None
        gx = None
        if ctx.needs_input_grad[2]:
            if opt.backward == "reference" or degV is None:
                gx = _SumAggrLinear._aggr(csrptr_t, indices_t, dT, degE, degV, W, opt)
            else:
                gx = _SumAggrLinear._aggr(csrptr_t, indices_t, _times_degV(dT, degV), degE, None, W, opt)
            if not fold and ca != 1.0:  # UniGIN: ca = 1 -- no [N, F] kernel for a multiplication by one
                gx = gx * ca  # after the aggregation: a subnormal ca rounds once, at the end
        gR = None
        if R is not None and ctx.needs_input_grad[4]:
            cbr = cbf / ca if fold else cbf  # a folded dT carries ca
            gR = dT if (not isinstance(cbr, torch.Tensor) and cbr == 1.0) else dT * cbr
        gcb = (dT * R).sum() if need_gcb else None
        return None, None, gx, gM, gR, gcb, None, None, None, None, None, None, None


def aggr_res_linear(csrptr_t, indices_t, node_feat, M, residual=None, ca=1.0, cb=0.0, degE=None, degV=None, W=None,
                    relu=False, options=None):
    """act((ca * Aggr(node_feat) + cb * residual) . M^T) in one pass where the widths allow
    (include/hg_aggr.h, hg_aggr_linear_res_f32).  cb may be a tensor (its gradient is returned)."""
    # a Python-number cb goes through as it is (no host-to-device copy, no sync to read it back)
    cb_a = cb if isinstance(cb, torch.Tensor) else float(cb)
    # T (the rows before the product) is written only if a backward pass can follow: Function.forward
    # itself always runs with grad mode off and needs_input_grad set, so decide here
    need_t = torch.is_grad_enabled() and any(
        isinstance(t, torch.Tensor) and t.requires_grad for t in (node_feat, M, residual, cb_a))
    return _AggrResLinear.apply(csrptr_t, indices_t, node_feat, M, residual, cb_a, degE, degV, W, float(ca),
                                bool(relu), need_t, _opt(options))


def hgnnaggr_linear(csrptr_t, indices_t, node_feat, weight, degE=None, degV=None, W=None, options=None):
    """Aggr(node_feat . weight^T) with the projection folded into the aggregation
    (include/hg_aggr.h, hg_aggr_linear_f32).  degE / degV / W optional: all three = hgnnaggr,
    degE + degV = unignnaggrdeg, none = unignnaggr."""
    return _SumAggrLinear.apply(csrptr_t, indices_t, node_feat, weight, degE, degV, W, _opt(options))


# ---- incidence-weighted aggregation (include/hg_aggr.h, hg_aggr_incidence_f32) ----------------------------------------

def _incidence_args(csrptr_t, indices_t, node_feat, v2e, e2v, opt, heads=1):
    """Argument checks of incidence_aggr, in an order that decides every refusal before a device is touched: variant,
    heads, dtypes, shapes and lengths, then where the tensors live."""
    if opt.variant not in ("auto", "pull"):
        raise ValueError("incidence_aggr runs the pull kernels: variant must be 'auto' or 'pull', got %r" % opt.variant)
    _heads(heads)
    for name, t in (("node_feat", node_feat), ("v2e_weight", v2e), ("e2v_weight", e2v)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32) \
                and not (name == "node_feat" and _rows_dtype_ok(t, opt)):  # Options.incidence_bf16 = 'rows': bf16 rows, never weights
            raise TypeError("%s must be a float32 tensor (incidence_aggr has no bfloat16 form), got %s"
                            % (name, getattr(t, "dtype", type(t))))
    if node_feat.dim() != 2:
        raise ValueError("node_feat must be [N, F]")
    if node_feat.shape[1] % heads:
        raise ValueError("node_feat's width %d is no multiple of heads = %d" % (node_feat.shape[1], heads))
    if not isinstance(indices_t, torch.Tensor):
        raise TypeError("indices_t must be an int32 tensor")
    nnz = indices_t.numel()
    for name, t in (("v2e_weight", v2e), ("e2v_weight", e2v)):
        if t is not None and t.numel() != nnz * heads:
            if heads == 1:
                raise ValueError("%s must have one weight per incidence (nnz = %d), got %d" % (name, nnz, t.numel()))
            raise ValueError("%s must have one weight per incidence and head (nnz * heads = %d), got %d"
                             % (name, nnz * heads, t.numel()))
    _check_index(csrptr_t, "csrptr_t")
    _check_index(indices_t, "indices_t")
    _check_feat(node_feat, "node_feat", bf16_ok=opt.incidence_bf16 == "rows")
    for name, t in (("v2e_weight", v2e), ("e2v_weight", e2v)):
        if t is not None:
            _check_feat(t, name, device=node_feat.device)


class _IncidenceAggr(torch.autograd.Function):
    """Y = Dv H_e2v De W H_v2e^T X with a weight per incidence, and its exact gradients for X and both weight arrays.
    With P = degV * dY:  G = the same call on P with the weights swapped and no degV (hop 1's table, De W H_e2v^T P, goes
    to xe_out); its output is dX.  dv2e[p = (e, u)] = <X[u], G[e]>, de2v[p = (e, v)] = <P[v], Xe[e]> (incidence_dot),
    Xe the forward's hop-1 table, kept only when e2v needs a gradient.  With heads = H the weights and their gradients are
    [nnz, H] and the products run over each head's own columns.  degE / degV / W get their exact gradients where they require
    one: q[e] = <sum_p v2e[p] X[u], sum_p e2v[p] P[v]> (Plan.hyperedge_dot), dW = q degE, ddegE = q W, and
    ddegV[v] = <dY[v], Z[v]> with Z the same call without degV (Plan.rows_dot); X is then kept as for dv2e.
    bfloat16 node_feat (Options.incidence_bf16 = 'rows'): the same node on the bf16-row kernels.  Y and dX are bfloat16;
    P is rounded to bfloat16 once (_times_degV), Xe and G stay float32, the weight gradients come from the mixed dots
    (bfloat16 X or P against float32 G or Xe) in float32; the scale gradients widen X and P for the float32 kernels."""

    @staticmethod
    def forward(ctx, csrptr_t, indices_t, node_feat, v2e, e2v, degE, degV, W, heads=1):
        N, F = node_feat.shape
        M = csrptr_t.numel() - 1
        plan = cached_plan(N, csrptr_t, indices_t)
        keep_xe = e2v is not None and ctx.needs_input_grad[4]
        Xe = torch.empty((M, F), dtype=torch.float32, device=node_feat.device) if keep_xe else None
        out = plan.aggregate_incidence(csrptr_t, indices_t, node_feat, v2e, e2v, degE, degV, W, xe_out=Xe, heads=heads)
        need_scale = any(t is not None and ctx.needs_input_grad[i] for i, t in ((5, degE), (6, degV), (7, W)))
        keep_x = (v2e is not None and ctx.needs_input_grad[3]) or need_scale
        ctx.save_for_backward(csrptr_t, indices_t, node_feat if keep_x else None, v2e, e2v, degE, degV, W, Xe)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, grad_out):
        csrptr_t, indices_t, X, v2e, e2v, degE, degV, W, Xe = ctx.saved_tensors
        g = grad_out.contiguous()
        N, F = g.shape
        M = csrptr_t.numel() - 1
        plan = cached_plan(N, csrptr_t, indices_t)
        P = g if degV is None else _times_degV(g, degV)
        need_x = ctx.needs_input_grad[2]
        need_v2e = v2e is not None and ctx.needs_input_grad[3]
        need_e2v = e2v is not None and ctx.needs_input_grad[4]
        gx = gv = ge = None
        if need_x or need_v2e:
            G = torch.empty((M, F), dtype=torch.float32, device=g.device) if need_v2e else None
            gx = plan.aggregate_incidence(csrptr_t, indices_t, P, e2v, v2e, degE, None, W, xe_out=G, heads=ctx.heads)
            if need_v2e:
                gv = plan.incidence_dot(csrptr_t, indices_t, X, G, heads=ctx.heads)
        if need_e2v:
            ge = plan.incidence_dot(csrptr_t, indices_t, P, Xe, heads=ctx.heads)
        need_dE, need_dV, need_dW = (t is not None and ctx.needs_input_grad[i] for i, t in ((5, degE), (6, degV), (7, W)))
        gE = gV = gW = None
        if need_dE or need_dW:  # q[e] = <sum_p v2e[p] X[u], sum_p e2v[p] P[v]>: both hyperedge sums in one kernel
            q = plan.hyperedge_dot(csrptr_t, indices_t, X.float(), P.float(), v2e, e2v, heads=ctx.heads)  # float(): bf16 rows widened
            gE, gW = _edge_scale_grads(plan, csrptr_t, q, degE, W, need_dE, need_dW)
        if need_dV:  # <dY[v], Z[v]>, Z the same call without degV
            Z = plan.aggregate_incidence(csrptr_t, indices_t, X.float(), v2e, e2v, degE, None, W, heads=ctx.heads)
            gV = plan.rows_dot(g.float(), Z)
        return None, None, gx if need_x else None, gv, ge, gE, gV, gW, None


def incidence_aggr(csrptr_t, indices_t, node_feat, v2e_weight=None, e2v_weight=None, degE=None, degV=None, W=None,
                   options=None, heads=1):
    """Y[v] = degV[v] * sum_{p=(e,v)} e2v[p] * (degE[e] * W[e] * sum_{p'=(e,u)} v2e[p'] * X[u]): the sum aggregation with a
    weight per (vertex, hyperedge) incidence, e.g. a probabilistic H or hypergraph attention's coefficients
    (include/hg_aggr.h, hg_aggr_incidence_f32).  v2e_weight / e2v_weight: float32 [nnz], aligned with indices_t, or None
    (unit weights); the same tensor twice for a symmetric weighting.  Gradients are exact for node_feat and both weight
    arrays and, where they require one, for degE / degV / W -- the reference has no rule for this operator, so
    Options.backward does not apply.
    Options.variant 'auto' and 'pull' run (both are the pull kernels); 'fused', 'push_atomic', 'push_groups' raise
    ValueError.  float32 only (TypeError for bfloat16) unless Options.incidence_bf16 = 'rows': then node_feat may be bfloat16
    and Y comes back bfloat16 -- Y = round_bf16(the float32 call on node_feat.float()) bit for bit -- with float32 weights,
    scales and weight / scale gradients, and a bfloat16 gradient for node_feat.
    heads = H > 1: one call for H attention heads.  node_feat is [N, H * C] and head h owns columns h C .. (h + 1) C - 1;
    the weights are [nnz, H] (nnz * H elements, head fastest) and column h weighs head h's columns; their gradients come
    back [nnz, H].  F % H != 0 raises ValueError.  heads = 1 is the call above, unchanged."""
    opt = _opt(options)
    if heads == 1:
        v2e, e2v = (_flat(t) if isinstance(t, torch.Tensor) else t for t in (v2e_weight, e2v_weight))
    else:
        _heads(heads)
        v2e, e2v = (_per_head(t, heads) if isinstance(t, torch.Tensor) else t for t in (v2e_weight, e2v_weight))
    _incidence_args(csrptr_t, indices_t, node_feat, v2e, e2v, opt, heads)
    degE, degV, W = _flat(degE), _flat(degV), _flat(W)
    if not (torch.is_grad_enabled() and _any_requires_grad(node_feat, v2e, e2v, degE, degV, W)):
        plan = cached_plan(node_feat.shape[0], csrptr_t, indices_t)
        return plan.aggregate_incidence(csrptr_t, indices_t, node_feat, v2e, e2v, degE, degV, W, heads=heads)
    return _IncidenceAggr.apply(csrptr_t, indices_t, node_feat, v2e, e2v, degE, degV, W, heads)


def HGNNAggrIncidence(hyperg, in_feat, v2e_weight, e2v_weight, degE, degV, Wdiag, options=None, heads=1):
    """HGNNAggr with a weight per incidence (incidence_aggr) on a HyperGraph's H_T tensors."""
    return incidence_aggr(hyperg.H_T_csrptr, hyperg.H_T_colind, in_feat, v2e_weight, e2v_weight, degE, degV, Wdiag,
                          options=options, heads=heads)


# ---- hypergraph attention coefficients (include/hg_aggr.h, hg_incidence_attention_f32) --------------------------------

_GROUPS = ("hyperedge", "vertex")


def _segment_args(what, csrptr_t, indices_t, floats, lengths, group, opt, heads=1, rng_state=None):
    """Argument checks of incidence_softmax / incidence_sum in _incidence_args' order: every refusal is decided before a
    device is touched.  floats: (name, tensor or None) pairs; lengths: the element count each must have.  rng_state: the
    dropout's state where one was passed: its dtype with the dtypes, its length with the lengths, its device last."""
    if opt is not None and opt.variant not in ("auto", "pull"):
        raise ValueError("%s runs the atomic-free segment kernels: variant must be 'auto' or 'pull', got %r"
                         % (what, opt.variant))
    _heads(heads)
    if group not in _GROUPS:
        raise ValueError("group / side must be 'hyperedge' or 'vertex', got %r" % (group,))
    for name, t in floats:
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32):
            raise TypeError("%s must be a float32 tensor (%s has no bfloat16 form), got %s"
                            % (name, what, getattr(t, "dtype", type(t))))
    if rng_state is not None:
        _rng_state_dtype(rng_state)
    if not isinstance(csrptr_t, torch.Tensor) or not isinstance(indices_t, torch.Tensor):
        raise TypeError("csrptr_t and indices_t must be int32 tensors")
    for (name, t), n in zip(floats, lengths):
        if t is not None and t.numel() != n:
            raise ValueError("%s must have %d elements, got %d" % (name, n, t.numel()))
    if rng_state is not None:
        _rng_state_length(rng_state)
    _check_index(csrptr_t, "csrptr_t")
    _check_index(indices_t, "indices_t")
    for name, t in floats:
        if t is not None:
            _check_feat(t, name, device=csrptr_t.device)
    if rng_state is not None:
        _rng_state_device(rng_state, csrptr_t.device)


class _IncidenceSoftmax(torch.autograd.Function):
    """alpha = softmax over each group of leaky_relu((sv[u] + se[e]) + t[p]) and its exact gradients: the backward kernel's
    ds = alpha (dalpha - sum_g alpha dalpha) leaky' is the gradient of t, dsv / dse are its sums over each vertex's /
    hyperedge's incidences.  sv, se and t (the logit per incidence) may each be None.  p_drop > 0: dropout on alpha fused
    into both kernels -- returns keep ? alpha / (1 - p) : 0, saves the undropped alpha and the two words of rng_state, from
    which the backward regenerates the mask: the plain backward on dalpha = keep ? dout / (1 - p) : 0."""

    @staticmethod
    def forward(ctx, csrptr_t, indices_t, sv, se, t, N, group, slope, heads, p_drop, rng_state):
        plan = cached_plan(N, csrptr_t, indices_t)
        if p_drop > 0.0:
            alpha, out = plan.incidence_attention_dropout(csrptr_t, indices_t, sv, se, group, slope, p_drop, rng_state,
                                                          heads=heads, entry=t)
        else:
            alpha = out = plan.incidence_attention(csrptr_t, indices_t, sv, se, group, slope, heads=heads, entry=t)
        ctx.save_for_backward(csrptr_t, indices_t, sv, se, t, alpha, rng_state)
        ctx.plan, ctx.group, ctx.slope, ctx.heads, ctx.p_drop = plan, group, slope, heads, p_drop  # the backward runs on this plan
        return out

    @staticmethod
    def backward(ctx, dout):
        csrptr_t, indices_t, sv, se, t, alpha, rng_state = ctx.saved_tensors
        plan = ctx.plan
        need_sv = sv is not None and ctx.needs_input_grad[2]
        need_se = se is not None and ctx.needs_input_grad[3]
        if ctx.p_drop > 0.0:
            ds, dsv, dse = plan.incidence_attention_dropout_backward(
                csrptr_t, indices_t, alpha, dout.contiguous(), sv, se, ctx.group, ctx.slope, ctx.p_drop, rng_state,
                need_sv=need_sv, need_se=need_se, heads=ctx.heads, entry=t)
        else:
            ds, dsv, dse = plan.incidence_attention_backward(csrptr_t, indices_t, alpha, dout.contiguous(), sv, se, ctx.group,
                                                             ctx.slope, need_sv=need_sv, need_se=need_se, heads=ctx.heads,
                                                             entry=t)
        dt = ds.view_as(t) if ctx.needs_input_grad[4] else None  # never set for t = None
        return None, None, dsv, dse, dt, None, None, None, None, None, None


def _dropout_p(dropout):
    """The `dropout` keyword as a float in [0, 1): ValueError otherwise, before any tensor is looked at."""
    if isinstance(dropout, bool) or not isinstance(dropout, numbers.Real) or not 0.0 <= float(dropout) < 1.0:
        raise ValueError("dropout must be a real number in [0, 1), got %r (1.0 is refused: the scale 1 / (1 - dropout) "
                         "of the kept coefficients would be infinite)" % (dropout,))
    return float(dropout)


def incidence_softmax(csrptr_t, indices_t, node_score=None, edge_score=None, group="hyperedge", negative_slope=0.2,
                      options=None, num_nodes=None, heads=1, dropout=0.0, training=True, rng_state=None,
                      return_rng_state=False, incidence_score=None):
    """Hypergraph attention's coefficients, alpha [nnz] aligned with indices_t: for every incidence p = (e, u)
    alpha[p] = softmax over p's group of leaky_relu(node_score[u] + edge_score[e], negative_slope); the group is p's
    hyperedge (group='hyperedge': the coefficients of a hyperedge's members sum to 1) or p's vertex (group='vertex').
    node_score [N] / edge_score [M]: float32, either may be None (0).  The result is what incidence_aggr takes as
    v2e_weight / e2v_weight.  Gradients are exact for both score vectors.  num_nodes: N; required when node_score is
    None, otherwise optional (node_score's length is taken as N; given, node_score must have that length).  Options.variant 'auto' and 'pull' run; the others raise ValueError.  float32 only (TypeError for bfloat16).
    heads = H > 1: a softmax per head in one call.  node_score holds N * H and edge_score M * H elements ([N, H] / [M, H],
    head fastest), alpha comes back [nnz, H]; N is taken as node_score's element count / H.  heads = 1 is the call above,
    unchanged.
    dropout = p in (0, 1) with training=True: the coefficients after dropout, keep ? alpha / (1 - p) : 0, from the same
    launch (hg_incidence_attention_dropout_heads_f32) -- no stored mask, no further pass; the gradients stay exact, the
    backward regenerates the mask.  rng_state: int64 [2] on the scores' device, the {key, sid} of the Philox mask (keep
    depends on it, the position in indices_t and the head alone); None draws one with torch.randint on that device: it
    follows torch.manual_seed, costs no host synchronisation and, captured into a graph, gives every replay a new mask.
    return_rng_state=True returns (coefficients, the state used -- None where no dropout ran).  dropout = 0.0 or
    training=False is the call above: the same code path, the same bits, torch's generator untouched.
    incidence_score: float32, nnz * heads elements ([nnz] / [nnz, H], aligned with indices_t, head fastest): a logit per
    (vertex, hyperedge) pair, added to the score -- leaky_relu((node_score[u] + edge_score[e]) + incidence_score[p]) -- for
    the scores that do not split into a vertex and a hyperedge term: scaled dot products (incidence_dot), GATv2, anything
    that depends on the pair (hg_incidence_attention_entry_heads_f32).  node_score and edge_score may then both be None
    (num_nodes is required, as whenever node_score is None).  Gradients are exact for all three; the gradient of
    incidence_score is the backward kernel's own output, no further pass.  It works with heads, both groups and dropout.
    None is the call above: the same code path, the same bits."""
    opt = _opt(options)
    p_drop = _dropout_p(dropout)
    if heads == 1:
        sv, se, t = (_flat(x) if isinstance(x, torch.Tensor) else x for x in (node_score, edge_score, incidence_score))
    else:
        _heads(heads)
        sv, se, t = (_per_head(x, heads) if isinstance(x, torch.Tensor) else x
                     for x in (node_score, edge_score, incidence_score))
    if sv is None and num_nodes is None:
        raise ValueError("incidence_softmax needs node_score or num_nodes (the number of vertices)")
    N = int(num_nodes) if num_nodes is not None else sv.numel() // heads
    M = csrptr_t.numel() - 1 if isinstance(csrptr_t, torch.Tensor) else 0
    if p_drop == 0.0 or not training:  # no dropout: the state is neither looked at nor drawn nor returned
        p_drop, rng_state = 0.0, None
    floats, lengths = (("node_score", sv), ("edge_score", se)), (N * heads, M * heads)
    if t is not None:
        nnz = indices_t.numel() if isinstance(indices_t, torch.Tensor) else 0
        floats, lengths = floats + (("incidence_score", t),), lengths + (nnz * heads,)
    _segment_args("incidence_softmax", csrptr_t, indices_t, floats, lengths, group, opt, heads, rng_state)
    slope = float(negative_slope)
    if p_drop > 0.0 and rng_state is None:  # on the device: no synchronisation, and a captured draw is drawn again by every replay
        info = torch.iinfo(torch.int64)  # randint's upper end is exclusive: every int64 but 2^63 - 1, which a key can spare
        rng_state = torch.randint(info.min, info.max, (2,), dtype=torch.int64, device=csrptr_t.device)
    if torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (sv, se, t)):
        out = _IncidenceSoftmax.apply(csrptr_t, indices_t, sv, se, t, N, group, slope, heads, p_drop, rng_state)
    elif p_drop > 0.0:  # nothing to differentiate: the operator itself, without the autograd node
        out = cached_plan(N, csrptr_t, indices_t).incidence_attention_dropout(csrptr_t, indices_t, sv, se, group, slope, p_drop,
                                                                             rng_state, heads=heads, entry=t)[1]
    else:
        out = cached_plan(N, csrptr_t, indices_t).incidence_attention(csrptr_t, indices_t, sv, se, group, slope, heads=heads,
                                                                     entry=t)
    return (out, rng_state) if return_rng_state else out


# ---- fused attention aggregation (include/hg_aggr.h, hg_aggr_incidence_attention_heads_f32) -------------------------------

class _IncidenceAttentionAggr(torch.autograd.Function):
    """incidence_aggr(X, alpha, alpha) on alpha = incidence_softmax(sv, se) as one node that never holds alpha between
    forward and backward.  The forward keeps X, the scores, the two statistics per segment and head and the scales; the
    backward forms alpha from the same scores with the softmax kernel (the bits the gather used), runs _IncidenceAggr's
    formulas with v2e = e2v = alpha -- hop 1's table Xe is gathered again for de2v -- and hands dalpha = dv2e + de2v to
    the softmax's backward.  Exact gradients for X, both scores and, where they require one, degE / degV / W."""

    @staticmethod
    def forward(ctx, csrptr_t, indices_t, node_feat, sv, se, degE, degV, W, group, slope, heads):
        plan = cached_plan(node_feat.shape[0], csrptr_t, indices_t)
        seg_max, seg_inv = plan.incidence_attention_stats(csrptr_t, indices_t, sv, se, group, slope, heads=heads)
        out = plan.aggregate_incidence_attention(csrptr_t, indices_t, node_feat, sv, se, group, slope, seg_max, seg_inv,
                                                 degE, degV, W, heads=heads)
        need_score = any(t is not None and ctx.needs_input_grad[i] for i, t in ((3, sv), (4, se)))
        need_scale = any(t is not None and ctx.needs_input_grad[i] for i, t in ((5, degE), (6, degV), (7, W)))
        ctx.save_for_backward(csrptr_t, indices_t, node_feat if need_score or need_scale else None, sv, se, seg_max, seg_inv,
                              degE, degV, W)
        ctx.group, ctx.slope, ctx.heads = group, slope, heads
        return out

    @staticmethod
    def backward(ctx, grad_out):
        csrptr_t, indices_t, X, sv, se, seg_max, seg_inv, degE, degV, W = ctx.saved_tensors
        g = grad_out.contiguous()
        N, F = g.shape
        M = csrptr_t.numel() - 1
        heads = ctx.heads
        plan = cached_plan(N, csrptr_t, indices_t)
        P = g if degV is None else g * degV.reshape(-1, 1)
        need_x = ctx.needs_input_grad[2]
        need_sv = sv is not None and ctx.needs_input_grad[3]
        need_se = se is not None and ctx.needs_input_grad[4]
        need_dE, need_dV, need_dW = (t is not None and ctx.needs_input_grad[i] for i, t in ((5, degE), (6, degV), (7, W)))
        need_score = need_sv or need_se
        gx = dsv = dse = gE = gV = gW = None
        if not (need_score or need_dE or need_dV or need_dW):  # dX alone: the adjoint is the fused call itself
            gx = plan.aggregate_incidence_attention(csrptr_t, indices_t, P, sv, se, ctx.group, ctx.slope, seg_max, seg_inv,
                                                    degE, None, W, heads=heads)
            return None, None, gx if need_x else None, None, None, None, None, None, None, None, None
        alpha = plan.incidence_attention(csrptr_t, indices_t, sv, se, ctx.group, ctx.slope, heads=heads)
        if need_x or need_score:
            G = torch.empty((M, F), dtype=torch.float32, device=g.device) if need_score else None
            gx = plan.aggregate_incidence(csrptr_t, indices_t, P, alpha, alpha, degE, None, W, xe_out=G, heads=heads)
        if need_score:
            dalpha = plan.incidence_dot(csrptr_t, indices_t, X, G, heads=heads)
            Xe = plan.gather_rows_incidence(0, csrptr_t, indices_t, X, alpha, degE, W, heads=heads)
            dalpha += plan.incidence_dot(csrptr_t, indices_t, P, Xe, heads=heads)  # dv2e + de2v, as autograd would add them
            del G, Xe
            _, dsv, dse = plan.incidence_attention_backward(csrptr_t, indices_t, alpha, dalpha, sv, se, ctx.group, ctx.slope,
                                                            need_sv=need_sv, need_se=need_se, heads=heads)
        if need_dE or need_dW:
            q = plan.hyperedge_dot(csrptr_t, indices_t, X, P, alpha, alpha, heads=heads)
            gE, gW = _edge_scale_grads(plan, csrptr_t, q, degE, W, need_dE, need_dW)
        if need_dV:
            Z = plan.aggregate_incidence(csrptr_t, indices_t, X, alpha, alpha, degE, None, W, heads=heads)
            gV = plan.rows_dot(g, Z)
        return None, None, gx if need_x else None, dsv, dse, gE, gV, gW, None, None, None


def incidence_attention_aggr(csrptr_t, indices_t, node_feat, node_score, edge_score, group="hyperedge", negative_slope=0.2,
                             degE=None, degV=None, W=None, heads=1, num_nodes=None, options=None):
    """Hypergraph attention's aggregation in one call: what
        alpha = incidence_softmax(csrptr_t, indices_t, node_score, edge_score, group=group, negative_slope=negative_slope,
                                  heads=heads, num_nodes=N)
        Y = incidence_aggr(csrptr_t, indices_t, node_feat, alpha, alpha, degE, degV, W, heads=heads)
    returns, bit for bit, without alpha [nnz, heads] ever existing: a segment kernel writes the softmax's maximum and
    reciprocal sum per group and head (two [M, heads] or [N, heads] arrays), and each lane of the two row gathers forms its
    coefficient from the two scores and those two numbers as it gathers the row (hg_aggr_incidence_attention_heads_f32).
    The plan's incidence permutation is not used.  node_score [N] / [N, heads], edge_score [M] / [M, heads]: float32,
    either may be None (0).  Gradients are exact for node_feat, both scores and, where they require one, degE / degV / W;
    nothing of nnz * heads elements is kept from forward to backward (the backward forms alpha again, and frees it).
    num_nodes: optional, must equal node_feat's row count.  Options.variant 'auto' and 'pull' run; the others raise
    ValueError.  float32 only (TypeError for bfloat16).  Not covered, use the two calls above: attention dropout, a logit
    per incidence (incidence_score is itself an [nnz, heads] array), bfloat16."""
    opt = _opt(options)
    if opt.variant not in ("auto", "pull"):
        raise ValueError("incidence_attention_aggr runs the pull kernels: variant must be 'auto' or 'pull', got %r"
                         % opt.variant)
    _heads(heads)
    if group not in _GROUPS:
        raise ValueError("group / side must be 'hyperedge' or 'vertex', got %r" % (group,))
    if heads == 1:
        sv, se = (_flat(x) if isinstance(x, torch.Tensor) else x for x in (node_score, edge_score))
    else:
        sv, se = (_per_head(x, heads) if isinstance(x, torch.Tensor) else x for x in (node_score, edge_score))
    floats = (("node_feat", node_feat), ("node_score", sv), ("edge_score", se))
    for name, t in floats:
        if (t is not None or name == "node_feat") and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32):
            raise TypeError("%s must be a float32 tensor (incidence_attention_aggr has no bfloat16 form), got %s"
                            % (name, getattr(t, "dtype", type(t))))
    if node_feat.dim() != 2:
        raise ValueError("node_feat must be [N, F]")
    N, F = node_feat.shape
    if F % heads:
        raise ValueError("node_feat's width %d is no multiple of heads = %d" % (F, heads))
    if num_nodes is not None and int(num_nodes) != N:
        raise ValueError("num_nodes = %d, but node_feat has %d rows" % (int(num_nodes), N))
    if not isinstance(csrptr_t, torch.Tensor) or not isinstance(indices_t, torch.Tensor):
        raise TypeError("csrptr_t and indices_t must be int32 tensors")
    M = csrptr_t.numel() - 1
    for (name, t), n in zip(floats[1:], (N * heads, M * heads)):
        if t is not None and t.numel() != n:
            raise ValueError("%s must have %d elements, got %d" % (name, n, t.numel()))
    _check_index(csrptr_t, "csrptr_t")
    _check_index(indices_t, "indices_t")
    _check_feat(node_feat, "node_feat")
    for name, t in floats[1:]:
        if t is not None:
            _check_feat(t, name, device=node_feat.device)
    degE, degV, W = _flat(degE), _flat(degV), _flat(W)
    slope = float(negative_slope)
    if not (torch.is_grad_enabled() and _any_requires_grad(node_feat, sv, se, degE, degV, W)):
        plan = cached_plan(N, csrptr_t, indices_t)
        return plan.aggregate_incidence_attention(csrptr_t, indices_t, node_feat, sv, se, group, slope, None, None,
                                                  degE, degV, W, heads=heads)
    return _IncidenceAttentionAggr.apply(csrptr_t, indices_t, node_feat, sv, se, degE, degV, W, group, slope, heads)


# ---- one weighted hop and the dot product per incidence (hg_gather_rows_incidence_heads_f32, hg_incidence_dot_heads_f32) ----

_HOPS = ("hyperedge", "vertex")


def _scaled(g, scale_a, scale_b):
    for sc in (scale_a, scale_b):
        if sc is not None:
            g = g * sc.reshape(-1, 1)  # a bfloat16 g is promoted: the scaled gradient stays float32 for the mixed hop and dot
    return g.contiguous()


def _hop(plan, csrptr_t, indices_t, to, src, w, scale_a, scale_b, heads, dtype=None):
    """One hop on the plan: the weighted panels kernel of incidence_aggr's hop, or without weights the library's
    unweighted row gather (Plan.gather_rows, hg_gather_rows_f32).  dtype: the result's (default: src's); bfloat16 rows on
    either side take the panels kernel's bf16-row instances, weighted or not (hg_gather_rows_incidence_heads_bf16)."""
    dtype = src.dtype if dtype is None else dtype
    if w is None and src.dtype == dtype == torch.float32:
        return plan.gather_rows(_HOPS.index(to), csrptr_t, indices_t, src, scale_a, scale_b)
    out = None
    if dtype != src.dtype:
        out = torch.empty((plan.M if to == "hyperedge" else plan.N, src.shape[1]), dtype=dtype, device=src.device)
    return plan.gather_rows_incidence(to, csrptr_t, indices_t, src, w, scale_a, scale_b, heads=heads, out=out)


class _IncidenceGather(torch.autograd.Function):
    """dst = scale . (H_w^T src) (to 'hyperedge') or scale . (H_w src) (to 'vertex') and its exact gradients: with
    gs = grad * scale, d src is the opposite hop of gs with the same weights and d weight[p = (e, u)] the product of the
    vertex row and the hyperedge row of (src, gs) over each head's columns (incidence_dot).  The scales get none."""

    @staticmethod
    def forward(ctx, csrptr_t, indices_t, src, w, scale_a, scale_b, N, to, heads):
        plan = cached_plan(N, csrptr_t, indices_t)
        keep_src = w is not None and ctx.needs_input_grad[3]
        ctx.save_for_backward(csrptr_t, indices_t, src if keep_src else None, w, scale_a, scale_b)
        ctx.N, ctx.to, ctx.heads, ctx.dtype = N, to, heads, src.dtype
        return _hop(plan, csrptr_t, indices_t, to, src, w, scale_a, scale_b, heads)

    @staticmethod
    def backward(ctx, grad):
        csrptr_t, indices_t, src, w, scale_a, scale_b = ctx.saved_tensors
        plan = cached_plan(ctx.N, csrptr_t, indices_t)
        gs = _scaled(grad, scale_a, scale_b)
        back = _HOPS[1 - _HOPS.index(ctx.to)]
        gsrc = gw = None
        if ctx.needs_input_grad[2]:
            gsrc = _hop(plan, csrptr_t, indices_t, back, gs, w, None, None, ctx.heads, ctx.dtype)
        if w is not None and ctx.needs_input_grad[3]:
            A, B = (src, gs) if ctx.to == "hyperedge" else (gs, src)  # A: the vertex rows, B: the hyperedge rows
            gw = plan.incidence_dot(csrptr_t, indices_t, A, B, heads=ctx.heads).view_as(w)
        return None, None, gsrc, gw, None, None, None, None, None


class _IncidenceReduce(torch.autograd.Function):
    """dst = scale . (max or min over each row's entries of src) with the winner's position recorded, and its exact
    gradient: dsrc is the select-gather of gs = grad * scale over the opposite hop (Plan.gather_rows_select), so the whole
    gradient goes to the winner, the smallest position among ties.  The node keeps arg and the scales, no source rows."""

    @staticmethod
    def forward(ctx, csrptr_t, indices_t, src, scale_a, scale_b, N, to, op):
        plan = cached_plan(N, csrptr_t, indices_t)
        dst, arg = plan.gather_rows_reduce(to, csrptr_t, indices_t, src, op, scale_a, scale_b)
        ctx.save_for_backward(csrptr_t, indices_t, arg, scale_a, scale_b)
        ctx.N, ctx.to = N, to
        ctx.mark_non_differentiable(arg)
        return dst, arg

    @staticmethod
    def backward(ctx, grad, _grad_arg):
        csrptr_t, indices_t, arg, scale_a, scale_b = ctx.saved_tensors
        plan = cached_plan(ctx.N, csrptr_t, indices_t)
        gsrc = None
        if ctx.needs_input_grad[2]:
            gsrc = plan.gather_rows_select(ctx.to, csrptr_t, indices_t, _scaled(grad, scale_a, scale_b), arg)
        return None, None, gsrc, None, None, None, None, None


_REDUCES = ("sum", "mean", "max", "min")


def incidence_gather(csrptr_t, indices_t, src, weight=None, to="hyperedge", scale_a=None, scale_b=None, heads=1,
                     options=None, num_nodes=None, reduce="sum", return_index=False):
    """One weighted hop of the incidence path as an operator of its own.  to='hyperedge': src is [N, F] and
    dst[e] = ((sum_{p=(e,u)} weight[p] * src[u]) * scale_a[e]) * scale_b[e], [M, F] -- hyperedge embeddings, e.g. the member
    mean with scale_a = 1 / |e|; to='vertex': src is [M, F] and dst[v] = ((sum_{p=(e,v)} weight[p] * src[e]) * scale_a[v]) *
    scale_b[v], [N, F].  weight: float32 [nnz] aligned with indices_t ([nnz, H] with heads = H, column h weighing head h's
    columns h F/H .. (h + 1) F/H - 1), or None (unit weights); the scales hold one factor per row of dst, or None.
    With weights it runs incidence_aggr's kernels for that hop (hg_gather_rows_incidence_heads_f32): hop 'hyperedge' into
    hop 'vertex' gives incidence_aggr's result bit for bit; without, the unweighted row gather (hg_gather_rows_f32).
    Differentiable in src and weight; the scales get no gradient here.  Options.variant 'auto' and 'pull' run;
    the others raise ValueError.  float32 only (TypeError for bfloat16) unless Options.incidence_bf16 = 'rows': a bfloat16 src
    gives a bfloat16 dst = round_bf16(the float32 call on src.float()), weighted or not, and gets a bfloat16 gradient; weight,
    scales and the weight's gradient stay float32.  num_nodes: N for to='vertex', where src does not
    tell it; without it N is the length of a given scale, else the largest member id + 1, read back from the device.
    reduce: 'sum' is the call above on its code path.  'mean' runs the same kernels with 1 / (row length) in the first scale
    slot and the caller's scale_a in the second, dst = (sum * (1 / len)) * scale_a; a scale_b raises ValueError; an empty row
    gives 0.  'max' / 'min' take the greatest / smallest entry of every row and column instead of the sum, scaled the same way
    (Plan.gather_rows_reduce): weight must be None and heads 1 (ValueError), float32 only (TypeError for bfloat16 whatever
    Options.incidence_bf16 says); the winner is chosen under > (<), the smallest position in indices_t among ties, an empty
    row gives +0.0 whatever its scale, and NaN inputs are unspecified.  The gradient goes to the winner alone -- not torch's
    amax rule, which shares it among ties -- through a select-gather without atomics.  return_index=True (max / min only)
    returns (dst, arg), arg int32 [rows, F] the winner's position in indices_t (-1: empty row), not differentiable."""
    opt = _opt(options)
    if opt.variant not in ("auto", "pull"):
        raise ValueError("incidence_gather runs the pull kernels: variant must be 'auto' or 'pull', got %r" % opt.variant)
    _heads(heads)
    if to not in _HOPS:
        raise ValueError("to must be 'hyperedge' or 'vertex', got %r" % (to,))
    if reduce not in _REDUCES:
        raise ValueError("reduce must be one of %s, got %r" % (", ".join(repr(r) for r in _REDUCES), reduce))
    if reduce in ("max", "min"):
        if weight is not None:
            raise ValueError("reduce=%r takes no weight (a comparison has no weighted form here)" % reduce)
        if heads != 1:
            raise ValueError("reduce=%r takes heads = 1" % reduce)
        if isinstance(src, torch.Tensor) and src.dtype == torch.bfloat16:
            raise TypeError("src must be a float32 tensor (reduce=%r has no bfloat16 form), got %s" % (reduce, src.dtype))
    elif return_index:
        raise ValueError("return_index needs reduce='max' or 'min', got %r" % reduce)
    if reduce == "mean" and scale_b is not None:
        raise ValueError("reduce='mean' keeps 1 / (row length) in the first scale slot and scale_a in the second: "
                         "scale_b must be None")
    w = weight
    if isinstance(w, torch.Tensor):
        w = _flat(w) if heads == 1 else _per_head(w, heads)
    scale_a, scale_b = _flat(scale_a), _flat(scale_b)
    for name, t in (("src", src), ("weight", w), ("scale_a", scale_a), ("scale_b", scale_b)):
        if (t is not None or name == "src") and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32) \
                and not (name == "src" and _rows_dtype_ok(t, opt)):
            raise TypeError("%s must be a float32 tensor (incidence_gather has no bfloat16 form), got %s"
                            % (name, getattr(t, "dtype", type(t))))
    if src.dim() != 2:
        raise ValueError("src must be [rows, F]")
    if src.shape[1] % heads:
        raise ValueError("src's width %d is no multiple of heads = %d" % (src.shape[1], heads))
    if not isinstance(csrptr_t, torch.Tensor) or not isinstance(indices_t, torch.Tensor):
        raise TypeError("csrptr_t and indices_t must be int32 tensors")
    nnz, M = indices_t.numel(), csrptr_t.numel() - 1
    if w is not None and w.numel() != nnz * heads:
        raise ValueError("weight must have one weight per incidence%s (%d elements), got %d"
                         % (" and head" if heads > 1 else "", nnz * heads, w.numel()))
    if to == "hyperedge":
        N = src.shape[0]
        if num_nodes is not None and int(num_nodes) != N:
            raise ValueError("src has %d rows, num_nodes is %d" % (N, int(num_nodes)))
    elif src.shape[0] != M:
        raise ValueError("src has %d rows, the hypergraph has %d hyperedges" % (src.shape[0], M))
    else:
        N = int(num_nodes) if num_nodes is not None else next((t.numel() for t in (scale_a, scale_b) if t is not None), None)
    for name, t in (("scale_a", scale_a), ("scale_b", scale_b)):
        if t is not None and t.numel() != (M if to == "hyperedge" else N):
            raise ValueError("%s must have one factor per row of the result (%d), got %d"
                             % (name, M if to == "hyperedge" else N, t.numel()))
    _check_index(csrptr_t, "csrptr_t")
    _check_index(indices_t, "indices_t")
    _check_feat(src, "src", bf16_ok=opt.incidence_bf16 == "rows")
    for name, t in (("weight", w), ("scale_a", scale_a), ("scale_b", scale_b)):
        if t is not None:
            _check_feat(t, name, device=src.device)
    if N is None:
        N = int(indices_t.max()) + 1 if nnz else 0
    if reduce in ("max", "min"):
        if torch.is_grad_enabled() and src.requires_grad:
            dst, arg = _IncidenceReduce.apply(csrptr_t, indices_t, src, scale_a, scale_b, N, to, reduce)
        else:
            dst, arg = cached_plan(N, csrptr_t, indices_t).gather_rows_reduce(to, csrptr_t, indices_t, src, reduce,
                                                                              scale_a, scale_b)
        return (dst, arg) if return_index else dst
    if reduce == "mean":
        scale_a, scale_b = cached_plan(N, csrptr_t, indices_t).row_recip(to, csrptr_t), scale_a
    if not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (src, w))):
        return _hop(cached_plan(N, csrptr_t, indices_t), csrptr_t, indices_t, to, src, w, scale_a, scale_b, heads)
    return _IncidenceGather.apply(csrptr_t, indices_t, src, w, scale_a, scale_b, N, to, heads)


def reduce_aggr(csrptr_t, indices_t, X, first="sum", second="sum", degE=None, degV=None, W=None, num_nodes=None,
                options=None):
    """The two hops with a reduction each, composed of incidence_gather calls: first ('sum', 'mean', 'max', 'min') takes the
    members of every hyperedge, Xe[e] = ((first_{u in e} X[u]) * degE[e]) * W[e]; second takes the hyperedges of every vertex,
    Y[v] = (second_{e contains v} Xe[e]) * degV[v].  first='mean' scales the sum by the single factor degE * W / |e| as
    hgnnaggr_mean forms it (non-finite values, which only an empty hyperedge has, set to 0); second='mean' divides by the
    vertex's number of incidences before degV.  UniSAGE's mean / max aggregators in either hop are such calls.  float32;
    differentiable in X (max / min: the gradient goes to the winner alone); degE / degV / W get no gradient here."""
    for name, r in (("first", first), ("second", second)):
        if r not in _REDUCES:
            raise ValueError("%s must be one of %s, got %r" % (name, ", ".join(repr(x) for x in _REDUCES), r))
    if not isinstance(X, torch.Tensor) or X.dtype != torch.float32:
        raise TypeError("X must be a float32 tensor (reduce_aggr has no bfloat16 form), got %s" % (getattr(X, "dtype", type(X)),))
    if X.dim() != 2:
        raise ValueError("X must be [N, F]")
    N = X.shape[0]
    if num_nodes is not None and int(num_nodes) != N:
        raise ValueError("X has %d rows, num_nodes is %d" % (N, int(num_nodes)))
    if first == "mean":
        _check_index(csrptr_t, "csrptr_t")
        num = None  # degE * W / |e|, in _MeanF1's order of operations
        for sc in (degE, W):
            if sc is not None:
                num = _flat(sc) if num is None else num * _flat(sc)
        s = (1.0 if num is None else num) / _edge_sizes(csrptr_t)
        s = torch.where(torch.isfinite(s), s, torch.zeros_like(s))
        Xe = incidence_gather(csrptr_t, indices_t, X, to="hyperedge", scale_a=s, options=options)
    else:
        Xe = incidence_gather(csrptr_t, indices_t, X, to="hyperedge", scale_a=degE, scale_b=W, options=options, reduce=first)
    return incidence_gather(csrptr_t, indices_t, Xe, to="vertex", scale_a=degV, options=options, num_nodes=N, reduce=second)


class _IncidenceDot(torch.autograd.Function):
    """out[p, h] = <A[u, head h], B[e, head h]> and its gradients, one weighted hop each: dA = the hop to the vertices of B
    weighted by the incoming gradient, dB = the hop to the hyperedges of A."""

    @staticmethod
    def forward(ctx, csrptr_t, indices_t, A, B, heads):
        plan = cached_plan(A.shape[0], csrptr_t, indices_t)
        ctx.save_for_backward(csrptr_t, indices_t, A if ctx.needs_input_grad[3] else None, B if ctx.needs_input_grad[2] else None)
        ctx.N, ctx.heads, ctx.dtypes = A.shape[0], heads, (A.dtype, B.dtype)
        return plan.incidence_dot(csrptr_t, indices_t, A, B, heads=heads)

    @staticmethod
    def backward(ctx, grad):
        csrptr_t, indices_t, A, B = ctx.saved_tensors
        plan = cached_plan(ctx.N, csrptr_t, indices_t)
        g = grad.contiguous()
        dA = dB = None
        if ctx.needs_input_grad[2]:  # each gradient in its operand's dtype: the mixed forms of the hop where A and B differ
            dA = _hop(plan, csrptr_t, indices_t, "vertex", B, g, None, None, ctx.heads, ctx.dtypes[0])
        if ctx.needs_input_grad[3]:
            dB = _hop(plan, csrptr_t, indices_t, "hyperedge", A, g, None, None, ctx.heads, ctx.dtypes[1])
        return None, None, dA, dB, None


def incidence_dot(csrptr_t, indices_t, A, B, heads=1, options=None):
    """The dot-product logit of every incidence p = (e, u): out[p] = <A[u], B[e]> for A [N, F] (a row per vertex) and B [M, F]
    (a row per hyperedge), [nnz] aligned with indices_t (hg_incidence_dot_f32).  heads = H > 1: A and B are [*, H * C],
    out[p, h] is the product over head h's columns and comes back [nnz, H].  Scaled by C ** -0.5 it is what
    incidence_softmax takes as incidence_score.  Differentiable in A and B: with g the incoming gradient,
    dA = incidence_gather(B, g, to='vertex') and dB = incidence_gather(A, g, to='hyperedge').  float32 only, unless
    Options.incidence_bf16 = 'rows': A and B may each be bfloat16; out stays float32 -- the float32 call on A.float(),
    B.float() bit for bit -- and each gradient comes back in its operand's dtype."""
    opt = _opt(options)
    _heads(heads)
    for name, t in (("A", A), ("B", B)):
        if not _rows_dtype_ok(t, opt):
            raise TypeError("%s must be a float32 tensor (incidence_dot has no bfloat16 form), got %s"
                            % (name, getattr(t, "dtype", type(t))))
    if not isinstance(csrptr_t, torch.Tensor) or not isinstance(indices_t, torch.Tensor):
        raise TypeError("csrptr_t and indices_t must be int32 tensors")
    M = csrptr_t.numel() - 1
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[1] or B.shape[0] != M:
        raise ValueError("A must be [N, F] and B [M = %d, F] of one width, got %s and %s" % (M, tuple(A.shape), tuple(B.shape)))
    if A.shape[1] % heads:
        raise ValueError("the width %d is no multiple of heads = %d" % (A.shape[1], heads))
    _check_index(csrptr_t, "csrptr_t")
    _check_index(indices_t, "indices_t")
    _check_feat(A, "A", bf16_ok=opt.incidence_bf16 == "rows")
    _check_feat(B, "B", device=A.device, bf16_ok=opt.incidence_bf16 == "rows")
    if not (torch.is_grad_enabled() and (A.requires_grad or B.requires_grad)):
        return cached_plan(A.shape[0], csrptr_t, indices_t).incidence_dot(csrptr_t, indices_t, A, B, heads=heads)
    return _IncidenceDot.apply(csrptr_t, indices_t, A, B, heads)


class _IncidenceSum(torch.autograd.Function):
    """out[g] = sum of val over group g; the backward is the gather dout[group(p)] on the plan's cached segment ids."""

    @staticmethod
    def forward(ctx, csrptr_t, indices_t, val, N, side, heads=1):
        plan = cached_plan(N, csrptr_t, indices_t)
        ctx.save_for_backward(csrptr_t, indices_t)
        ctx.N, ctx.side = N, side
        return plan.incidence_sum(csrptr_t, indices_t, val, side, heads=heads)

    @staticmethod
    def backward(ctx, dout):  # heads: dout [groups, H] -> [nnz, H], the same row gather
        csrptr_t, indices_t = ctx.saved_tensors
        plan = cached_plan(ctx.N, csrptr_t, indices_t)
        return None, None, dout[plan.segment_ids(csrptr_t, indices_t, ctx.side)], None, None, None


def incidence_sum(csrptr_t, indices_t, val, side="hyperedge", num_nodes=None, heads=1):
    """Segment sums of a value per incidence (float32 [nnz], aligned with indices_t): out[e] = sum over hyperedge e's
    members (side='hyperedge', [M]) or out[v] = sum over vertex v's hyperedges (side='vertex', [N]) -- e.g. the weighted
    degrees of a probabilistic H.  Deterministic, no atomics (hg_incidence_sum_f32); differentiable in val.  num_nodes: N;
    without it N is taken as the largest member id + 1 (read back from the device on every call, and vertices beyond it,
    which are in no hyperedge, get no row) -- pass it.  heads = H > 1: val holds nnz * H elements ([nnz, H], head
    fastest) and the sums come back [M, H] / [N, H], one column per head; heads = 1 is the call above, unchanged."""
    if heads == 1:
        v = _flat(val) if isinstance(val, torch.Tensor) else val
    else:
        _heads(heads)
        v = _per_head(val, heads) if isinstance(val, torch.Tensor) else val
    nnz = indices_t.numel() if isinstance(indices_t, torch.Tensor) else 0
    _segment_args("incidence_sum", csrptr_t, indices_t, (("val", v),), (nnz * heads,), side, None, heads)
    if v is None:
        raise TypeError("val must be a float32 tensor")
    N = int(num_nodes) if num_nodes is not None else (int(indices_t.max()) + 1 if nnz else 0)
    if not (torch.is_grad_enabled() and v.requires_grad):
        return cached_plan(N, csrptr_t, indices_t).incidence_sum(csrptr_t, indices_t, v, side, heads=heads)
    return _IncidenceSum.apply(csrptr_t, indices_t, v, N, side, heads)


# ---- module `hgnnaggr` (hgnnaggr.cc:122-151) ---------------------------------

def hgnnaggr(balan_key, balan_row, group_st, group_ed, csrptr_t, indices_t, node_feat, degE, degV, W, options=None):
    """hgnnaggr with fused degE and degV.  (`options`: this backend's per-call Options; the reference's ten
    positional arguments are unchanged.)"""
    return _sum_aggr(balan_key, balan_row, group_st, group_ed, csrptr_t, indices_t, node_feat, degE, degV, W, options)


def _sum_aggr(balan_key, balan_row, group_st, group_ed, csrptr_t, indices_t, node_feat, degE, degV, W, options):
    opt = _opt(options)
    # nothing to differentiate (inference, or a feature tensor outside the graph): the operator itself, without the
    # autograd node -- a third of the host cost of a launch-bound call
    if not (torch.is_grad_enabled() and _any_requires_grad(node_feat, degE, degV, W)):
        return _forward((balan_key, balan_row, group_st, group_ed), csrptr_t, indices_t, node_feat, degE, degV, W, opt)
    return _SumAggr.apply(balan_key, balan_row, group_st, group_ed, csrptr_t, indices_t, node_feat, degE, degV, W, opt)


def _edge_sizes(csrptr_t):
    return (csrptr_t[1:] - csrptr_t[:-1]).to(torch.float32)


class _MeanF1(torch.autograd.Function):
    """first hop = mean (HGNNAggr_MeanF1, hgnnaggr.cc:66-90; kernels hgnnaggr_cuda.cu:86-142):
    the hyperedge sum is scaled by degE*W/|e| (one factor, as the reference computes it), the
    second hop is the ordinary one.  Backward = the same operator on grad_out (the reference's
    backward kernel differs only in where it divides by |e|).  degE / degV / W get no gradient from this node."""

    @staticmethod
    def forward(ctx, csrptr_t, indices_t, node_feat, degE, degV, W):
        _check_index(csrptr_t, "csrptr_t")
        s = _flat(degE) * _flat(W) / _edge_sizes(csrptr_t)
        s = torch.where(torch.isfinite(s), s, torch.zeros_like(s))  # empty hyperedge: never read
        ctx.save_for_backward(csrptr_t, indices_t, s, _flat(degV))
        plan = cached_plan(node_feat.shape[0], csrptr_t, indices_t)
        return plan.aggregate(csrptr_t, indices_t, node_feat, s, _flat(degV), None)

    @staticmethod
    def backward(ctx, grad_out):
        csrptr_t, indices_t, s, degV = ctx.saved_tensors
        plan = cached_plan(grad_out.shape[0], csrptr_t, indices_t)
        g = plan.aggregate(csrptr_t, indices_t, grad_out.contiguous(), s, degV, None)
        return None, None, g, None, None, None


class _MaxF1(torch.autograd.Function):
    """first hop = per-column max with arg-max table (HGNNAggr_MaxF1, hgnnaggr.cc:92-120;
    kernels hgnnaggr_cuda.cu:144-208).  Loop bounds use M, not the reference's N (defect D2).  degE / degV / W get no
    gradient from this node."""

    @staticmethod
    def forward(ctx, csrptr_t, indices_t, node_feat, degE, degV, W):
        _check_feat(node_feat, "node_feat")
        _check_index(csrptr_t, "csrptr_t")
        _check_index(indices_t, "indices_t")
        N, F = node_feat.shape
        M = csrptr_t.numel() - 1
        degE, degV, W = _flat(degE), _flat(degV), _flat(W)
        dev = node_feat.device
        Xe = torch.empty((M, F), dtype=torch.float32, device=dev)
        record = torch.empty((M, F), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().hg_gather_max_f32(M, F, _ptr(csrptr_t), _ptr(indices_t), _ptr(node_feat),
                                                    _ptr(degE), _ptr(W), _ptr(Xe), _ptr(record),
                                                    _stream_handle(dev)))
        plan = cached_plan(N, csrptr_t, indices_t)
        out = plan.gather_rows(1, csrptr_t, indices_t, Xe, degV, None)
        ctx.save_for_backward(csrptr_t, indices_t, degE, degV, W, record)
        ctx.mark_non_differentiable(record)
        return out, record

    @staticmethod
    def backward(ctx, grad_out, _grad_record):
        csrptr_t, indices_t, degE, degV, W, record = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        N, F = grad_out.shape
        M = csrptr_t.numel() - 1
        plan = cached_plan(N, csrptr_t, indices_t)
        T = plan.gather_rows(0, csrptr_t, indices_t, grad_out, degE, W)  # (sum grad) * degE * W
        g = torch.empty((N, F), dtype=torch.float32, device=grad_out.device)
        with torch.cuda.device(grad_out.device):
            _lib.check(_lib.lib().hg_scatter_record_f32(N, M, F, _ptr(T), _ptr(record), _ptr(degV), _ptr(g),
                                                        _stream_handle(grad_out.device)))
        return None, None, g, None, None, None


def hgnnaggr_mean(csrptr_t, indices_t, node_feat, degE, degV, W):
    """hgnnaggr with f1 mean (hgnnaggr.cc:131-136)."""
    return _MeanF1.apply(csrptr_t, indices_t, node_feat, degE, degV, W)


def hgnnaggr_max(csrptr_t, indices_t, node_feat, degE, degV, W):
    """hgnnaggr with f1 max (hgnnaggr.cc:138-144): returns [out, record_table]."""
    return list(_MaxF1.apply(csrptr_t, indices_t, node_feat, degE, degV, W))


# ---- module `unignnaggr` (unignnaggr.cc:81-102) ------------------------------

def unignnaggrdeg(balan_key, balan_row, group_st, group_ed, csrptr_t, indices_t, node_feat, degE, degV, options=None):
    return _sum_aggr(balan_key, balan_row, group_st, group_ed, csrptr_t, indices_t, node_feat, degE, degV, None, options)


def unignnaggr(balan_key, balan_row, group_st, group_ed, csrptr_t, indices_t, node_feat, options=None):
    return _sum_aggr(balan_key, balan_row, group_st, group_ed, csrptr_t, indices_t, node_feat, None, None, None, options)


# the names the reference's Python wrapper actually calls (unignnconv.py:7,10);
# the reference module does not export them (defect D4), this one does
unignnconvdeg = unignnaggrdeg
unignnconv = unignnaggr


# ---- wrappers (source/python/hgnnaggr.py, unignnconv.py) ----------------------

def HGNNAggr(hyperg, in_feat, degE, degV, Wdiag, first_aggr="sum", options=None):
    """first_aggr is accepted and ignored, as in the reference (hgnnaggr.py:6-7);
    it has a default so the reference test's 5-argument call works (hgnn_test.py:89)."""
    return hgnnaggr(hyperg.group_key, hyperg.group_row, hyperg.group_start, hyperg.group_end,
                    hyperg.H_T_csrptr, hyperg.H_T_colind, in_feat, degE, degV, Wdiag, options=options)


def HGNNAggrLinear(hyperg, in_feat, weight, degE, degV, Wdiag, options=None):
    """HGNNAggr(hyperg, in_feat . weight^T, ...) in one pass."""
    return hgnnaggr_linear(hyperg.H_T_csrptr, hyperg.H_T_colind, in_feat, weight, degE, degV, Wdiag, options=options)


def UniGNNConvLinear(dl, in_feat, weight, options=None):
    """UniGNNConv(dl, in_feat . weight^T) in one pass."""
    return hgnnaggr_linear(dl.H_T_csrptr, dl.H_T_colind, in_feat, weight, options=options)


def UniGNNConvdeg(dl, in_feat, degE, degV, options=None):
    return unignnaggrdeg(dl.group_key, dl.group_row, dl.group_start, dl.group_end,
                         dl.H_T_csrptr, dl.H_T_colind, in_feat, degE, degV, options=options)


def UniGNNConv(dl, in_feat, options=None):
    return unignnaggr(dl.group_key, dl.group_row, dl.group_start, dl.group_end,
                      dl.H_T_csrptr, dl.H_T_colind, in_feat, options=options)
