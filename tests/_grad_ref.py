"""Float64 reference of every operator's gradient (CPU, plain torch): test infrastructure only.

The aggregation is  A(x) = Dv H De W H^T x  (H [N, M] the incidence, Dv = diag(degV), De W = diag(degE * W); any of the
three may be absent).  Its two documented backward rules (hypergef_amd/ops.py):
  * "reference": the gradient of x is A(g) -- forward(grad_out), as hgnnaggr.cc:51-64 computes it;
  * "adjoint":   the true transpose, A^T(g) = H De W H^T Dv g.
Both are float64 autograd Functions here, and the layer formulas below are written with them, so that
torch.autograd.grad in float64 yields the value every input gradient of the library should have under either rule.
An empty hyperedge (degE = 1/0 = inf) contributes nothing, as in models.TorchHGNNConv (nan_to_num).

Error scale.  Every expression here is multilinear in its inputs once the relu mask is fixed.  Its "mass" is the same
expression evaluated on absolute values (|X|, |G|, |M|, |R|, |ca|, |cb|, |degE|, |degV|, |W|) under the same mask:
the sum of the absolute values of all the terms that were added to form an element.  A computation that rounds each
intermediate z with relative error <= u is then off by at most (number of roundings on the path) * u * mass, whatever
the order of its sums, because each rounding error is bounded by u * |z| <= u * mass(z) and flows through the rest of
the path by the same absolute-valued linear maps that build the mass.  The checks are |got - ref| <= c * max(mass,
TINY) per element, with c below.
"""
import torch

F64 = torch.float64

# fp32 paths: 1e-5 = 168 fp32 units (2^-24) of the mass.  Each fp32 rounding costs at most one unit; the longest paths
# here (a 25k-term hub sum, a 20k-row weight-gradient contraction) stay far inside that in any blocked or tree order,
# and this is the bound the forward tests already use for the any-order kernels (_assert_close_any_order).
FP32_C = 1e-5
# bf16 rounding of a value z (round to nearest, 8 significant bits): |error| <= 2^-8 |z| <= 2^-8 mass(z).
BF16_ROUNDING = 2.0 ** -8
# Floor of the scale: four units of fp32's smallest subnormal (2^-149) per c -- a gradient scaled by a subnormal factor
# (ca = 2^-130) is itself subnormal, where fp32 has absolute, not relative, resolution.  Far below any normal value.
TINY = 4 * 2.0 ** -149 / FP32_C


def any_order_c(inc):
    """Per-vertex c ([N, 1]) for the push kernels, whose fp32 atomics add a vertex's terms in arbitrary order.  A sum
    of n terms added one by one in any order is off by at most (n - 1) u * (sum of |terms|) (recursive summation,
    u = 2^-24); a vertex's value is a sum over its deg(v) hyperedges of sums over at most max |e| members, then three
    scalings: n_v = deg(v) + max |e| + 3.  That exceeds FP32_C only on hub rows (the power-law shape's hub has 25542
    hyperedges), where one order of adding can indeed drift past 168 units of the mass."""
    import numpy as np
    deg = np.bincount(inc.colind, minlength=inc.N).astype(np.float64)
    sizes = np.diff(inc.csrptr)
    widest = np.zeros(inc.N)
    np.maximum.at(widest, inc.colind, np.repeat(sizes, sizes).astype(np.float64))
    n = torch.from_numpy(deg + widest + 3).reshape(-1, 1)
    return torch.clamp(n * 2.0 ** -24, min=FP32_C)


def bf16_c(roundings):
    """c for a path with `roundings` bf16 roundings of intermediates (2^-8 of the mass each, see above) plus the fp32
    accumulation inside the kernels and GEMMs (FP32_C)."""
    return roundings * BF16_ROUNDING + FP32_C


def f64(t):
    """A tensor (any device, fp32 / bf16 / numpy) as a CPU float64 tensor: exact for fp32 and bf16 values."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    return t.detach().to("cpu", F64)


class Graph:
    """H from an Incidence (H_T in CSR: row = hyperedge, entries = member vertices), the scales as float64 vectors."""

    def __init__(self, inc, degE=None, degV=None, W=None):
        import numpy as np
        self.inc = inc
        self.N, self.M = inc.N, inc.M
        self.V = torch.from_numpy(inc.colind.astype(np.int64))
        self.E = torch.from_numpy(np.repeat(np.arange(inc.M, dtype=np.int64), np.diff(inc.csrptr)))
        self.degE = None if degE is None else f64(degE).reshape(-1)
        self.degV = None if degV is None else f64(degV).reshape(-1)
        self.W = None if W is None else f64(W).reshape(-1)
        se = None
        if self.degE is not None:
            se = torch.nan_to_num(self.degE, posinf=0.0)  # empty hyperedge: 1/0, never summed into anything
        if self.W is not None:
            se = self.W.clone() if se is None else se * self.W
        self.se = se
        self._abs = None

    def abs(self):
        """The same graph with |degE|, |degV|, |W|: the mass of an expression is evaluated on it."""
        if self._abs is None:
            g = Graph.__new__(Graph)
            g.__dict__.update(self.__dict__)
            g.degE = None if self.degE is None else self.degE.abs()
            g.degV = None if self.degV is None else self.degV.abs()
            g.W = None if self.W is None else self.W.abs()
            g.se = None if self.se is None else self.se.abs()
            g._abs = g
            self._abs = g
        return self._abs

    def v2e(self, x):  # H^T x
        return torch.zeros(self.M, x.shape[1], dtype=x.dtype).index_add_(0, self.E, x[self.V])

    def e2v(self, xe):  # H xe
        return torch.zeros(self.N, xe.shape[1], dtype=xe.dtype).index_add_(0, self.V, xe[self.E])

    def A(self, x):
        """Dv H De W H^T x."""
        xe = self.v2e(x)
        if self.se is not None:
            xe = xe * self.se.reshape(-1, 1)
        y = self.e2v(xe)
        return y if self.degV is None else y * self.degV.reshape(-1, 1)

    def AT(self, g):
        """A^T g = H De W H^T Dv g."""
        if self.degV is not None:
            g = g * self.degV.reshape(-1, 1)
        ge = self.v2e(g)
        if self.se is not None:
            ge = ge * self.se.reshape(-1, 1)
        return self.e2v(ge)

    def aggr(self, x, rule):
        """A(x) as an autograd node whose backward follows `rule` ("reference" or "adjoint")."""
        return {"reference": _Reference, "adjoint": _Adjoint}[rule].apply(x, self)


class _Reference(torch.autograd.Function):
    """The reference's rule: the gradient is A(g) (hgnnaggr.cc:51-64) -- the transpose only without degV."""

    @staticmethod
    def forward(ctx, x, graph):
        ctx.graph = graph
        return graph.A(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.graph.A(g), None


class _Adjoint(torch.autograd.Function):
    """The exact transpose A^T(g)."""

    @staticmethod
    def forward(ctx, x, graph):
        ctx.graph = graph
        return graph.A(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.graph.AT(g), None


# ---- the operators' formulas ----------------------------------------------------------------------------------------
# Each takes float64 tensors (with requires_grad where a gradient is wanted) and plain numbers; `graph` is a Graph, or
# its .abs() for the mass.

def sum_aggr(graph, x, rule):
    """hgnnaggr / unignnaggrdeg / unignnaggr: A(x)."""
    return graph.aggr(x, rule)


def hgnnaggr_linear(graph, x, weight, rule):
    """ops.hgnnaggr_linear: Aggr(X . W^T)."""
    return graph.aggr(x @ weight.t(), rule)


def aggr_res_linear(graph, x, m, rule, residual=None, ca=1.0, cb=0.0, mask=None):
    """ops.aggr_res_linear: act((ca Aggr(X) + cb R) . M^T).  `mask` (bool, [N, F_out]) is the relu's: taken from the
    kernel's own output (out > 0, what threshold_backward reads), None without relu.  cb: a number or a 0-d / 1-element
    tensor."""
    t = graph.aggr(x, rule) * ca
    if residual is not None:
        t = t + residual * (cb.reshape(()) if isinstance(cb, torch.Tensor) else cb)
    p = t @ m.t()
    return p if mask is None else p * mask.to(F64)


def aggr_res_linear_pre(graph, x, m, residual=None, ca=1.0, cb=0.0):
    """The pre-activation (ca Aggr(X) + cb R) . M^T itself, with nothing requiring a gradient (the relu mask's check)."""
    with torch.no_grad():
        return aggr_res_linear(graph, x, m, "reference", residual, ca, cb, None)


def unigin(graph, x, weight, eps, rule):
    """HyperGsysUinGINConv (unigin.py:20-22): (1 + eps) X W^T + Aggr(X W^T), unweighted Aggr.  The mass evaluates
    1 + |eps| >= |1 + eps|: an upper bound, valid for the fused form too."""
    z = x @ weight.t()
    return z * (1 + eps.reshape(())) + graph.aggr(z, rule)


def unigcnii(graph, x, x0, weight, rule, ca, cb, c_id, c_w, mask=None):
    """HyperGsysUniGCNII (unigcnii.py:19-21): Xi = ca Aggr(X) + cb X0 (ca = 1 - alpha, cb = alpha), then
    c_id Xi + c_w Xi W^T (c_id = 1 - beta, c_w = beta), relu by `mask`.  Written as the two-step formula: its mass
    bounds the fused form's (|c_id I + c_w W| <= |c_id| I + |c_w| |W|) as well."""
    xi = graph.aggr(x, rule) * ca + x0 * cb
    out = xi * c_id + (xi @ weight.t()) * c_w
    return out if mask is None else out * mask.to(F64)


def linear(x, weight, bias=None):
    """ops.Linear: X . W^T + b."""
    y = x @ weight.t()
    return y if bias is None else y + bias


# ---- value, gradients and their masses ------------------------------------------------------------------------------

def _absolute(v):
    if isinstance(v, torch.Tensor):
        return v.detach().abs().requires_grad_(v.requires_grad)
    if isinstance(v, (int, float)):
        return abs(v)
    if isinstance(v, tuple):
        return tuple(_absolute(e) for e in v)
    return v


def evaluate(fn, graph, inputs, grad_out, wrt):
    """fn(graph, **inputs) in float64 and the gradients of <grad_out, fn> for the inputs named in `wrt`; then the same
    on absolute values (graph.abs(), |inputs|, |grad_out|): the masses.  Returns (out, {name: grad}, out_mass,
    {name: grad_mass}).  Tensors are taken as CPU float64 (exact for fp32 / bf16); inputs not in `wrt` are constants;
    `graph` may be None for a formula without aggregation."""
    def run(g, ins, go):
        ins = {k: (f64(v).requires_grad_(k in wrt) if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
               for k, v in ins.items()}
        out = fn(g, **ins)
        grads = torch.autograd.grad(out, [ins[k] for k in wrt], go, allow_unused=True) if wrt else ()
        grads = {k: (torch.zeros_like(ins[k]) if gr is None else gr) for k, gr in zip(wrt, grads)}
        return out.detach(), grads
    out, grads = run(graph, inputs, f64(grad_out))
    abs_inputs = {k: (_absolute(v) if k != "mask" else v) for k, v in inputs.items()}
    out_mass, grad_mass = run(None if graph is None else graph.abs(), abs_inputs, f64(grad_out).abs())
    return out, grads, out_mass, grad_mass


def bad_elements(got, ref, mass, c):
    """Boolean map of the elements outside |got - ref| <= c * max(mass, TINY); non-finite values are outside."""
    got = f64(got)
    ref = f64(ref).reshape(got.shape)
    mass = f64(mass).reshape(got.shape)
    tol = c * torch.clamp(mass, min=TINY)  # c: a number, or per-row [N, 1] (any_order_c)
    return ~(torch.isfinite(got) & ((got - ref).abs() <= tol))


def assert_within(got, ref, mass, c, what=""):
    """|got - ref| <= c * max(mass, TINY) per element, with the first offenders in the message."""
    c_max = float(c.max()) if isinstance(c, torch.Tensor) else c
    assert got is not None, "%s: no gradient returned" % what
    assert tuple(got.shape) == tuple(ref.shape), "%s: shape %s, want %s" % (what, tuple(got.shape), tuple(ref.shape))
    bad = bad_elements(got, ref, mass, c)
    if bool(bad.any()):
        g, r, m = f64(got).reshape(ref.shape), f64(ref), f64(mass).reshape(ref.shape)
        idx = torch.nonzero(bad)[:4].tolist()
        cells = ", ".join("%s: got %.9g want %.9g (mass %.3g)" % (tuple(i), float(g[tuple(i)]), float(r[tuple(i)]),
                                                                  float(m[tuple(i)])) for i in idx)
        raise AssertionError("%s: %d of %d elements outside %g of the mass; %s" % (
            what, int(bad.sum()), bad.numel(), c_max, cells))


def assert_mask_agrees(out, pre, pre_mass, c, what=""):
    """The relu mask the library used (its own output > 0) has the float64 pre-activation's sign wherever |pre| exceeds
    the error bound c * max(mass, TINY): near-zero pre-activations may go either way, a wrong mask may not."""
    on = f64(out) > 0
    pre = f64(pre)
    sure = pre.abs() > c * torch.clamp(f64(pre_mass), min=TINY)
    wrong = sure & (on != (pre > 0))
    assert not bool(wrong.any()), "%s: relu mask disagrees with the float64 sign at %d elements, e.g. %s" % (
        what, int(wrong.sum()), torch.nonzero(wrong)[:4].tolist())
