"""bf16 features in the sum aggregation (-m gpu).  The contract (include/hg_aggr.h, hg_aggr_fused_bf16): X and Y bf16,
everything between them fp32, each element accumulated in the fp32 call's order and rounded once.  So for F % 4 == 0
    plan.aggregate(Xb, ..., variant=v) == plan.aggregate(Xb.float(), ..., variant=v).to(torch.bfloat16)
bit for bit, v in {auto, fused, pull}: that is checked with no tolerance.  Where the invariant is not claimed (padded
widths, X above 2 GiB) the result is held against float64 computed from the bf16 inputs at
|y - truth| <= 2^-8 |truth| + 1e-5 * mass (mass: the element's l1 mass).  Features are randn.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from hypergef_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VARIANTS = ("auto", "fused", "pull")


def _make(name):
    return {
        "cora": synth.cora_shape,
        "citeseer": synth.citeseer_shape,
        "pubmed": synth.pubmed_shape,
        "ragged": lambda: synth.random_incidence(700, 450, 7.0, seed=3, empty_frac=0.1),
        "dense": lambda: synth.random_incidence(300, 40, 150.0, seed=6),
        "powerlaw": lambda: synth.powerlaw(20000, 60000, seed=3, max_size=4096),
    }[name]()


def _scales(inc, seed=0):
    from oracle import oracle as orc
    degE, degV = orc.degrees(inc.N, inc.M, inc.csrptr, inc.colind)
    W = (np.random.default_rng(seed).random(inc.M) + 0.5).astype(np.float32)
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (degE, degV, W)]


def _graph(inc):
    return torch.from_numpy(inc.csrptr).to(DEV), torch.from_numpy(inc.colind).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_invariant(plan, ptr, ind, Xb, scales, variant, what):
    degE, degV, W = scales
    yb = plan.aggregate(ptr, ind, Xb, degE, degV, W, variant=variant)
    yf = plan.aggregate(ptr, ind, Xb.float(), degE, degV, W, variant=variant)
    assert yb.dtype == torch.bfloat16 and yb.shape == Xb.shape
    want = yf.to(torch.bfloat16)
    same = _bits(yb) == _bits(want)
    if not bool(same.all()):
        i = torch.nonzero(~same)[0].tolist()
        raise AssertionError("%s: %d elements differ, first %s: got %r want %r (fp32 %r)" % (
            what, int((~same).sum()), i, float(yb[i[0], i[1]]), float(want[i[0], i[1]]), float(yf[i[0], i[1]])))


def _float64(inc, X, degE=None, degV=None, W=None):
    import scipy.sparse as sp
    HT = sp.csr_matrix((np.ones(inc.nnz), inc.colind, inc.csrptr), shape=(inc.M, inc.N))
    Xe = HT @ np.asarray(X, np.float64)
    if degE is not None:
        Xe *= np.asarray(degE, np.float64).reshape(-1, 1)
    if W is not None:
        Xe *= np.asarray(W, np.float64).reshape(-1, 1)
    Y = HT.T.tocsr() @ Xe
    if degV is not None:
        Y *= np.asarray(degV, np.float64).reshape(-1, 1)
    return Y


def _assert_bf16_bound(y, inc, X, degE=None, degV=None, W=None, rel=2.0 ** -8, what=""):
    """|y - truth| <= rel |truth| + 1e-5 mass, truth in float64 from the bf16 inputs."""
    c = lambda t: None if t is None else t.detach().double().cpu().numpy()
    Xn, dE, dV, Wn = c(X), c(degE), c(degV), c(W)
    truth = _float64(inc, Xn, dE, dV, Wn)
    mass = _float64(inc, np.abs(Xn), None if dE is None else np.abs(dE), None if dV is None else np.abs(dV),
                    None if Wn is None else np.abs(Wn))
    got = y.detach().double().cpu().numpy()
    bad = np.abs(got - truth) > rel * np.abs(truth) + 1e-5 * mass
    assert not bad.any(), "%s: %d of %d off, max err %g" % (what, int(bad.sum()), bad.size, float(np.abs(got - truth).max()))


@pytest.mark.parametrize("shape", ["cora", "citeseer", "pubmed", "ragged", "dense", "powerlaw"])
def test_bf16_equals_fp32_rounded_once(hg, shape):
    from hypergef_amd.plan import Plan
    inc = _make(shape)
    ptr, ind = _graph(inc)
    plan = Plan.from_tensors(inc.N, ptr, ind)
    scales = _scales(inc)
    g = torch.Generator(device=DEV).manual_seed(1)
    for F in (4, 8, 16, 32, 64, 128, 260):
        Xb = torch.randn(inc.N, F, device=DEV, generator=g).to(torch.bfloat16)
        for v in VARIANTS:
            _assert_invariant(plan, ptr, ind, Xb, (None, None, None), v, "%s F=%d %s unweighted" % (shape, F, v))
            _assert_invariant(plan, ptr, ind, Xb, scales, v, "%s F=%d %s weighted" % (shape, F, v))


@pytest.mark.parametrize("opts", [dict(fused_tile_bytes=4096), dict(t_big=16), dict(t_big=8, fused_tile_bytes=8192)])
@pytest.mark.parametrize("shape", ["pubmed", "powerlaw"])
def test_bf16_invariant_with_materialisation_and_pieces(hg, shape, opts):
    """Plan options that force materialised hyperedges (t_big) and split vertices (small tiles): the pre-pass, the
    pieces' partial rows and their fixups stay fp32 in the bf16 call."""
    from hypergef_amd import plan as planmod
    inc = _make(shape)
    ptr, ind = _graph(inc)
    plan = planmod.Plan.from_tensors(inc.N, ptr, ind, planmod.make_opts(**opts))
    scales = _scales(inc, 2)
    g = torch.Generator(device=DEV).manual_seed(2)
    for F in (16, 32, 64):
        Xb = torch.randn(inc.N, F, device=DEV, generator=g).to(torch.bfloat16)
        for v in VARIANTS:
            _assert_invariant(plan, ptr, ind, Xb, scales, v, "%s %s F=%d %s" % (shape, opts, F, v))
            _assert_invariant(plan, ptr, ind, Xb, (None, None, None), v, "%s %s F=%d %s plain" % (shape, opts, F, v))


@pytest.mark.parametrize("shape", ["cora", "ragged", "powerlaw"])
def test_bf16_against_float64_padded_widths(hg, shape):
    from hypergef_amd.plan import Plan
    inc = _make(shape)
    ptr, ind = _graph(inc)
    plan = Plan.from_tensors(inc.N, ptr, ind)
    degE, degV, W = _scales(inc, 3)
    g = torch.Generator(device=DEV).manual_seed(3)
    for F in (1, 3, 33, 67, 32):
        Xb = torch.randn(inc.N, F, device=DEV, generator=g).to(torch.bfloat16)
        for v in VARIANTS:
            y = plan.aggregate(ptr, ind, Xb, degE, degV, W, variant=v)
            assert y.dtype == torch.bfloat16 and tuple(y.shape) == (inc.N, F) and y.is_contiguous()
            _assert_bf16_bound(y, inc, Xb, degE, degV, W, what="%s F=%d %s" % (shape, F, v))
            y = plan.aggregate(ptr, ind, Xb, variant=v)
            _assert_bf16_bound(y, inc, Xb, what="%s F=%d %s plain" % (shape, F, v))


@pytest.mark.parametrize("shape", ["cora", "pubmed", "powerlaw", "ragged"])
def test_bf16_outputs_stay_inside_their_buffers(hg, shape):
    """Y inside a larger bf16 buffer, the workspace inside a larger one, both sentinel-filled: not one byte outside
    changes (padded widths included, whose Y is written through a copy)."""
    from hypergef_amd.plan import Plan
    inc = _make(shape)
    ptr, ind = _graph(inc)
    plan = Plan.from_tensors(inc.N, ptr, ind)
    G = 4096
    sentinel = 7.25
    for F in (32, 20, 64, 4, 7):
        Xb = torch.randn(inc.N, F, device=DEV).to(torch.bfloat16)
        nws = plan.workspace_bytes((F + 3) // 4 * 4)
        for v in VARIANTS:
            for off in (0, 4):  # 4 elements = 8 bytes: the smallest alignment the kernels take as it is
                ybuf = torch.full((G + off + inc.N * F + G,), sentinel, device=DEV, dtype=torch.bfloat16)
                wbuf = torch.full((G + nws + G,), 0xA5, device=DEV, dtype=torch.uint8)
                Y = ybuf[G + off:G + off + inc.N * F].view(inc.N, F)
                ws = wbuf[G:G + nws] if F % 4 == 0 else None
                plan.aggregate(ptr, ind, Xb, variant=v, out=Y, workspace=ws)
                torch.cuda.synchronize()
                assert bool((ybuf[:G + off] == sentinel).all()) and bool((ybuf[G + off + inc.N * F:] == sentinel).all()), \
                    (shape, F, v, off)
                assert bool((wbuf[:G] == 0xA5).all()) and bool((wbuf[G + nws:] == 0xA5).all()), (shape, F, v, off)
                ref = plan.aggregate(ptr, ind, Xb, variant=v)
                assert bool((_bits(Y) == _bits(ref)).all()), (shape, F, v, off)


def test_bf16_x_above_2gib_as_bf16(hg):
    """X of more than 2 GiB in bf16 (the 64-bit-offset path of every kernel that reads it) against float64."""
    from hypergef_amd.plan import Plan
    free, _ = torch.cuda.mem_get_info()
    base = synth.random_incidence(2000, 1500, 6.0, seed=11)
    F = 1024
    reps = (1 << 31) // (base.N * F * 2) + 1  # X: just past 2 GiB in bf16
    inc = synth.replicate_block_diagonal(base, reps)
    need = inc.N * F * (2 + 2 + 4 + 4) + inc.M * F * 4 * 2
    if need > free * 0.8:
        pytest.skip("needs %.1f GB of device memory" % (need / 1e9))
    ptr, ind = _graph(inc)
    plan = Plan.from_tensors(inc.N, ptr, ind)
    degE, degV, W = _scales(inc, 4)
    Xb = torch.randn(inc.N, F, device=DEV).to(torch.bfloat16)
    assert Xb.numel() * 2 > (1 << 31)
    # truth for a sample of output rows: the block-diagonal batch keeps every row's support in its own replica
    for v in VARIANTS:
        y = plan.aggregate(ptr, ind, Xb, degE, degV, W, variant=v)
        torch.cuda.synchronize()
        for r0 in (0, (reps - 1) * base.N):  # first and last replica, the latter beyond 2 GiB of X
            Xs = Xb[r0:r0 + base.N]
            sl = slice(r0, r0 + base.N)
            eb = slice(r0 // base.N * base.M, r0 // base.N * base.M + base.M)
            _assert_bf16_bound(y[sl], base, Xs, degE[eb], degV[sl], W[eb], what="2 GiB %s replica at %d" % (v, r0))
        del y


def test_bf16_autograd(hg):
    from hypergef_amd import _lib, ops
    inc = _make("cora")
    hyperg = _hypergraph(inc)
    F = 32
    degE, degV = hyperg.degE, hyperg.degV
    W = torch.rand(inc.M, 1, device=DEV) + 0.5
    X0 = torch.randn(inc.N, F, device=DEV).to(torch.bfloat16)
    G0 = torch.randn(inc.N, F, device=DEV).to(torch.bfloat16)
    L = _lib.lib()
    real = L.hg_aggr_fused_f32
    calls = {"f32": 0}

    def counting(*a):
        calls["f32"] += 1
        return real(*a)

    grads = {}
    for mode in ("reference", "adjoint"):
        x = X0.clone().requires_grad_(True)
        with ops.options(backward=mode):
            y = ops.HGNNAggr(hyperg, x, degE, degV, W)
            assert y.dtype == torch.bfloat16
            L.hg_aggr_fused_f32 = counting
            try:
                y.backward(G0)
                torch.cuda.synchronize()
            finally:
                L.hg_aggr_fused_f32 = real
        assert x.grad.dtype == torch.bfloat16
        grads[mode] = x.grad
    assert calls["f32"] == 0, "the bf16 backward ran an fp32 aggregation"
    # reference mode: the backward is the same operator on grad_out, so the invariant holds for the gradient too
    with ops.options(backward="reference"):
        want = ops.HGNNAggr(hyperg, G0.float(), degE, degV, W).to(torch.bfloat16)
    assert bool((_bits(grads["reference"]) == _bits(want)).all())
    # adjoint mode (degV moved to the front, product rounded to bf16 once): within 2^-7 of the l1 mass
    g64 = G0.double().cpu().numpy()
    dE, dV, Wn = degE.double().cpu().numpy(), degV.double().cpu().numpy(), W.reshape(-1).double().cpu().numpy()
    # the adjoint of Dv H De W H^T is H De W H^T Dv: degV first
    truth = _float64(inc, g64 * dV.reshape(-1, 1), dE, None, Wn)
    mass = _float64(inc, np.abs(g64) * np.abs(dV).reshape(-1, 1), np.abs(dE), None, np.abs(Wn))
    got = grads["adjoint"].double().cpu().numpy()
    assert (np.abs(got - truth) <= 2.0 ** -7 * mass + 1e-6).all()


def _hypergraph(inc):
    import hypergef_amd as hg
    return hg.HyperGraph.from_incidence(inc, DEV, data_name="cora")


class _Args:
    def __init__(self, model):
        self.model, self.activation, self.input_drop, self.dropout = model, "relu", 0.0, 0.0
        self.backend = "hgsys"


@pytest.mark.parametrize("model", ["HGNN", "UniGIN", "UniGCNII"])
def test_bf16_models_train(hg, model):
    import copy
    import torch.nn.functional as Fn
    from hypergef_amd import models
    inc = _make("cora")
    hyperg = _hypergraph(inc)
    torch.manual_seed(0)
    nfeat, nhid, nclass = 64, 32, 7
    if model == "UniGCNII":
        m32 = models.UniGCNII(_Args("UniGCNII"), hyperg, nfeat, nhid, nclass, 2, 1).to(DEV)
    else:
        m32 = models.HGsysHGNN(_Args(model), hyperg, nfeat, nhid, nclass, 2, "sum", 1).to(DEV)
    m16 = copy.deepcopy(m32).to(torch.bfloat16)
    with torch.no_grad():  # the same weights: the fp32 model gets the bf16 model's values
        for p32, p16 in zip(m32.parameters(), m16.parameters()):
            p32.copy_(p16.float())
    X = torch.randn(inc.N, nfeat, device=DEV).to(torch.bfloat16)
    y = torch.randint(0, nclass, (inc.N,), device=DEV)
    l32 = Fn.nll_loss(m32(X.float()), y)
    l16 = Fn.nll_loss(m16(X), y)
    assert l16.dtype == torch.bfloat16
    assert abs(float(l16) - float(l32)) <= 2e-2 * abs(float(l32)), (float(l16), float(l32))
    assert hyperg.degE.dtype == torch.float32 and hyperg.degV.dtype == torch.float32
    opt = torch.optim.Adam(m16.parameters(), lr=0.01)
    first = None
    for _ in range(10):
        opt.zero_grad()
        loss = Fn.nll_loss(m16(X), y)
        loss.backward()
        for p in m16.parameters():
            assert p.grad is None or p.grad.dtype == torch.bfloat16
        opt.step()
        first = float(loss) if first is None else first
    assert float(Fn.nll_loss(m16(X), y)) < first


@pytest.mark.parametrize("model", ["HGNN", "UniGCNII"])
@pytest.mark.parametrize("capture", [False, True])
def test_bf16_driver(hg, model, capture):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "hgsys.py"), "--model", model, "--dname", "cora",
           "--epochs", "3", "--dtype", "bfloat16"]
    cmd += ["--graph", "--graph-train"] if capture else ["--no-graph"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "avg epoch time" in r.stdout and "avg inference time" in r.stdout
    assert "failed" not in r.stdout, r.stdout[-2000:]
    if capture:
        assert r.stdout.count("as a hipGraph replay") == 2, r.stdout[-2000:]


def test_bf16_hipgraph_replay(hg):
    from hypergef_amd.plan import Plan
    inc = _make("pubmed")
    ptr, ind = _graph(inc)
    plan = Plan.from_tensors(inc.N, ptr, ind)
    degE, degV, W = _scales(inc)
    X = torch.randn(inc.N, 32, device=DEV).to(torch.bfloat16)
    eager = plan.aggregate(ptr, ind, X, degE, degV, W)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        plan.aggregate(ptr, ind, X, degE, degV, W)
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        Ys = plan.aggregate(ptr, ind, X, degE, degV, W)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert bool((_bits(Ys) == _bits(eager)).all())


def test_bf16_errors(hg):
    from hypergef_amd import _lib, ops
    from hypergef_amd.plan import Plan
    inc = _make("cora")
    hyperg = _hypergraph(inc)
    ptr, ind = _graph(inc)
    plan = Plan.from_tensors(inc.N, ptr, ind)
    X = torch.randn(inc.N, 32, device=DEV).to(torch.bfloat16)
    for v in ("push_atomic", "push_groups"):
        with pytest.raises((TypeError, _lib.HgError)):
            with ops.options(variant=v):
                ops.HGNNAggr(hyperg, X, hyperg.degE, hyperg.degV, torch.ones(inc.M, 1, device=DEV))
    with pytest.raises((TypeError, _lib.HgError)):
        plan.aggregate(ptr, ind, X, variant="push_atomic")
    with pytest.raises(TypeError):
        plan.aggregate(ptr, ind, X.half())
    with pytest.raises(TypeError):
        plan.aggregate(ptr, ind, X, out=torch.empty(inc.N, 32, device=DEV))
    with pytest.raises(TypeError):
        plan.aggregate(ptr, ind, X.float(), out=torch.empty(inc.N, 32, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(TypeError):  # the fused linear entry point stays fp32
        plan.aggregate_linear(ptr, ind, X, torch.randn(16, 32, device=DEV).to(torch.bfloat16))
    torch.cuda.synchronize()
    # the C ABI itself: F = 6 and an X only 2-byte aligned are refused with a message, nothing launched
    L = _lib.lib()
    ws = torch.empty(plan.workspace_bytes(8), dtype=torch.uint8, device=DEV)
    Y = torch.empty(inc.N * 8 + 8, dtype=torch.bfloat16, device=DEV)
    Xr = torch.zeros(inc.N * 8 + 8, dtype=torch.bfloat16, device=DEV)
    vp = ctypes.c_void_p
    for F, xp in ((6, Xr.data_ptr()), (8, Xr.data_ptr() + 2)):
        rc = L.hg_aggr_fused_bf16(plan._h, F, vp(ptr.data_ptr()), vp(ind.data_ptr()), vp(xp), None, None, None,
                                  vp(Y.data_ptr()), vp(ws.data_ptr()), ws.numel(), _lib.HG_VARIANT_AUTO, None)
        assert rc == _lib.HG_ERR_UNSUPPORTED, (F, rc)
        assert L.hg_last_error()
    torch.cuda.synchronize()


def test_bf16_padded_width_with_a_workspace_sized_for_f(hg):
    """A caller that sizes its workspace with workspace_bytes(F) for a width the bf16 path pads (F % 4 != 0) gets the
    same result as without one; the padded call runs at the padded width, whose workspace may be larger."""
    from hypergef_amd.plan import Plan
    for shape in ("cora", "powerlaw"):
        inc = _make(shape)
        ptr, ind = _graph(inc)
        plan = Plan.from_tensors(inc.N, ptr, ind)
        for F in (3, 7, 33):
            Xb = torch.randn(inc.N, F, device=DEV).to(torch.bfloat16)
            for v in VARIANTS:
                if v == "fused":
                    plan.prepare(F)
                ws = torch.empty(max(plan.workspace_bytes(F), 256), dtype=torch.uint8, device=DEV)
                y = plan.aggregate(ptr, ind, Xb, variant=v, workspace=ws)
                ref = plan.aggregate(ptr, ind, Xb, variant=v)
                assert bool((_bits(y) == _bits(ref)).all()), (shape, F, v)
