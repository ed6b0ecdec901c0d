"""CPU-only checks of the scale gradients (degE, degV, W): the float64 formulas of tests/_scale_grad_ref.py against torch
autograd on a dense-H restatement, the argument refusals of Plan.hyperedge_dot / Plan.rows_dot (all raised before a device
is touched) and the learn_hyperedge_weight flag of the two layers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _grad_ref as gr  # noqa: E402
import _scale_grad_ref as sr  # noqa: E402

from hypergef_amd import synth  # noqa: E402

F64 = torch.float64


def _dup_vertex():
    """A hand-made H_T: vertex 2 listed twice in hyperedge 1, an empty hyperedge 2, vertex 4 in no hyperedge."""
    ptr = np.array([0, 3, 7, 7, 9], np.int32)
    ind = np.array([0, 2, 3, 1, 2, 2, 5, 0, 5], np.int32)
    return synth.Incidence(6, 4, ptr, ind, name="dup")


SHAPES = {
    "cora": synth.cora_shape,
    "ragged": lambda: synth.random_incidence(300, 200, 5.0, seed=3, empty_frac=0.1),
    "dup": _dup_vertex,
}


def _case(shape, F, heads, weighted, seed=0):
    inc = SHAPES[shape]()
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, dtype=F64, generator=g)  # noqa: E731
    degE = torch.from_numpy(np.diff(inc.csrptr).astype(np.float64)).pow(-1)  # inf on the empty hyperedges
    degV = torch.rand(inc.N, dtype=F64, generator=g) + 0.5
    W = torch.rand(inc.M, dtype=F64, generator=g) + 0.5
    v2e = rnd(inc.nnz, heads) if weighted else None
    e2v = rnd(inc.nnz, heads) if weighted else None
    return inc, sr.Index(inc), rnd(inc.N, F), rnd(inc.N, F), degE, degV, W, v2e, e2v


def _dense(inc, w, heads, h):
    """H with head h's weights, [N, M] float64 (a vertex listed twice in a hyperedge adds up)."""
    H = torch.zeros(inc.N, inc.M, dtype=F64)
    E = np.repeat(np.arange(inc.M), np.diff(inc.csrptr))
    vals = torch.ones(inc.nnz, dtype=F64) if w is None else w.reshape(-1, heads)[:, h]
    H.index_put_((torch.from_numpy(inc.colind.astype(np.int64)), torch.from_numpy(E)), vals, accumulate=True)
    return H


def _dense_aggr(inc, x, degE, degV, W, v2e, e2v, heads):
    """Y = Dv H_e2v De W H_v2e^T X head by head on dense matrices; the empty hyperedges' factor is selected to 0."""
    live = torch.from_numpy(np.diff(inc.csrptr) > 0)
    s = torch.ones(inc.M, dtype=F64)
    for t in (degE, W):
        if t is not None:
            s = s * torch.where(live, t, torch.zeros((), dtype=F64))
    C = x.shape[1] // heads
    cols = []
    for h in range(heads):
        xe = _dense(inc, v2e, heads, h).t() @ x[:, h * C:(h + 1) * C]
        cols.append(_dense(inc, e2v, heads, h) @ (xe * s.reshape(-1, 1)))
    y = torch.cat(cols, 1)
    return y if degV is None else y * degV.reshape(-1, 1)


@pytest.mark.parametrize("present", ["EVW", "EV", "W", "V", "EW"])
@pytest.mark.parametrize("weighted,heads", [(False, 1), (True, 1), (True, 2)])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_formulas_equal_autograd_on_dense_h(shape, weighted, heads, present):
    inc, idx, x, dy, degE, degV, W, v2e, e2v = _case(shape, 4, heads, weighted)
    degE, degV, W = (t if k in present else None for k, t in (("E", degE), ("V", degV), ("W", W)))
    leaves = {k: t.clone().requires_grad_(True) for k, t in (("degE", degE), ("degV", degV), ("W", W)) if t is not None}
    y = _dense_aggr(inc, x, leaves.get("degE"), leaves.get("degV"), leaves.get("W"), v2e, e2v, heads)
    want = dict(zip(leaves, torch.autograd.grad(y, list(leaves.values()), dy)))
    torch.testing.assert_close(sr.fn(idx, x, degE, degV, W, v2e, e2v, heads), y.detach(), rtol=1e-12, atol=1e-12)
    got = sr.scale_grads(idx, x, dy, degE, degV, W, v2e, e2v, heads)
    empty = torch.from_numpy(np.diff(inc.csrptr) == 0)
    for k in ("degE", "degV", "W"):
        if k not in leaves:
            assert got[k] is None
            continue
        assert torch.isfinite(got[k]).all()
        torch.testing.assert_close(got[k], want[k], rtol=1e-11, atol=1e-11)
        if k != "degV":
            assert (got[k][empty] == 0).all(), "an empty hyperedge's gradient is exactly 0"
    if "degV" in leaves:  # a vertex in no hyperedge
        isolated = torch.from_numpy(np.bincount(inc.colind, minlength=inc.N) == 0)
        assert (got["degV"][isolated] == 0).all()


def test_fn_works_with_evaluate_and_its_mass_bounds_the_value():
    inc, idx, x, dy, degE, degV, W, v2e, e2v = _case("ragged", 4, 2, True, seed=1)
    v2e[::3] = -v2e[::3].abs()
    ins = {"x": x, "degE": degE, "degV": degV, "W": W, "v2e": v2e, "e2v": e2v, "heads": 2}
    out, grads, out_mass, grad_mass = gr.evaluate(sr.fn, idx, ins, dy, ("degE", "degV", "W"))
    closed = sr.scale_grads(idx, x, dy, degE, degV, W, v2e, e2v, 2)
    masses = sr.scale_grad_masses(idx, x, dy, degE, degV, W, v2e, e2v, 2)
    for k in ("degE", "degV", "W"):
        torch.testing.assert_close(grads[k], closed[k], rtol=1e-11, atol=1e-11)
        torch.testing.assert_close(grad_mass[k], masses[k], rtol=1e-11, atol=1e-11)
        assert (closed[k].abs() <= masses[k] * (1 + 1e-12)).all()
    assert (out.abs() <= out_mass * (1 + 1e-12)).all()


def test_edge_dot_is_q_and_is_symmetric():
    inc, idx, x, dy, degE, degV, W, v2e, e2v = _case("dup", 6, 3, True, seed=2)
    q = sr.edge_dot(idx, x, v2e, dy, e2v, 3)
    torch.testing.assert_close(q, sr.edge_dot(idx, dy, e2v, x, v2e, 3), rtol=0, atol=0)
    assert q[2] == 0 and q.shape == (inc.M,)
    S, G = sr.v2e_sum(idx, x, v2e, 3), sr.v2e_sum(idx, dy, e2v, 3)
    torch.testing.assert_close(q, (S * G).sum(1), rtol=1e-13, atol=1e-13)


# ---- refusals: all before a device is touched -------------------------------------------------------------------------

def _host_plan(inc):
    from hypergef_amd.plan import Plan, make_opts
    return Plan.from_host(inc.N, inc.M, inc.csrptr, inc.colind, opts=make_opts(host_only=True))


def _cpu_args(inc, F=4):
    return (torch.from_numpy(inc.csrptr), torch.from_numpy(inc.colind), torch.zeros(inc.N, F), torch.zeros(inc.N, F))


def test_hyperedge_dot_refusals_in_order(hg):
    inc = _dup_vertex()
    plan = _host_plan(inc)
    ptr, ind, A, B = _cpu_args(inc)
    w = torch.zeros(inc.nnz)
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="heads"):
            plan.hyperedge_dot(ptr, ind, A.double(), B, heads=bad)  # heads is decided before the dtypes
    for kw in ({"A": A.to(torch.bfloat16)}, {"B": B.double()}, {"a_weight": w.double()}, {"b_weight": w.to(torch.float16)},
               {"A": None}, {"B": "x"}):
        args = {"A": A, "B": B, "a_weight": w, "b_weight": w}
        args.update(kw)
        with pytest.raises(TypeError, match="float32"):
            plan.hyperedge_dot(ptr, ind, args["A"], args["B"][:3] if isinstance(args["B"], torch.Tensor) else args["B"],
                               args["a_weight"], args["b_weight"])  # a dtype is decided before the shapes
    with pytest.raises(ValueError, match=r"\[N = 6, F\]"):
        plan.hyperedge_dot(ptr, ind, A[:5], B[:5])
    with pytest.raises(ValueError, match=r"\[N = 6, F\]"):
        plan.hyperedge_dot(ptr, ind, A, torch.zeros(inc.N, 5))
    with pytest.raises(ValueError, match="at least 1"):
        plan.hyperedge_dot(ptr, ind, torch.zeros(inc.N, 0), torch.zeros(inc.N, 0))
    with pytest.raises(ValueError, match="no multiple of heads"):
        plan.hyperedge_dot(ptr, ind, A, B, heads=3)
    with pytest.raises(ValueError, match="a_weight must have nnz \\* heads = 18"):
        plan.hyperedge_dot(ptr, ind, A, B, a_weight=w, heads=2)
    with pytest.raises(ValueError, match="b_weight must have nnz \\* heads = 9"):
        plan.hyperedge_dot(ptr, ind, A, B, a_weight=w, b_weight=torch.zeros(inc.nnz + 1))
    with pytest.raises(TypeError, match="csrptr_t must be an int32"):  # lengths are decided before the index tensors
        plan.hyperedge_dot(ptr.long(), ind, A, B, w, w)
    with pytest.raises(RuntimeError, match="must be on a GPU"):  # and where the tensors live comes last
        plan.hyperedge_dot(ptr, ind, A, B, w, w)


def test_rows_dot_refusals_in_order(hg):
    plan = _host_plan(_dup_vertex())
    A = torch.zeros(5, 4)
    with pytest.raises(TypeError, match="A must be a float32"):
        plan.rows_dot(A.double(), A[:3])
    with pytest.raises(TypeError, match="B must be a float32"):
        plan.rows_dot(A, A.to(torch.bfloat16)[:3])
    with pytest.raises(ValueError, match="one shape"):
        plan.rows_dot(A, A[:3])
    with pytest.raises(ValueError, match="one shape"):
        plan.rows_dot(A.reshape(-1), A.reshape(-1))
    with pytest.raises(ValueError, match="F >= 1"):
        plan.rows_dot(torch.zeros(5, 0), torch.zeros(5, 0))
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        plan.rows_dot(A, A)


def test_library_exports_the_two_entries(hg):
    from hypergef_amd import _lib
    L = _lib.lib()
    for name in ("hg_hyperedge_dot_heads_f32", "hg_rows_dot_f32"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert L.hg_version() == 410
    # the refusals that need no device: a null plan, then a host-only one
    inc = _dup_vertex()
    plan = _host_plan(inc)
    assert L.hg_hyperedge_dot_heads_f32(None, 4, 1, None, None, None, None, None, None, None, None) == _lib.HG_ERR_INVALID
    for F, heads in ((4, 0), (4, 3), (0, 1)):
        assert L.hg_hyperedge_dot_heads_f32(plan._h, F, heads, None, None, None, None, None, None, None, None) == _lib.HG_ERR_INVALID
    assert L.hg_hyperedge_dot_heads_f32(plan._h, 4, 2, None, None, None, None, None, None, None, None) == _lib.HG_ERR_UNSUPPORTED
    assert b"HG_PLAN_HOST_ONLY" in L.hg_last_error()
    assert L.hg_rows_dot_f32(-1, 4, None, None, None, None) == _lib.HG_ERR_INVALID
    assert L.hg_rows_dot_f32(3, 0, None, None, None, None) == _lib.HG_ERR_INVALID
    assert L.hg_rows_dot_f32(3, 4, None, None, None, None) == _lib.HG_ERR_INVALID
    assert L.hg_rows_dot_f32(0, 4, None, None, None, None) == _lib.HG_OK


# ---- the model flag ----------------------------------------------------------------------------------------------------

def _names(module):
    return sorted(n for n, _ in module.named_parameters())


@pytest.mark.parametrize("layer", ["hgnn", "attn_additive", "attn_dot"])
def test_learn_hyperedge_weight_changes_parameters_only_when_set(hg, layer):
    inc = _dup_vertex()
    hyperg = hg.HyperGraph.from_incidence(inc, "cpu", data_name="toy")

    def build(**kw):
        torch.manual_seed(0)
        if layer == "hgnn":
            from hypergef_amd.models import HyperGsysHGNN
            return HyperGsysHGNN(hyperg, 5, 3, "sum", **kw)
        return hg.HypergraphAttnConv(hyperg, 5, 3, heads=2, score=layer.split("_")[1], **kw)

    plain, off, on = build(), build(learn_hyperedge_weight=False), build(learn_hyperedge_weight=True)
    assert _names(plain) == _names(off) and sorted(plain.state_dict()) == sorted(off.state_dict())
    assert "Wdiag" not in plain.state_dict() and not isinstance(off.Wdiag, torch.nn.Parameter)
    assert not off.Wdiag.requires_grad and torch.equal(off.Wdiag, torch.ones(inc.M))
    for k, v in plain.state_dict().items():
        assert torch.equal(v, off.state_dict()[k]) and torch.equal(v, on.state_dict()[k])
    assert _names(on) == sorted(_names(plain) + ["Wdiag"])
    assert sorted(on.state_dict()) == sorted(list(plain.state_dict()) + ["Wdiag"])
    assert isinstance(on.Wdiag, torch.nn.Parameter) and on.Wdiag.requires_grad
    assert on.Wdiag.shape == (inc.M,) and torch.equal(on.Wdiag.detach(), torch.ones(inc.M))
    off.load_state_dict(plain.state_dict())  # today's checkpoints still load
