"""What ops.incidence_softmax, ops.incidence_sum and the four softmax methods of Plan refuse, with which exception, which
text and in which order, without a device: one table per layer, each row (id, call, exception, the whole text).  Where two
faults are made at once the row's id names the one that must win.

The operators are called with ops.cached_plan replaced by a function that fails the test: every refusal is decided before
a plan -- a device -- is asked for.  The Plan methods run on a host-only plan of the toy graph.

CPU tensors stop at "must be on a GPU", the last refusal but one of every call.  What lies behind it (the length texts of
alpha / dalpha / dout / out, the state's device) is reached with `gpu(t)`: the same CPU tensor as a subclass whose is_cuda
is True, so that every other check -- dtype, contiguity, the devices being one -- still runs on it.  No call here gets as
far as an allocation or a C entry."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402

INC = ar.toy()
N, M, NNZ, H = INC.N, INC.M, INC.nnz, 3
BF16, I64 = torch.bfloat16, torch.int64

ON_GPU = "%s must be on a GPU (no CPU fallback in this backend)"
HEADS = "heads must be an integer >= 1, got %r"
GROUP = "group / side must be 'hyperedge' or 'vertex', got %r"
DROPOUT = ("dropout must be a real number in [0, 1), got %r (1.0 is refused: the scale 1 / (1 - dropout) of the kept "
           "coefficients would be infinite)")
VARIANT = "%s runs the atomic-free segment kernels: variant must be 'auto' or 'pull', got %r"
NO_BF16 = "%s must be a float32 tensor (%s has no bfloat16 form), got %s"
ELEMENTS = "%s must have %d elements, got %d"
NUM_NODES = "incidence_softmax needs node_score or num_nodes (the number of vertices)"
CSR = "csrptr_t and indices_t must be int32 tensors"
INT32 = "%s must be an int32 tensor"
RNG_DTYPE = "rng_state must be an int64 tensor of 2 elements {key, sid}, got %s"
RNG_LENGTH = "rng_state must have 2 elements {key, sid}, got %d"
TOUCHED = "device touched"


class _OnGpu(torch.Tensor):
    is_cuda = True


def gpu(t):
    return t.as_subclass(_OnGpu)


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


PTR, IND = torch.from_numpy(INC.csrptr), torch.from_numpy(INC.colind)
GPTR, GIND = gpu(PTR), gpu(IND)
RNG = z(2, dtype=I64)


def check(call, exc, text):
    with pytest.raises(exc) as got:
        call()
    assert type(got.value) is exc and str(got.value) == text, (type(got.value), str(got.value))


# ---- ops.incidence_softmax -------------------------------------------------------------------------------------------

def softmax_cases(ops):
    S = ops.incidence_softmax
    fused = ops.Options(variant="fused")
    sv, se, t = z(N), z(M), z(NNZ)
    svh, seh, th = z(N, H), z(M, H), z(NNZ, H)
    me = "incidence_softmax"
    return [
        # the keywords, before any tensor is looked at: dropout, then heads, then num_nodes, then the variant, then group
        ("dropout-1.0", lambda: S(PTR, IND, sv, se, dropout=1.0), ValueError, DROPOUT % 1.0),
        ("dropout-negative", lambda: S(PTR, IND, sv, se, dropout=-0.1), ValueError, DROPOUT % -0.1),
        ("dropout-bool", lambda: S(PTR, IND, sv, se, dropout=True), ValueError, DROPOUT % True),
        ("dropout-string", lambda: S(PTR, IND, sv, se, dropout="0.5"), ValueError, DROPOUT % "0.5"),
        ("dropout-range-when-not-training", lambda: S(PTR, IND, sv, se, dropout=2, training=False), ValueError, DROPOUT % 2),
        ("dropout-over-heads", lambda: S(PTR, IND, sv, se, dropout=1.5, heads=0), ValueError, DROPOUT % 1.5),
        ("heads-0", lambda: S(PTR, IND, sv, se, heads=0), ValueError, HEADS % 0),
        ("heads-float", lambda: S(PTR, IND, sv, se, heads=2.0), ValueError, HEADS % 2.0),
        ("heads-bool", lambda: S(PTR, IND, sv, se, heads=True), ValueError, HEADS % True),
        ("heads-over-num_nodes", lambda: S(PTR, IND, None, se, heads=-1), ValueError, HEADS % -1),
        ("heads-over-variant", lambda: S(PTR, IND, sv, se, heads=0, options=fused), ValueError, HEADS % 0),
        ("num_nodes-missing", lambda: S(PTR, IND, None, se), ValueError, NUM_NODES),
        ("num_nodes-missing-entry", lambda: S(PTR, IND, None, None, incidence_score=t), ValueError, NUM_NODES),
        ("num_nodes-over-variant", lambda: S(PTR, IND, None, se, options=fused, group="edge"), ValueError, NUM_NODES),
        ("variant-fused", lambda: S(PTR, IND, sv, se, options=fused), ValueError, VARIANT % (me, "fused")),
        ("variant-push", lambda: S(PTR, IND, sv, se, options=ops.Options(variant="push_atomic")), ValueError,
         VARIANT % (me, "push_atomic")),
        ("variant-entry", lambda: S(PTR, IND, svh, seh, heads=H, incidence_score=th, options=fused), ValueError,
         VARIANT % (me, "fused")),
        ("variant-over-group", lambda: S(PTR, IND, sv, se, options=fused, group="edge"), ValueError, VARIANT % (me, "fused")),
        ("group", lambda: S(PTR, IND, sv, se, group="edge"), ValueError, GROUP % "edge"),
        ("group-number", lambda: S(PTR, IND, sv, se, group=0), ValueError, GROUP % 0),
        ("group-entry-dropout", lambda: S(PTR, IND, sv, se, group="node", incidence_score=t, dropout=0.5), ValueError,
         GROUP % "node"),
        ("group-over-dtype", lambda: S(PTR, IND, sv.to(BF16), se, group="edge"), ValueError, GROUP % "edge"),
        # dtypes: the floats in the order node, edge, incidence, then the state, then the CSR pair
        ("node-bf16", lambda: S(PTR, IND, sv.to(BF16), se), TypeError, NO_BF16 % ("node_score", me, BF16)),
        ("edge-f64", lambda: S(PTR, IND, sv, se.double()), TypeError, NO_BF16 % ("edge_score", me, torch.float64)),
        ("edge-list", lambda: S(PTR, IND, sv, [0.0] * M), TypeError, NO_BF16 % ("edge_score", me, list)),
        ("entry-bf16", lambda: S(PTR, IND, svh, seh, heads=H, incidence_score=th.to(BF16)), TypeError,
         NO_BF16 % ("incidence_score", me, BF16)),
        ("entry-bf16-alone", lambda: S(PTR, IND, None, None, num_nodes=N, incidence_score=t.to(BF16)), TypeError,
         NO_BF16 % ("incidence_score", me, BF16)),
        ("node-over-edge-dtype", lambda: S(PTR, IND, sv.half(), se.to(BF16)), TypeError,
         NO_BF16 % ("node_score", me, torch.float16)),
        ("dtype-over-length", lambda: S(PTR, IND, sv, se[:-1].to(BF16)), TypeError, NO_BF16 % ("edge_score", me, BF16)),
        ("entry-dtype-over-length", lambda: S(PTR, IND, svh, seh[:-1], heads=H, incidence_score=th.to(BF16)), TypeError,
         NO_BF16 % ("incidence_score", me, BF16)),
        ("float-dtype-over-rng-dtype", lambda: S(PTR, IND, sv, se.to(BF16), dropout=0.5, rng_state=z(2)), TypeError,
         NO_BF16 % ("edge_score", me, BF16)),
        ("rng-f32", lambda: S(PTR, IND, sv, se, dropout=0.5, rng_state=z(2)), TypeError, RNG_DTYPE % torch.float32),
        ("rng-i32-entry", lambda: S(PTR, IND, svh, seh, heads=H, incidence_score=th, dropout=0.5,
                                    rng_state=z(2, dtype=torch.int32)), TypeError, RNG_DTYPE % torch.int32),
        ("rng-tuple", lambda: S(PTR, IND, sv, se, dropout=0.5, rng_state=(1, 2)), TypeError, RNG_DTYPE % tuple),
        ("rng-dtype-over-lengths", lambda: S(PTR, IND, sv, se[:-1], dropout=0.5, rng_state=z(3)), TypeError,
         RNG_DTYPE % torch.float32),
        ("rng-dtype-over-csr", lambda: S(None, IND, sv, se, dropout=0.5, rng_state=z(2)), TypeError, RNG_DTYPE % torch.float32),
        ("csr-none", lambda: S(None, IND, sv, None), TypeError, CSR),
        ("csr-list", lambda: S(PTR, INC.colind.tolist(), sv, se), TypeError, CSR),
        ("csr-over-lengths", lambda: S(PTR, None, sv, se[:-1], incidence_score=t), TypeError, CSR),
        # lengths: node, edge, incidence, then the state
        ("node-length", lambda: S(PTR, IND, sv[:-1], se, num_nodes=N), ValueError, ELEMENTS % ("node_score", N, N - 1)),
        ("node-length-num_nodes", lambda: S(PTR, IND, sv, se, num_nodes=N + 2), ValueError,
         ELEMENTS % ("node_score", N + 2, N)),
        ("node-length-heads", lambda: S(PTR, IND, z(N * H + 1), seh, heads=H), ValueError,
         ELEMENTS % ("node_score", N * H, N * H + 1)),  # N is taken as the element count // heads
        ("edge-length", lambda: S(PTR, IND, sv, z(M + 1)), ValueError, ELEMENTS % ("edge_score", M, M + 1)),
        ("edge-length-heads", lambda: S(PTR, IND, svh, se, heads=H), ValueError, ELEMENTS % ("edge_score", M * H, M)),
        ("entry-length", lambda: S(PTR, IND, sv, se, incidence_score=z(NNZ + 1)), ValueError,
         ELEMENTS % ("incidence_score", NNZ, NNZ + 1)),
        ("entry-length-heads", lambda: S(PTR, IND, svh, seh, heads=H, incidence_score=t), ValueError,
         ELEMENTS % ("incidence_score", NNZ * H, NNZ)),
        ("entry-length-alone-dropout", lambda: S(PTR, IND, None, None, num_nodes=N, incidence_score=z(NNZ - 1), dropout=0.5),
         ValueError, ELEMENTS % ("incidence_score", NNZ, NNZ - 1)),
        ("node-over-edge-length", lambda: S(PTR, IND, sv[:-1], se[:-1], num_nodes=N), ValueError, ELEMENTS % ("node_score", N, N - 1)),
        ("edge-over-entry-length", lambda: S(PTR, IND, sv, se[:-1], incidence_score=t[:-1]), ValueError,
         ELEMENTS % ("edge_score", M, M - 1)),
        ("float-length-over-rng-length", lambda: S(PTR, IND, sv, se[:-1], dropout=0.5, rng_state=z(3, dtype=I64)), ValueError,
         ELEMENTS % ("edge_score", M, M - 1)),
        ("rng-length", lambda: S(PTR, IND, sv, se, dropout=0.5, rng_state=z(3, dtype=I64)), ValueError, RNG_LENGTH % 3),
        ("rng-length-entry", lambda: S(PTR, IND, svh, seh, heads=H, incidence_score=th, dropout=0.25,
                                       rng_state=z(1, dtype=I64)), ValueError, RNG_LENGTH % 1),
        ("rng-length-over-device", lambda: S(PTR.long(), IND, sv, se, dropout=0.5, rng_state=z(2, 2, dtype=I64)), ValueError,
         RNG_LENGTH % 4),
        # the index dtype, then where the tensors live: the CSR pair, the floats, the state
        ("csrptr-int64", lambda: S(PTR.long(), IND, sv, se), TypeError, INT32 % "csrptr_t"),
        ("indices-int64", lambda: S(GPTR, IND.long(), sv, se), TypeError, INT32 % "indices_t"),
        ("not-on-gpu", lambda: S(PTR, IND, sv, se), RuntimeError, ON_GPU % "csrptr_t"),
        ("not-on-gpu-heads", lambda: S(PTR, IND, svh, seh, heads=H, group="vertex"), RuntimeError, ON_GPU % "csrptr_t"),
        ("not-on-gpu-entry", lambda: S(PTR, IND, svh, seh, heads=H, incidence_score=th), RuntimeError, ON_GPU % "csrptr_t"),
        ("not-on-gpu-dropout", lambda: S(PTR, IND, sv, se, dropout=0.5, rng_state=RNG), RuntimeError, ON_GPU % "csrptr_t"),
        ("not-on-gpu-entry-dropout", lambda: S(PTR, IND, None, None, num_nodes=N, incidence_score=t, dropout=0.5,
                                               rng_state=RNG, return_rng_state=True), RuntimeError, ON_GPU % "csrptr_t"),
        ("not-on-gpu-no-scores", lambda: S(PTR, IND, None, None, num_nodes=N), RuntimeError, ON_GPU % "csrptr_t"),
        ("indices-not-on-gpu", lambda: S(GPTR, IND, sv, se), RuntimeError, ON_GPU % "indices_t"),
        ("csr-over-floats-device", lambda: S(PTR, GIND, gpu(sv), se), RuntimeError, ON_GPU % "csrptr_t"),
        ("node-not-on-gpu", lambda: S(GPTR, GIND, sv, gpu(se)), RuntimeError, ON_GPU % "node_score"),
        ("edge-not-on-gpu", lambda: S(GPTR, GIND, gpu(sv), se, incidence_score=t), RuntimeError, ON_GPU % "edge_score"),
        ("entry-not-on-gpu", lambda: S(GPTR, GIND, gpu(sv), gpu(se), incidence_score=t), RuntimeError,
         ON_GPU % "incidence_score"),
        ("node-not-contiguous", lambda: S(GPTR, GIND, gpu(z(N, 2))[:, 0], gpu(se)), RuntimeError, "node_score must be contiguous"),
        ("floats-over-rng-device", lambda: S(GPTR, GIND, gpu(sv), se, dropout=0.5, rng_state=RNG), RuntimeError,
         ON_GPU % "edge_score"),
        ("rng-not-on-gpu", lambda: S(GPTR, GIND, gpu(sv), gpu(se), dropout=0.5, rng_state=RNG), RuntimeError,
         ON_GPU % "rng_state"),
        ("rng-not-on-gpu-entry", lambda: S(GPTR, GIND, None, None, num_nodes=N, incidence_score=gpu(t), dropout=0.5,
                                           rng_state=RNG), RuntimeError, ON_GPU % "rng_state"),
        # the state is looked at only where dropout runs: dropout = 0.0 or training=False get past a state no call would take
        ("rng-ignored-dropout-0", lambda: S(PTR, IND, sv, se, rng_state=z(3)), RuntimeError, ON_GPU % "csrptr_t"),
        ("rng-ignored-not-training", lambda: S(PTR, IND, sv, se, dropout=0.5, training=False, rng_state="no state"),
         RuntimeError, ON_GPU % "csrptr_t"),
        ("rng-ignored-entry", lambda: S(PTR, IND, sv, se, incidence_score=t, dropout=0.5, training=False, rng_state=z(3)),
         RuntimeError, ON_GPU % "csrptr_t"),
        # every check passed: the next thing asked for is the plan
        ("passes-plain", lambda: S(GPTR, GIND, gpu(sv), gpu(se)), AssertionError, TOUCHED),
        ("passes-heads-vertex", lambda: S(GPTR, GIND, gpu(svh), None, heads=H, group="vertex"), AssertionError, TOUCHED),
        ("passes-entry", lambda: S(GPTR, GIND, None, None, num_nodes=N, incidence_score=gpu(th), heads=H), AssertionError,
         TOUCHED),
        ("passes-dropout", lambda: S(GPTR, GIND, gpu(sv), gpu(se), dropout=0.5, rng_state=gpu(RNG)), AssertionError, TOUCHED),
        ("passes-entry-dropout", lambda: S(GPTR, GIND, gpu(sv), None, incidence_score=gpu(t), dropout=0.5, rng_state=gpu(RNG)),
         AssertionError, TOUCHED),
        ("passes-bad-rng-dropout-0", lambda: S(GPTR, GIND, gpu(sv), gpu(se), rng_state=z(3)), AssertionError, TOUCHED),
    ]


# ---- ops.incidence_sum ------------------------------------------------------------------------------------------------

def sum_cases(ops):
    S = ops.incidence_sum
    v, vh = z(NNZ), z(NNZ, H)
    me = "incidence_sum"
    return [
        ("heads-0", lambda: S(PTR, IND, v, heads=0), ValueError, HEADS % 0),
        ("heads-over-side", lambda: S(PTR, IND, v, side="edge", heads=1.0), ValueError, HEADS % 1.0),
        ("side", lambda: S(PTR, IND, v, side="edge"), ValueError, GROUP % "edge"),
        ("side-over-dtype", lambda: S(PTR, IND, v.to(BF16), side=1), ValueError, GROUP % 1),
        ("val-bf16", lambda: S(PTR, IND, v.to(BF16)), TypeError, NO_BF16 % ("val", me, BF16)),
        ("val-list", lambda: S(PTR, IND, [0.0] * NNZ), TypeError, NO_BF16 % ("val", me, list)),
        ("val-dtype-over-length", lambda: S(PTR, IND, v[:-1].double(), side="vertex"), TypeError,
         NO_BF16 % ("val", me, torch.float64)),
        ("csr-none", lambda: S(PTR, None, v), TypeError, CSR),
        ("val-length", lambda: S(PTR, IND, v[:-1]), ValueError, ELEMENTS % ("val", NNZ, NNZ - 1)),
        ("val-length-heads", lambda: S(PTR, IND, v, heads=H, side="vertex"), ValueError, ELEMENTS % ("val", NNZ * H, NNZ)),
        ("val-length-over-index-dtype", lambda: S(PTR.long(), IND, z(NNZ + 1)), ValueError, ELEMENTS % ("val", NNZ, NNZ + 1)),
        ("csrptr-int64", lambda: S(PTR.long(), IND, v), TypeError, INT32 % "csrptr_t"),
        ("not-on-gpu", lambda: S(PTR, IND, v, num_nodes=N), RuntimeError, ON_GPU % "csrptr_t"),
        ("not-on-gpu-heads", lambda: S(PTR, IND, vh, side="vertex", num_nodes=N, heads=H), RuntimeError, ON_GPU % "csrptr_t"),
        ("not-on-gpu-over-val-none", lambda: S(PTR, IND, None), RuntimeError, ON_GPU % "csrptr_t"),
        ("val-not-on-gpu", lambda: S(GPTR, GIND, v), RuntimeError, ON_GPU % "val"),
        ("val-none", lambda: S(GPTR, GIND, None), TypeError, "val must be a float32 tensor"),
        ("passes", lambda: S(GPTR, GIND, gpu(v), num_nodes=N), AssertionError, TOUCHED),
        ("passes-heads", lambda: S(GPTR, GIND, gpu(vh), side="vertex", num_nodes=N, heads=H), AssertionError, TOUCHED),
    ]


@pytest.mark.parametrize("cases", [softmax_cases, sum_cases])
def test_operator_refusals(hg, monkeypatch, cases):
    from hypergef_amd import ops

    def touched(*a, **k):
        raise AssertionError(TOUCHED)

    monkeypatch.setattr(ops, "cached_plan", touched)
    state = torch.random.get_rng_state()
    table = cases(ops)
    assert len({c[0] for c in table}) == len(table)
    for name, call, exc, text in table:
        try:
            check(call, exc, text)
        except BaseException as err:
            raise AssertionError("%s: %s" % (name, err)) from err
    assert torch.equal(torch.random.get_rng_state(), state)  # no refusal costs a draw from torch's generator


# ---- the four Plan methods, on a host-only plan ------------------------------------------------------------------------

FEAT = "%s must be a float32 tensor"
NNZ_ELEMENTS = "%s must have nnz%s = %d elements, got %d"


def plan_cases(plan):
    fwd, bwd = plan.incidence_attention, plan.incidence_attention_backward
    drop, drop_bwd = plan.incidence_attention_dropout, plan.incidence_attention_dropout_backward
    sv, se, t, a = gpu(z(N)), gpu(z(M)), gpu(z(NNZ)), gpu(z(NNZ))
    svh, seh, th, ah = gpu(z(N, H)), gpu(z(M, H)), gpu(z(NNZ, H)), gpu(z(NNZ, H))
    rng = gpu(RNG)
    cases = []
    # what all four decide first, in one order: heads, the group, the CSR pair
    for name, call in (("fwd", lambda **k: fwd(k.pop("ptr", GPTR), k.pop("ind", GIND), sv, se, **k)),
                       ("bwd", lambda **k: bwd(k.pop("ptr", GPTR), k.pop("ind", GIND), a, a, sv, se, **k)),
                       ("drop", lambda **k: drop(k.pop("ptr", GPTR), k.pop("ind", GIND), sv, se, rng_state=rng, **k)),
                       ("drop_bwd", lambda **k: drop_bwd(k.pop("ptr", GPTR), k.pop("ind", GIND), a, a, sv, se, rng_state=rng,
                                                         **k))):
        cases += [
            (name + "-heads-over-group", lambda c=call: c(heads=0, group="edge"), ValueError, HEADS % 0),
            (name + "-heads-bool", lambda c=call: c(heads=True), ValueError, HEADS % True),
            (name + "-group-over-csr", lambda c=call: c(group="edge", ptr=PTR), ValueError, GROUP % "edge"),
            (name + "-group-2", lambda c=call: c(group=2), ValueError, GROUP % 2),
            (name + "-csrptr-none", lambda c=call: c(ptr=None, ind=None), TypeError, INT32 % "csrptr_t"),
            (name + "-csrptr-not-on-gpu", lambda c=call: c(ptr=PTR, ind=IND), RuntimeError, ON_GPU % "csrptr_t"),
            (name + "-indices-int64", lambda c=call: c(ind=gpu(IND.long())), TypeError, INT32 % "indices_t"),
            (name + "-indices-not-on-gpu", lambda c=call: c(ind=IND), RuntimeError, ON_GPU % "indices_t"),
        ]
    cases += [
        # incidence_attention: the scores (node, edge, entry), then out
        ("fwd-node-dtype", lambda: fwd(GPTR, GIND, gpu(z(N).to(BF16)), se), TypeError, FEAT % "node_score"),
        ("fwd-node-not-on-gpu", lambda: fwd(GPTR, GIND, z(N), se), RuntimeError, ON_GPU % "node_score"),
        ("fwd-node-length", lambda: fwd(GPTR, GIND, sv[:-1], se), ValueError, ELEMENTS % ("node_score", N, N - 1)),
        ("fwd-node-length-heads", lambda: fwd(GPTR, GIND, sv, seh, heads=H), ValueError, ELEMENTS % ("node_score", N * H, N)),
        ("fwd-node-over-edge", lambda: fwd(GPTR, GIND, sv[:-1], z(M)), ValueError, ELEMENTS % ("node_score", N, N - 1)),
        ("fwd-edge-length", lambda: fwd(GPTR, GIND, None, se[:-1], group="vertex"), ValueError,
         ELEMENTS % ("edge_score", M, M - 1)),
        ("fwd-entry-length", lambda: fwd(GPTR, GIND, sv, se, entry=t[:-1]), ValueError,
         ELEMENTS % ("incidence_score", NNZ, NNZ - 1)),
        ("fwd-entry-length-heads", lambda: fwd(GPTR, GIND, svh, seh, heads=H, entry=t), ValueError,
         ELEMENTS % ("incidence_score", NNZ * H, NNZ)),
        ("fwd-entry-not-on-gpu", lambda: fwd(GPTR, GIND, None, None, entry=z(NNZ)), RuntimeError, ON_GPU % "incidence_score"),
        ("fwd-scores-over-out", lambda: fwd(GPTR, GIND, sv, se[:-1], out=a[:-1]), ValueError,
         ELEMENTS % ("edge_score", M, M - 1)),
        ("fwd-out-dtype", lambda: fwd(GPTR, GIND, sv, se, out=gpu(z(NNZ).double())), TypeError, FEAT % "out"),
        ("fwd-out-not-on-gpu", lambda: fwd(GPTR, GIND, sv, se, out=z(NNZ)), RuntimeError, ON_GPU % "out"),
        ("fwd-out-length", lambda: fwd(GPTR, GIND, sv, se, out=a[:-1]), ValueError,
         "out must have nnz * heads = %d elements" % NNZ),
        ("fwd-out-length-heads", lambda: fwd(GPTR, GIND, svh, seh, heads=H, out=a), ValueError,
         "out must have nnz * heads = %d elements" % (NNZ * H)),
        ("fwd-out-length-entry", lambda: fwd(GPTR, GIND, None, None, heads=H, entry=th, out=gpu(z(NNZ * H + 1))), ValueError,
         "out must have nnz * heads = %d elements" % (NNZ * H)),
        # incidence_attention_backward: alpha, dalpha, their lengths in that order, then the scores
        ("bwd-alpha-none", lambda: bwd(GPTR, GIND, None, a, sv, se), TypeError, FEAT % "alpha"),
        ("bwd-alpha-not-on-gpu", lambda: bwd(GPTR, GIND, z(NNZ), a, sv, se), RuntimeError, ON_GPU % "alpha"),
        ("bwd-dalpha-dtype", lambda: bwd(GPTR, GIND, a, gpu(z(NNZ).half()), sv, se), TypeError, FEAT % "dalpha"),
        ("bwd-dalpha-not-on-gpu", lambda: bwd(GPTR, GIND, a, z(NNZ), sv, se), RuntimeError, ON_GPU % "dalpha"),
        ("bwd-dalpha-not-contiguous", lambda: bwd(GPTR, GIND, a, gpu(z(NNZ, 2))[:, 0], sv, se), RuntimeError,
         "dalpha must be contiguous"),
        ("bwd-dalpha-device-over-alpha-length", lambda: bwd(GPTR, GIND, a[:-1], z(NNZ), sv, se), RuntimeError, ON_GPU % "dalpha"),
        ("bwd-alpha-length", lambda: bwd(GPTR, GIND, a[:-1], a, sv, se), ValueError, NNZ_ELEMENTS % ("alpha", "", NNZ, NNZ - 1)),
        ("bwd-alpha-length-heads", lambda: bwd(GPTR, GIND, a, ah, svh, seh, heads=H), ValueError,
         NNZ_ELEMENTS % ("alpha", " * heads", NNZ * H, NNZ)),
        ("bwd-alpha-over-dalpha-length", lambda: bwd(GPTR, GIND, a[:-1], a[:-2], sv, se), ValueError,
         NNZ_ELEMENTS % ("alpha", "", NNZ, NNZ - 1)),
        ("bwd-dalpha-length", lambda: bwd(GPTR, GIND, a, gpu(z(NNZ + 1)), sv, se), ValueError,
         NNZ_ELEMENTS % ("dalpha", "", NNZ, NNZ + 1)),
        ("bwd-dalpha-length-heads", lambda: bwd(GPTR, GIND, ah, a, svh, seh, heads=H, group="vertex"), ValueError,
         NNZ_ELEMENTS % ("dalpha", " * heads", NNZ * H, NNZ)),
        ("bwd-dalpha-length-entry", lambda: bwd(GPTR, GIND, ah, a, None, None, heads=H, entry=th), ValueError,
         NNZ_ELEMENTS % ("dalpha", " * heads", NNZ * H, NNZ)),
        ("bwd-dalpha-over-scores", lambda: bwd(GPTR, GIND, a, a[:-1], sv[:-1], se), ValueError,
         NNZ_ELEMENTS % ("dalpha", "", NNZ, NNZ - 1)),
        ("bwd-node-length", lambda: bwd(GPTR, GIND, a, a, sv[:-1], se), ValueError, ELEMENTS % ("node_score", N, N - 1)),
        ("bwd-entry-length", lambda: bwd(GPTR, GIND, ah, ah, svh, seh, heads=H, entry=t), ValueError,
         ELEMENTS % ("incidence_score", NNZ * H, NNZ)),
        ("bwd-edge-not-on-gpu", lambda: bwd(GPTR, GIND, a, a, sv, z(M)), RuntimeError, ON_GPU % "edge_score"),
        # incidence_attention_dropout: the scores, then the state: dtype, length, device
        ("drop-scores-over-rng", lambda: drop(GPTR, GIND, sv, se[:-1], rng_state=z(3)), ValueError,
         ELEMENTS % ("edge_score", M, M - 1)),
        ("drop-entry-length", lambda: drop(GPTR, GIND, sv, se, rng_state=rng, entry=gpu(z(NNZ + 1))), ValueError,
         ELEMENTS % ("incidence_score", NNZ, NNZ + 1)),
        ("drop-rng-none", lambda: drop(GPTR, GIND, sv, se), TypeError, RNG_DTYPE % type(None)),
        ("drop-rng-dtype-over-length", lambda: drop(GPTR, GIND, sv, se, rng_state=z(3)), TypeError, RNG_DTYPE % torch.float32),
        ("drop-rng-length", lambda: drop(GPTR, GIND, svh, seh, heads=H, rng_state=z(3, dtype=I64)), ValueError, RNG_LENGTH % 3),
        ("drop-rng-length-over-device", lambda: drop(GPTR, GIND, sv, se, rng_state=z(1, dtype=I64), entry=t), ValueError,
         RNG_LENGTH % 1),
        ("drop-rng-not-on-gpu", lambda: drop(GPTR, GIND, sv, se, rng_state=RNG), RuntimeError, ON_GPU % "rng_state"),
        ("drop-rng-not-contiguous", lambda: drop(GPTR, GIND, sv, se, rng_state=gpu(z(2, 2, dtype=I64))[:, 0]), RuntimeError,
         "rng_state must be contiguous"),
        # incidence_attention_dropout_backward: alpha, dout -- under that name --, the scores, the state
        ("drop_bwd-alpha-none", lambda: drop_bwd(GPTR, GIND, None, a, sv, se, rng_state=rng), TypeError, FEAT % "alpha"),
        ("drop_bwd-dout-dtype", lambda: drop_bwd(GPTR, GIND, a, gpu(z(NNZ).double()), sv, se, rng_state=rng), TypeError,
         FEAT % "dout"),
        ("drop_bwd-dout-not-on-gpu", lambda: drop_bwd(GPTR, GIND, a, z(NNZ), sv, se, rng_state=rng), RuntimeError, ON_GPU % "dout"),
        ("drop_bwd-alpha-length", lambda: drop_bwd(GPTR, GIND, a[:-1], a, sv, se, rng_state=rng), ValueError,
         NNZ_ELEMENTS % ("alpha", "", NNZ, NNZ - 1)),
        ("drop_bwd-alpha-over-dout-length", lambda: drop_bwd(GPTR, GIND, a, a, svh, seh, heads=H, rng_state=rng), ValueError,
         NNZ_ELEMENTS % ("alpha", " * heads", NNZ * H, NNZ)),
        ("drop_bwd-dout-length", lambda: drop_bwd(GPTR, GIND, a, a[:-1], sv, se, rng_state=rng), ValueError,
         NNZ_ELEMENTS % ("dout", "", NNZ, NNZ - 1)),
        ("drop_bwd-dout-length-heads", lambda: drop_bwd(GPTR, GIND, ah, a, svh, seh, heads=H, rng_state=rng), ValueError,
         NNZ_ELEMENTS % ("dout", " * heads", NNZ * H, NNZ)),
        ("drop_bwd-dout-length-entry", lambda: drop_bwd(GPTR, GIND, ah, gpu(z(NNZ * H - 1)), svh, seh, heads=H, rng_state=rng,
                                                        entry=th, group="vertex"), ValueError,
         NNZ_ELEMENTS % ("dout", " * heads", NNZ * H, NNZ * H - 1)),
        ("drop_bwd-dout-over-scores-over-rng", lambda: drop_bwd(GPTR, GIND, a, a[:-1], sv[:-1], se, rng_state=z(3)), ValueError,
         NNZ_ELEMENTS % ("dout", "", NNZ, NNZ - 1)),
        ("drop_bwd-scores-over-rng", lambda: drop_bwd(GPTR, GIND, a, a, sv[:-1], se, rng_state=z(3)), ValueError,
         ELEMENTS % ("node_score", N, N - 1)),
        ("drop_bwd-rng-none", lambda: drop_bwd(GPTR, GIND, a, a, sv, se), TypeError, RNG_DTYPE % type(None)),
        ("drop_bwd-rng-dtype-over-length", lambda: drop_bwd(GPTR, GIND, a, a, sv, se, rng_state=z(3, dtype=torch.int32)),
         TypeError, RNG_DTYPE % torch.int32),
        ("drop_bwd-rng-length", lambda: drop_bwd(GPTR, GIND, a, a, sv, se, rng_state=z(4, dtype=I64), entry=t), ValueError,
         RNG_LENGTH % 4),
        ("drop_bwd-rng-not-on-gpu", lambda: drop_bwd(GPTR, GIND, ah, ah, svh, seh, heads=H, rng_state=RNG), RuntimeError,
         ON_GPU % "rng_state"),
    ]
    return cases


def test_plan_method_refusals(hg):
    from hypergef_amd.plan import Plan, make_opts
    plan = Plan.from_host(INC.N, INC.M, INC.csrptr, INC.colind, opts=make_opts(host_only=True))
    table = plan_cases(plan)
    assert len({c[0] for c in table}) == len(table)
    for name, call, exc, text in table:
        try:
            check(call, exc, text)
        except BaseException as err:
            raise AssertionError("%s: %s" % (name, err)) from err
