"""Attention dropout over a neighbour table on the GPU.  The contract is bits: with keep the library's host statement of the mask,
alpha_drop = where(keep, fl(alpha * scale), +0) and the gradients are the no-dropout node's on where(keep, fl(dout * scale), +0).
The values: test_table_softmax_gpu._ref in float64, head by head, fed the masked gradient, at that file's bound
(2 c + (L + D + 8) U) max(mass, TINY) plus one U: every term of mass has |dalpha| as a factor, and fl(dout * scale) is one rounding.
Tables: that file's [77, k] (15 % out of range), k = 1, 9, 64, and hub_table(1), vertex rows either side of HG_TABLE_SEQ_MAX;
H = 1, 3, 4: scalar slab, odd, 16-byte slab.  STATE's mask keeps 49-53 % of each at p = 0.5."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dropout_ref as dr  # noqa: E402
from test_table_softmax_gpu import TINY, U, _bits, _dev, _ref, _table  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STATE = (0x0123456789ABCDEF, -0x0123456700000003)  # {key, sid} as int64
NAMES = ("d node_score", "d edge_score", "d entry_score")


def _case(hg, which, H):
    idx, n = _table(which)
    tail = (H,) if H > 1 else ()
    rng = np.random.default_rng(100 + H)
    host = [rng.standard_normal(s + tail).astype(np.float32) for s in ((n,), idx.shape[:1], idx.shape, idx.shape)]
    valid = np.broadcast_to(((idx >= 0) & (idx < n)).reshape(idx.shape + (1,) * len(tail)), idx.shape + tail)
    didx = _dev(idx)
    tp = hg.ops.knn_transpose(didx, n)

    def softmax(group, scores, **kw):
        return hg.ops.knn_softmax(didx, scores[0], scores[1], group, 0.2, scores[2], transpose=tp, num_nodes=n, heads=H, **kw)
    return idx, n, host, [_dev(a) for a in host], valid, torch.tensor(STATE, dtype=torch.int64, device=DEV), softmax


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("which,H", [(w, H) for w in (1, 9, 64, "hub") for H in (1, 3, 4)])
def test_bits_and_float64(hg, which, H, p):
    idx, n, (sv, se, en, dout), dev, valid, state, softmax = _case(hg, which, H)
    keep = dr.keep_of_state(state, p, idx.size, H).reshape(valid.shape)
    assert (0.25 <= keep.mean() <= 0.75) if p == 0.5 else (keep.any() and not keep.all())
    dalpha = np.where(keep, dout * dr.scale(p), np.float32(0))
    dalpha64 = np.where(keep, dout.astype(np.float64) * np.float64(dr.scale(p)), 0.0)
    dropped = []
    for group in ("hyperedge", "vertex"):
        ins = [t.clone().requires_grad_(True) for t in dev[:3]]
        out, used = softmax(group, ins, dropout=p, rng_state=state, return_rng_state=True)
        alpha = softmax(group, ins)
        got, want = out.detach().cpu().numpy(), np.where(keep, alpha.detach().cpu().numpy() * dr.scale(p), np.float32(0))
        assert used is state and np.array_equal(got.view(np.int32), want.view(np.int32)), group
        assert not got.view(np.int32)[~valid].any(), "an out-of-range position is not +0.0"
        dropped.append((got == 0) & valid)  # a candidate's alpha is never 0 at these scores
        grads = torch.autograd.grad(out, ins, dev[3])
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(grads, torch.autograd.grad(alpha, ins, _dev(dalpha)))), group
        for h in range(H):
            col = (lambda a: a[..., h]) if H > 1 else (lambda a: a)
            r = _ref(idx, n, group, col(sv), col(se), col(en), 0.2, col(dalpha64))
            for name, a, ref, mass, D in zip(NAMES, grads, r["grads"], r["mass"], r["D"]):
                err = np.abs(col(a.cpu().numpy()) - ref)
                bound = (2 * r["c"] + (r["L"] + D + 8) * U + U) * np.maximum(mass, TINY)
                print("%s %s H=%d h=%d p=%g %s: worst error / bound = %.3g" % (group, which, H, h, p, name, (err / bound).max()))
                assert (err <= bound).all(), (group, h, name, float((err / bound).max()))
    assert np.array_equal(dropped[0], dropped[1]) and np.array_equal(dropped[0], ~keep & valid), "the groups' masks differ"


def test_neutral_cases(hg):
    _, _, _, dev, _, state, softmax = _case(hg, 9, 3)
    plain = softmax("vertex", dev)
    before = torch.cuda.get_rng_state()
    for kw in (dict(dropout=0.0), dict(dropout=0.0, rng_state=state), dict(dropout=0.5, training=False, rng_state=state)):
        got, used = softmax("vertex", dev, return_rng_state=True, **kw)
        assert used is None and torch.equal(_bits(got), _bits(plain)), kw
    assert torch.equal(torch.cuda.get_rng_state(), before), "a call without dropout drew from torch's generator"
    with pytest.raises(RuntimeError, match="rng_state must be on a GPU"):
        softmax("vertex", dev, dropout=0.5, rng_state=state.cpu())


def test_layer_and_capture(hg):
    torch.manual_seed(26)
    X, G = torch.randn(60, 8, device=DEV), torch.randn(60, 16, device=DEV)
    kw = dict(k=5, device_graph=True, attention="hyperedge", heads=2)
    layer = hg.DynamicHypergraphConv(8, 8, dropout=0.5, **kw).to(DEV)
    plain = hg.DynamicHypergraphConv(8, 8, **kw).to(DEV)
    plain.load_state_dict(layer.state_dict())
    with torch.no_grad():
        assert torch.equal(_bits(layer.eval()(X)), _bits(plain.eval()(X))), "eval() is not the layer without dropout"
    layer.train()
    x = X.clone().requires_grad_(True)

    def step():
        for t in (x, *layer.parameters()):
            t.grad = None
        y = layer(x)
        y.backward(G)
        return y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = step()
    graph.replay()
    first = (y.detach().clone(), x.grad.clone())
    assert all(torch.isfinite(t).all() for t in first)
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(first[0], y) and not torch.equal(first[1], x.grad), "two replays drew the same mask"
