"""Dot-product attention over a kNN neighbour table against the same result composed from existing operators (GPU only; no GPU
is an error).  k = 10; cells N x F at H = 1 and 4; device ms between events (a) and wall ms between synchronisations (b), warm,
medians of three rounds, candidates in turn, one process.

(a) ops.knn_dot_attention_aggr, forward and forward + backward (gradients of X and query), against
      composed: knn_graph.table_dot(heads) * scale -> ops.knn_softmax(entry_score=) -> ops.knn_aggr(weight_grad=True); table_dot
                has no gradient, so the backward stops at the logits (the composed path is favoured);
      torch:    X[idx], einsum, softmax, index_add_ (forward and autograd's backward).
(b) one training step of DynamicHypergraphConv(F -> H x F / H, k, device_graph=True, attention='hyperedge', score='dot'): eager,
    replayed from a hipGraph, and HyperGraph.from_knn + HypergraphAttnConv(score='dot') rebuilt every forward.

    python tools/table_dot_attention_probe.py [--steps 20] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

import torch  # noqa: E402

from table_aggr_probe import device_ms, rounds, wall_ms  # noqa: E402

CELLS = ((2708, 32), (12311, 32), (50000, 32), (50000, 128))
HEADS = (1, 4)
K = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("table_dot_attention_probe: no GPU (this probe measures the device; there is no CPU fallback)")
    import hypergef_amd as hg
    from hypergef_amd import knn_graph as kg
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "k": K, "steps": args.steps, "operator": [], "layer": []}
    for N, F in CELLS:
        g = kg.KnnHypergraph.build(torch.randn(N, 32, device=dev, generator=gen), K)
        idx, tp, long_idx = g.idx, (g.ptr_v, g.pos_v), g.idx.long()
        X = torch.randn(N, F, device=dev, generator=gen).requires_grad_(True)
        Q = torch.randn(N, F, device=dev, generator=gen).requires_grad_(True)
        G = torch.randn(N, F, device=dev, generator=gen)
        for H in HEADS:
            Ch, scale = F // H, (F // H) ** -0.5

            def fused():
                return hg.ops.knn_dot_attention_aggr(idx, X, Q, 0.2, None, g.degE, g.degV, transpose=tp, heads=H)

            def composed():
                t = composed.leaf = (kg.table_dot(idx, X.detach(), Q.detach(), heads=H).view(N, K, H) * scale).requires_grad_(True)
                alpha = hg.ops.knn_softmax(idx, None, None, "hyperedge", 0.2, entry_score=t if H > 1 else t.view(N, K),
                                           transpose=tp, num_nodes=N, heads=H)
                return hg.ops.knn_aggr(idx, X, alpha, g.degE, g.degV, transpose=tp, weight_grad=True)

            def eager():
                Xj = X.view(N, H, Ch)[long_idx]
                t = torch.einsum("ihc,ishc->ish", Q.view(N, H, Ch), Xj) * scale
                alpha = torch.softmax(torch.nn.functional.leaky_relu(t, 0.2), 1)[..., None]
                E = g.degE.view(N, 1, 1) * (alpha * Xj).sum(1)
                Y = torch.zeros(N, H, Ch, device=dev).index_add_(0, long_idx.reshape(-1), (alpha * E[:, None]).reshape(N * K, H, Ch))
                return (g.degV.view(N, 1, 1) * Y).view(N, F)

            forms = {}
            for name, f in (("fused", fused), ("composed", composed), ("torch", eager)):
                def fwd(f=f):
                    with torch.no_grad():
                        f()

                def both(f=f):
                    y = f()
                    torch.autograd.grad(y, [X, Q] + ([f.leaf] if hasattr(f, "leaf") else []), G, allow_unused=True)
                forms[name + "_fwd"], forms[name + "_fwd_bwd"] = fwd, both
            with torch.no_grad():
                err = float((fused() - eager()).abs().max())
            ms, runs = rounds(forms, 10 * args.steps, device_ms)
            r = {"N": N, "F": F, "H": H, "device_ms": ms, "runs": runs, "max_abs_diff_to_torch": err,
                 "max_in_degree": int((g.ptr_v[1:] - g.ptr_v[:-1]).max())}
            res["operator"].append(r)
            print(json.dumps(r), flush=True)
    for N, F in CELLS:
        P = torch.randn(N, F, device=dev, generator=gen)
        for H in HEADS:
            torch.manual_seed(1)
            layer = hg.DynamicHypergraphConv(F, F // H, k=K, device_graph=True, attention="hyperedge", heads=H, score="dot").to(dev)
            Gy = torch.ones(N, F, device=dev)

            def step():
                for p in layer.parameters():
                    p.grad = None
                layer(P).backward(Gy)

            def planned():
                ref = hg.HypergraphAttnConv(hg.HyperGraph.from_knn(P, K, dev), F, F // H, group="hyperedge", heads=H, score="dot").to(dev)
                ref(P).backward(Gy)

            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            forms = {"eager": step, "captured": graph.replay, "planned_rebuilt": planned}
            ms, runs = rounds(forms, args.steps, wall_ms)
            r = {"N": N, "F": F, "H": H, "step_wall_ms": ms, "runs": runs}
            res["layer"].append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
