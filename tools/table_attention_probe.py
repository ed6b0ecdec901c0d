"""Fused attention aggregation over a kNN neighbour table against the two calls it replaces (GPU only; no GPU is an error).

Layer: one training step (forward + backward, eager, wall ms between synchronisations, medians of three rounds, candidates in
turn) of DynamicHypergraphConv(F -> H x F / H, k, device_graph=True, attention=group, heads=H) with fused_attention False and
True on the same build and input, and torch.cuda.max_memory_allocated over one step of each.
Hop 1: device ms between events of knn_graph.table_attention_gather (the hyperedge gather with the coefficients formed inside)
at H heads of Ch columns, and of knn_graph.table_gather on a stored alpha.  Whether the wave's LDS slab or the per-lane form
runs is the library's rule (csrc/hg_table_attention.hip, kSlabMinCh); a build with -DHG_TABLE_SLAB_MIN_CH=1000000 has no slab,
and HG_AGGR_LIB=that build runs this probe on it: two runs, one table.

    python tools/table_attention_probe.py [--steps 20] [--n 50000] [--k 10] [--out profiles/NAME.json]
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

LAYERS = ((128, 4), (256, 4))      # (F, H): the layer maps F -> H x F / H
HOPS = ((4, 16), (4, 64), (8, 8))  # (H, Ch) of the hop-1 gather


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("table_attention_probe: no GPU (this probe measures the device; there is no CPU fallback)")
    import hypergef_amd as hg
    from hypergef_amd import _lib, knn_graph as kg
    dev = torch.device("cuda:0")
    N, K = args.n, args.k
    gen = torch.Generator(device=dev).manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "lib": _lib.LIB_PATH, "N": N, "k": K, "steps": args.steps, "layer": [], "hop1": []}
    for F, H in LAYERS:
        X = torch.randn(N, F, device=dev, generator=gen)
        G = torch.ones(N, F, device=dev)
        for group in ("hyperedge", "vertex"):
            forms, peak = {}, {}
            for name, flag in (("unfused", False), ("fused", True)):
                torch.manual_seed(1)
                layer = hg.DynamicHypergraphConv(F, F // H, k=K, device_graph=True, attention=group, heads=H, fused_attention=flag).to(dev)

                def step(layer=layer):
                    for p in layer.parameters():
                        p.grad = None
                    layer(X).backward(G)
                forms[name] = step
                step()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                step()
                torch.cuda.synchronize()
                peak[name] = torch.cuda.max_memory_allocated()
            ms, runs = rounds(forms, args.steps, wall_ms)
            r = {"F": F, "H": H, "group": group, "step_wall_ms": ms, "runs": runs, "peak_bytes": peak}
            res["layer"].append(r)
            print(json.dumps(r), flush=True)
    P = torch.randn(N, 32, device=dev, generator=gen)
    g = kg.KnnHypergraph.build(P, K)
    for H, Ch in HOPS:
        X = torch.randn(N, H * Ch, device=dev, generator=gen)
        sv, se = torch.randn(N, H, device=dev, generator=gen), torch.randn(N, H, device=dev, generator=gen)
        for group in ("hyperedge", "vertex"):
            with torch.no_grad():
                m, inv = kg.table_attention_stats(g.idx, N, group, sv, se, 0.2, g.ptr_v, g.pos_v, H)
                alpha = kg.table_softmax(g.idx, N, group, sv, se, None, 0.2, g.ptr_v, g.pos_v, H)
                forms = {"attention_gather": lambda: kg.table_attention_gather(g.idx, None, None, N, X, group, sv, se, 0.2, m, inv,
                                                                                 None, g.degE, H),
                         "gather_on_alpha": lambda: kg.table_gather(g.idx, X, alpha, None, g.degE, heads=H),
                         "softmax": lambda: kg.table_softmax(g.idx, N, group, sv, se, None, 0.2, g.ptr_v, g.pos_v, H),
                         "stats": lambda: kg.table_attention_stats(g.idx, N, group, sv, se, 0.2, g.ptr_v, g.pos_v, H)}
                same = torch.equal(forms["attention_gather"](), forms["gather_on_alpha"]())
                ms, runs = rounds(forms, 10 * args.steps, device_ms)
            r = {"H": H, "Ch": Ch, "group": group, "device_ms": ms, "runs": runs, "same_bits": same}
            res["hop1"].append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
