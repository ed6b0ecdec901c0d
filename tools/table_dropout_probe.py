"""Attention dropout over a kNN neighbour table: the fused form against softmax + torch dropout (GPU only; no GPU is an error).

At the dynamic layer's shape -- N = 4096 rows of F = 32, k = 16, H = 4, the table of ops.knn(randn [N, F], k) -- device ms
between events per forward + backward (all three score gradients) over 10 * steps calls, warm, medians of three rounds, the
candidates in turn, both groups:
    fused  ops.knn_softmax(..., heads=H, dropout=0.5): hg_table_softmax_dropout_heads_f32 and its backward
    parts  torch.nn.functional.dropout(ops.knn_softmax(..., heads=H), 0.5): what the library offered before
    plain  ops.knn_softmax(..., heads=H) with no dropout at all, for scale

    python tools/table_dropout_probe.py [--steps 20] [--rows 4096] [--k 16] [--heads 4] [--out profiles/r26_table_dropout]
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
import torch.nn.functional as F_  # noqa: E402

from table_aggr_probe import device_ms, rounds  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("table_dropout_probe: no GPU (this probe measures the device; there is no CPU fallback)")
    import hypergef_amd as hg
    from hypergef_amd import knn_graph as kg
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    N, K, H = args.rows, args.k, args.heads
    g = kg.KnnHypergraph.build(torch.randn(N, 32, device=dev), K)
    scores = [torch.randn(s, device=dev, requires_grad=True) for s in ((N, H), (N, H), (N, K, H))]
    G = torch.randn(N, K, H, device=dev)
    forms = {}
    for group in ("hyperedge", "vertex"):
        def alpha(group=group, **kw):
            return hg.ops.knn_softmax(g.idx, scores[0], scores[1], group, 0.2, scores[2], transpose=(g.ptr_v, g.pos_v), heads=H, **kw)
        makers = {"fused": lambda alpha=alpha: alpha(dropout=0.5), "parts": lambda alpha=alpha: F_.dropout(alpha(), 0.5),
                  "plain": alpha}
        for name, make in makers.items():
            forms["%s_%s" % (name, group)] = lambda make=make: torch.autograd.grad(make(), scores, G)
    ms, runs = rounds(forms, 10 * args.steps, device_ms)
    res = {"device": torch.cuda.get_device_name(0), "rows": N, "k": K, "heads": H, "steps": args.steps, "device_ms": ms,
           "device_ms_runs": runs,
           "fused_over_parts": {grp: round(ms["fused_" + grp] / ms["parts_" + grp], 3) for grp in ("hyperedge", "vertex")}}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out + ".json", "w") as f:
            json.dump(res, f, indent=1)
        with open(args.out + ".md", "w") as f:
            f.write("# Attention dropout over a kNN neighbour table (tools/table_dropout_probe.py, %s)\n\n" % res["device"])
            f.write("N = %d, k = %d, H = %d, p = 0.5; device ms between events per forward + backward (three score gradients), warm, "
                    "medians of 3 rounds.  `fused` = ops.knn_softmax(dropout=0.5), `parts` = ops.knn_softmax + "
                    "torch.nn.functional.dropout, `plain` = ops.knn_softmax without dropout.\n\n"
                    "| group | fused | parts | plain | fused / parts |\n|---|---|---|---|---|\n" % (N, K, H))
            for grp in ("hyperedge", "vertex"):
                f.write("| %s | %.4f | %.4f | %.4f | %.3f |\n" % (grp, ms["fused_" + grp], ms["parts_" + grp], ms["plain_" + grp],
                                                                 res["fused_over_parts"][grp]))


if __name__ == "__main__":
    main()
