"""One multi-head call chain against the per-head loop and against the single-head call of the same width (GPU only; no GPU
is an error).

The chain is the attention layer's sparse part with gradients: alpha = incidence_softmax(sv, se), Y = incidence_aggr(Z, alpha,
alpha), then backward for sv, se and Z (softmax backward, the swapped aggregation, two incidence_dot calls).  Three forms:
  * heads: one call of each operator with heads=H on Z [N, H C], sv [N, H], se [M, H];
  * loop:  the only formulation without heads -- per head h the slice copies Z[:, hC:(h+1)C].contiguous(), sv[:, h], se[:, h],
    the single-head chain at width C, and the concatenation of the H results;
  * single: the single-head chain at the same F = H C with one [nnz] weight array: the same feature bytes and 1 / H of the
    weight bytes -- what the extra weights cost.
Per cell the outputs and gradients of heads and loop are compared first (they must agree: column h has the bits of the
single-head call, so any difference is a bug), then forward + backward of each form is timed in three alternating runs.

The condition: on every cell the heads form beats the loop by more than the runs' own spread, i.e. the slowest heads run is
faster than the fastest loop run.

    python tools/heads_probe.py [--steps 20] [--cells cora8x8,...] [--out profiles/r08_heads]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

CELLS = [  # (name, shape, replicas, H, C)
    ("cora8x8", "cora", 1024, 8, 8),
    ("cora4x16", "cora", 1024, 4, 16),
    ("pubmed8x16", "pubmed", 64, 8, 16),
    ("powerlaw8x8", "powerlaw", 1, 8, 8),
]
SLOPE = 0.2


def timed(fn, steps, warmup=2):
    import bench
    for _ in range(warmup):
        fn()
    wall, _ = bench.timed_steps(fn, steps, torch.cuda.synchronize, lambda: None)
    return wall / steps * 1e3


def run_cell(name, shape, replicas, H, C, args, dev):
    import bench
    import hypergef_amd as hg
    from hypergef_amd import ops
    _, inc = bench.make_workload(shape, replicas)
    N, M, nnz, F = inc.N, inc.M, inc.nnz, H * C
    hyperg = hg.HyperGraph.from_incidence(inc, dev, ngs=1 << 30)
    ptr, ind, degE, degV = hyperg.H_T_csrptr, hyperg.H_T_colind, hyperg.degE, hyperg.degV
    g = torch.Generator(device=dev).manual_seed(0)
    Z = torch.randn(N, F, device=dev, generator=g).requires_grad_(True)
    sv = torch.randn(N, H, device=dev, generator=g).requires_grad_(True)
    se = torch.randn(M, H, device=dev, generator=g).requires_grad_(True)
    dY = torch.randn(N, F, device=dev, generator=g)
    leaves = (Z, sv, se)

    def chain(z, a, b, heads):
        alpha = ops.incidence_softmax(ptr, ind, a, b, negative_slope=SLOPE, num_nodes=N, heads=heads)
        return ops.incidence_aggr(ptr, ind, z, alpha, alpha, degE, degV, None, heads=heads)

    def heads_form():
        return torch.autograd.grad(chain(Z, sv, se, H), leaves, dY)

    def loop_form():
        outs = [chain(Z[:, h * C:(h + 1) * C].contiguous(), sv[:, h].contiguous(), se[:, h].contiguous(), 1) for h in range(H)]
        return torch.autograd.grad(torch.cat(outs, 1), leaves, dY)

    def single_form():
        return torch.autograd.grad(chain(Z, sv[:, 0].contiguous(), se[:, 0].contiguous(), 1), leaves, dY)

    with torch.no_grad():
        y_heads = chain(Z, sv, se, H)
        y_loop = torch.cat([chain(Z[:, h * C:(h + 1) * C].contiguous(), sv[:, h].contiguous(), se[:, h].contiguous(), 1)
                            for h in range(H)], 1)
    diff = {"Y": float((y_heads - y_loop).abs().max())}
    for nm, a, b in zip(("dZ", "dsv", "dse"), heads_form(), loop_form()):
        diff[nm] = float((a - b).abs().max() / b.abs().max())
    del y_heads, y_loop
    runs = {"heads": [], "loop": [], "single": []}
    for _ in range(3):  # alternate: a drift of the box's clocks lands on every form
        runs["heads"].append(timed(heads_form, args.steps))
        runs["loop"].append(timed(loop_form, max(3, args.steps // 2)))
        runs["single"].append(timed(single_form, args.steps))
    med = {k: sorted(v)[1] for k, v in runs.items()}
    # bytes the weights add to the single-head call: (H - 1) more floats per incidence in each hop, forward and backward,
    # beside two hops of F-wide rows per incidence (the gathers; DESIGN 3.8 counts the same rows)
    extra_share = (H - 1) * 4.0 / (F * 4.0 + 4.0)
    r = {"cell": name, "workload": "%s x%d" % (shape, replicas), "H": H, "C": C, "N": N, "M": M, "nnz": nnz,
         "max_diff_heads_vs_loop": diff, "runs_ms": {k: [round(x, 4) for x in v] for k, v in runs.items()},
         "median_ms": {k: round(v, 4) for k, v in med.items()},
         "loop_over_heads": round(med["loop"] / med["heads"], 2), "heads_over_single": round(med["heads"] / med["single"], 3),
         "extra_weight_bytes_share": round(extra_share, 3),
         "ok": max(runs["heads"]) < min(runs["loop"])}
    return r


def write(stem, res, steps):
    with open(stem + ".json", "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "steps": steps, "cells": res}, f, indent=1)
    with open(stem + ".md", "w") as f:
        f.write("# Multi-head incidence path (tools/heads_probe.py, %d steps per timing, three alternating runs)\n\n" % steps)
        f.write("Forward + backward of softmax -> incidence_aggr with gradients for Z, sv, se; medians, all three runs in the "
                ".json.\n\n| cell | H x C | heads ms (runs) | per-head loop ms (runs) | loop / heads | single-head same F ms | "
                "heads / single | extra weight bytes | condition |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in res:
            f.write("| %s | %d x %d | %.3f (%s) | %.3f (%s) | %.2fx | %.3f | %.3f | +%.1f %% | %s |\n" % (
                r["workload"], r["H"], r["C"], r["median_ms"]["heads"], ", ".join("%.3f" % x for x in r["runs_ms"]["heads"]),
                r["median_ms"]["loop"], ", ".join("%.3f" % x for x in r["runs_ms"]["loop"]), r["loop_over_heads"],
                r["median_ms"]["single"], r["heads_over_single"], 100 * r["extra_weight_bytes_share"],
                "met" if r["ok"] else "NOT met"))
        f.write("\nWeight access of the per-head gather instances: direct reads (4 H contiguous bytes per entry beside the row "
                "they scale).  Staging panel_nnz x H floats in LDS was not built and not measured: at H = 16 it is 64 KiB per "
                "workgroup, two workgroups per CU.  The heads / single column is what the direct reads cost beside the same "
                "rows with one weight per entry.\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--cells", default="all")
    p.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("heads_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    want = None if args.cells == "all" else set(args.cells.split(","))
    res = []
    for cell in CELLS:
        if want is not None and cell[0] not in want:
            continue
        r = run_cell(*cell, args, dev)
        res.append(r)
        print("%-12s H %d C %2d  heads %.3f ms  loop %.3f ms (%.2fx)  single-head F=%d %.3f ms (heads / single %.3f, extra weight "
              "bytes +%.1f %%)  max diff vs loop %s  %s" % (
                  r["cell"], r["H"], r["C"], r["median_ms"]["heads"], r["median_ms"]["loop"], r["loop_over_heads"],
                  r["H"] * r["C"], r["median_ms"]["single"], r["heads_over_single"], 100 * r["extra_weight_bytes_share"],
                  r["max_diff_heads_vs_loop"], "ok" if r["ok"] else "LOSES"), flush=True)
        if args.out:  # after every cell: a run cut short keeps what it measured
            write(args.out, res, args.steps)
        torch.cuda.empty_cache()
    ok = all(r["ok"] for r in res)
    print("condition (heads beats the per-head loop beyond the runs' spread on every cell): %s" % ("met" if ok else "NOT met"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
