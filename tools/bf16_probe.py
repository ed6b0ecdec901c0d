"""bf16 against fp32 on the target cells (GPU only; no GPU is an error, there is no fallback).

For each workload -- the bench headline (cora x1024, F = 32), the other five target cells, power-law 1M/4M at F = 64 and
the weighted headline -- one process times the fp32 call and the bf16 call (hg_aggr_fused_bf16) alternately, in rounds
of `--steps` back-to-back calls between two device events, and reports per dtype the median ms per step, the ratio
bf16 / fp32, and the bf16 fraction of the 8 TB/s roofline on bf16 algorithmic bytes (bench.py's b_alg with X and Y at
two bytes per element).  The fp32 input is the bf16 input widened, so the timed outputs must satisfy the invariant of
include/hg_aggr.h: Y_bf16 == round_bf16(Y_fp32) bit for bit -- checked on the outputs of the last timed round.

At bf16, X alone fits the 256 MiB Infinity Cache on several cells (flagged `x<IC`); a fraction above what HBM alone
allows is possible there.  X + Y is at least 355 MB on every cell.

    python tools/bf16_probe.py [--steps 20] [--rounds 7] [--cells headline,pubmed64...] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0
IC_BYTES = 256 << 20
# (name, shape, replicas, F, weighted): bench.py's replica counts
CELLS = [
    ("headline", "cora", 1024, 32, False),
    ("citeseer1024", "citeseer", 1024, 32, False),
    ("pubmed256", "pubmed", 256, 32, False),
    ("cora256_F128", "cora", 256, 128, False),
    ("citeseer256_F128", "citeseer", 256, 128, False),
    ("pubmed64_F128", "pubmed", 64, 128, False),
    ("powerlaw_F64", "powerlaw", 1, 64, False),
    ("headline_weighted", "cora", 1024, 32, True),
]


def b_alg(N, M, nnz, F, n_w, has_degV, feat_bytes):
    """bench.py:b_alg with X and Y at feat_bytes per element (indices, pointers and scales stay 4 bytes)."""
    return feat_bytes * 2 * N * F + 4 * (2 * nnz + (M + 1) + (N + 1) + n_w * M + (N if has_degV else 0))


def run_cell(name, shape, replicas, F, weighted, steps, rounds, warmup, dev):
    import bench
    import hypergef_amd as hg
    from hypergef_amd import plan as planmod
    base, inc = bench.make_workload(shape, replicas)
    ptr = torch.from_numpy(inc.csrptr).to(dev)
    ind = torch.from_numpy(inc.colind).to(dev)
    plan = planmod.Plan.from_tensors(inc.N, ptr, ind)
    degE = degV = W = None
    if weighted:  # as bench.py: the hypergraph's degE / degV, HGNNConv's unit W
        hyperg = hg.HyperGraph.from_incidence(inc, dev, data_name=shape)
        degE, degV = hyperg.degE.reshape(-1), hyperg.degV.reshape(-1)
        degE = torch.where(torch.isinf(degE), torch.zeros_like(degE), degE)
        W = torch.ones(inc.M, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    Xb = torch.randn(inc.N, F, device=dev, generator=g).to(torch.bfloat16)
    Xf = Xb.float()
    Yf = torch.empty(inc.N, F, device=dev)
    Yb = torch.empty(inc.N, F, device=dev, dtype=torch.bfloat16)
    ws = torch.empty(max(plan.workspace_bytes(F), 256), dtype=torch.uint8, device=dev)
    calls = {"fp32": lambda: plan.aggregate(ptr, ind, Xf, degE, degV, W, out=Yf, workspace=ws),
             "bf16": lambda: plan.aggregate(ptr, ind, Xb, degE, degV, W, out=Yb, workspace=ws)}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for k, fn in calls.items():  # alternate: a drift of the box's clocks lands on both dtypes
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / steps)
    exact = bool((Yb.view(torch.int16) == Yf.to(torch.bfloat16).view(torch.int16)).all())
    ms = {k: statistics.median(v) for k, v in times.items()}
    n_w = 0 if not weighted else 1  # W == 1 is dropped (Plan._drop_unit_weights): degE only
    bb = b_alg(inc.N, inc.M, inc.nnz, F, n_w, weighted, 2)
    bf = b_alg(inc.N, inc.M, inc.nnz, F, n_w, weighted, 4)
    x_bytes = inc.N * F * 2
    return {"cell": name, "workload": "%s x%d F=%d%s" % (shape, replicas, F, " weighted" if weighted else ""),
            "variant": plan.auto_variant(F), "ms_fp32": round(ms["fp32"], 5), "ms_bf16": round(ms["bf16"], 5),
            "ratio": round(ms["bf16"] / ms["fp32"], 4),
            "frac_fp32": round(bf / (ms["fp32"] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4),
            "frac_bf16": round(bb / (ms["bf16"] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4),
            "bytes_ratio": round(bb / bf, 4), "x_bf16_MB": round(x_bytes / 1e6, 1),
            "xy_bf16_MB": round(2 * x_bytes / 1e6, 1), "x_fits_ic": x_bytes < IC_BYTES,
            "bit_exact": exact, "ms_rounds": {k: [round(t, 5) for t in v] for k, v in times.items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--cells", default="all")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bf16_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    want = None if args.cells == "all" else set(args.cells.split(","))
    res = []
    for cell in CELLS:
        if want is not None and cell[0] not in want:
            continue
        r = run_cell(*cell, args.steps, args.rounds, args.warmup, dev)
        res.append(r)
        print("%-18s %-26s %-5s fp32 %.4f ms  bf16 %.4f ms  ratio %.3f  frac fp32 %.3f bf16 %.3f%s  bit-exact %s" % (
            r["cell"], r["workload"], r["variant"], r["ms_fp32"], r["ms_bf16"], r["ratio"], r["frac_fp32"],
            r["frac_bf16"], " (x<IC)" if r["x_fits_ic"] else "", r["bit_exact"]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": args.steps, "rounds": args.rounds,
                       "cells": res}, f, indent=1)
    ok = all(r["bit_exact"] for r in res)
    print("invariant on the timed outputs: %s" % ("holds on every cell" if ok else "BROKEN"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
