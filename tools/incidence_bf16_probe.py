"""bf16 feature rows on the incidence path against the two things a bf16 model could do before (GPU only; no GPU is an error).

Cells: tools/incidence_probe.py's (cora x1024 F=32, pubmed x256 F=32, pubmed x64 F=128, power-law 1M/4M F=64), each at
H = 1 and H = 8 heads (weights [nnz] / [nnz, 8]), inputs as that probe builds them.

Per cell and H, three variants of the same call, timed in one process in alternating rounds (a drift of the clocks lands on
all three); ms per call = wall time of `--steps` calls between two synchronisations (bench.timed_steps):
  bf16   the bf16-row entries (Plan.aggregate_incidence on a bf16 X; ops.incidence_aggr with Options(incidence_bf16="rows"))
  fp32   (a) the float32 call on float32 rows
  widen  (b) what a bf16 model had to do on the parent commit: X.float(), the float32 call, .to(bfloat16)
for the forward alone and for one training step (forward + backward with gradients for X and both weight arrays).
Reported: the median and the minimum over the rounds, and the ratios bf16 / fp32 and bf16 / widen of the medians (below 1:
bf16 rows are faster).  No threshold: the expectation is only that the bytes per gathered row halve.

    python tools/incidence_bf16_probe.py [--steps 30] [--rounds 5] [--cells headline,...] [--out profiles/r14_incidence_bf16]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from incidence_probe import CELLS, timed  # noqa: E402

HEADS = (1, 8)
VARIANTS = ("bf16", "fp32", "widen")


def run_cell(name, shape, replicas, F, H, args, dev):
    import bench
    import hypergef_amd as hg
    from hypergef_amd import ops
    from hypergef_amd.plan import cached_plan
    _, inc = bench.make_workload(shape, replicas)
    ptr = torch.from_numpy(inc.csrptr).to(dev)
    ind = torch.from_numpy(inc.colind).to(dev)
    plan = cached_plan(inc.N, ptr, ind)  # the plan the operators run on
    hyperg = hg.HyperGraph.from_incidence(inc, dev, ngs=1 << 30)
    degE, degV = hyperg.degE.reshape(-1), hyperg.degV.reshape(-1)
    degE = torch.where(torch.isinf(degE), torch.zeros_like(degE), degE)
    del hyperg
    g = torch.Generator(device=dev).manual_seed(0)
    BF = torch.bfloat16
    Xb = torch.randn(inc.N, F, device=dev, generator=g).to(BF)
    Xf = Xb.float()
    wshape = (inc.nnz,) if H == 1 else (inc.nnz, H)
    v2e = torch.rand(wshape, device=dev, generator=g) + 0.5
    e2v = torch.rand(wshape, device=dev, generator=g) + 0.5
    dYb = torch.randn(inc.N, F, device=dev, generator=g).to(BF)
    dYf = dYb.float()
    ws = torch.empty(max(plan.incidence_workspace_bytes(F), 256), dtype=torch.uint8, device=dev)
    Yb, Yf = torch.empty(inc.N, F, dtype=BF, device=dev), torch.empty(inc.N, F, device=dev)
    rows = ops.Options(incidence_bf16="rows")
    fwd = {
        "bf16": lambda: plan.aggregate_incidence(ptr, ind, Xb, v2e, e2v, degE, degV, None, out=Yb, workspace=ws, heads=H),
        "fp32": lambda: plan.aggregate_incidence(ptr, ind, Xf, v2e, e2v, degE, degV, None, out=Yf, workspace=ws, heads=H),
        "widen": lambda: Yb.copy_(plan.aggregate_incidence(ptr, ind, Xb.float(), v2e, e2v, degE, degV, None, out=Yf,
                                                           workspace=ws, heads=H)),
    }
    assert torch.equal(fwd["bf16"]().view(torch.int16), fwd["widen"]().view(torch.int16)), "the two bf16 results differ"

    def step(kind):
        x = (Xf if kind == "fp32" else Xb).detach().requires_grad_(True)
        a, b = v2e.detach().requires_grad_(True), e2v.detach().requires_grad_(True)

        def run():
            x.grad = a.grad = b.grad = None
            if kind == "bf16":
                y = ops.incidence_aggr(ptr, ind, x, a, b, degE, degV, None, options=rows, heads=H)
            elif kind == "fp32":
                y = ops.incidence_aggr(ptr, ind, x, a, b, degE, degV, None, heads=H)
            else:
                y = ops.incidence_aggr(ptr, ind, x.float(), a, b, degE, degV, None, heads=H).to(BF)
            y.backward(dYf if kind == "fp32" else dYb)
        return run
    train = {k: step(k) for k in VARIANTS}

    r = {"cell": name, "workload": "%s x%d F=%d H=%d" % (shape, replicas, F, H), "N": inc.N, "M": inc.M, "nnz": inc.nnz,
         "F": F, "heads": H}
    for phase, fns in (("forward", fwd), ("train", train)):
        runs = {k: [] for k in VARIANTS}
        for _ in range(args.rounds):
            for k in VARIANTS:
                runs[k].append(timed(fns[k], args.steps, args.warmup))
        med = {k: statistics.median(v) for k, v in runs.items()}
        r[phase] = {"runs_ms": {k: [round(t, 5) for t in v] for k, v in runs.items()},
                    "median_ms": {k: round(t, 5) for k, t in med.items()},
                    "min_ms": {k: round(min(v), 5) for k, v in runs.items()},
                    "bf16_over_fp32": round(med["bf16"] / med["fp32"], 3),
                    "bf16_over_widen": round(med["bf16"] / med["widen"], 3)}
    torch.cuda.synchronize()
    return r


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--cells", default="all")
    p.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("incidence_bf16_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    want = None if args.cells == "all" else set(args.cells.split(","))
    res = []
    for name, shape, replicas, F in CELLS:
        if want is not None and name not in want:
            continue
        for H in HEADS:
            r = run_cell(name, shape, replicas, F, H, args, dev)
            res.append(r)
            for phase in ("forward", "train"):
                m = r[phase]
                print("%-26s %-8s bf16 %.4f  fp32 %.4f  widen %.4f ms (medians of %d)   bf16/fp32 %.3f   bf16/widen %.3f" % (
                    r["workload"], phase, m["median_ms"]["bf16"], m["median_ms"]["fp32"], m["median_ms"]["widen"], args.rounds,
                    m["bf16_over_fp32"], m["bf16_over_widen"]), flush=True)
        from hypergef_amd.plan import clear_plan_cache
        clear_plan_cache()
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out + ".json", "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": args.steps, "rounds": args.rounds, "cells": res}, f, indent=1)
        with open(args.out + ".md", "w") as f:
            f.write("# bf16 feature rows on the incidence path (tools/incidence_bf16_probe.py)\n\n"
                    "%s; %d rounds of %d calls per timing, the three variants alternating in one process; ms per call, median "
                    "(minimum).  bf16: the bf16-row entries; fp32: the float32 call; widen: X.float(), the float32 call, "
                    ".to(bfloat16) -- what a bf16 model had to do before.  Ratios of the medians; below 1 the bf16 rows are "
                    "faster.  Every cell measured is listed.\n\n" % (torch.cuda.get_device_name(0), args.rounds, args.steps))
            f.write("| workload | phase | bf16 ms | fp32 ms | widen ms | bf16 / fp32 | bf16 / widen |\n|---|---|---|---|---|---|---|\n")
            for r in res:
                for phase in ("forward", "train"):
                    m = r[phase]
                    f.write("| %s | %s | %s | %.3f | %.3f |\n" % (r["workload"], phase, " | ".join(
                        "%.4f (%.4f)" % (m["median_ms"][k], m["min_ms"][k]) for k in VARIANTS), m["bf16_over_fp32"],
                        m["bf16_over_widen"]))


if __name__ == "__main__":
    main()
