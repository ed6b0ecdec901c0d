"""The incidence-weighted aggregation against the parent's unweighted pull and against torch (GPU only; no GPU is an error).

Cells (bench.make_workload, as tools/bf16_probe.py): cora x1024 F=32, pubmed x256 F=32, pubmed x64 F=128, power-law 1M/4M
F=64.  Inputs as `bench.py --weighted` builds them (degE with inf -> 0, degV; its all-ones W is dropped by the operator
layer, so none is passed here), plus random positive weights v2e, e2v in [0.5, 1.5).

Per cell:
  * parent: `bench.py --shape S --replicas R --feat F --variant pull --no-row-stream --weighted` run as a child process
    with HG_AGGR_LIB = --parent-lib (a build of the parent commit), three times, alternating with three timings of the
    weighted forward (hg_aggr_incidence_f32) in this process: the same panels + wave-task kernels without weights.
    ms per step = wall time of `--steps` calls between two synchronisations (bench.timed_steps), as bench reports it.
  * the criterion: median weighted <= median parent * (1 + dB / B_pull) * (1 + m), with B_pull = bench.b_alg + 8 M F
    (hop 1 writes the Xe table and hop 2 reads it), dB = 4 nnz (hop-1 weights) + 4 nnz (perm) + 64 nnz (hop 2's
    scattered weight reads, a full 64-byte line each), m = max(the parent's own spread over its three runs, 3 %).
  * torch: the same forward with index_add_ and the weights, and (A[V] * B[E]).sum(1) against incidence_dot: ratios.
  * for information: the weighted forward over the default unweighted `auto` call of the same cell.

    python tools/incidence_probe.py --parent-lib PATH [--steps 50] [--cells headline,...] [--out profiles/r06_incidence]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

CELLS = [  # (name, shape, replicas, F)
    ("headline", "cora", 1024, 32),
    ("pubmed256", "pubmed", 256, 32),
    ("pubmed64_F128", "pubmed", 64, 128),
    ("powerlaw_F64", "powerlaw", 1, 64),
]


def timed(fn, steps, warmup):
    import bench
    for _ in range(warmup):
        fn()
    wall, dev_s = bench.timed_steps(fn, steps, torch.cuda.synchronize, lambda: None)
    return wall / steps * 1e3


def parent_ms(shape, replicas, F, steps, warmup, lib):
    env = dict(os.environ, HG_AGGR_LIB=lib)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--shape", shape, "--replicas", str(replicas),
           "--feat", str(F), "--variant", "pull", "--no-row-stream", "--weighted", "--steps", str(steps),
           "--warmup", str(warmup)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("parent bench failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return float(line["ms_per_step"])


def run_cell(name, shape, replicas, F, args, dev):
    import bench
    import hypergef_amd as hg
    from hypergef_amd import plan as planmod
    _, inc = bench.make_workload(shape, replicas)
    ptr = torch.from_numpy(inc.csrptr).to(dev)
    ind = torch.from_numpy(inc.colind).to(dev)
    plan = planmod.Plan.from_tensors(inc.N, ptr, ind)
    hyperg = hg.HyperGraph.from_incidence(inc, dev, ngs=1 << 30)
    degE, degV = hyperg.degE.reshape(-1), hyperg.degV.reshape(-1)
    degE = torch.where(torch.isinf(degE), torch.zeros_like(degE), degE)
    del hyperg
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(inc.N, F, device=dev, generator=g)
    v2e = torch.rand(inc.nnz, device=dev, generator=g) + 0.5
    e2v = torch.rand(inc.nnz, device=dev, generator=g) + 0.5
    Y = torch.empty(inc.N, F, device=dev)
    ws = torch.empty(max(plan.incidence_workspace_bytes(F), 256), dtype=torch.uint8, device=dev)
    weighted = lambda: plan.aggregate_incidence(ptr, ind, X, v2e, e2v, degE, degV, None, out=Y, workspace=ws)  # noqa: E731
    ws_auto = torch.empty(max(plan.workspace_bytes(F), 256), dtype=torch.uint8, device=dev)
    Ya = torch.empty(inc.N, F, device=dev)
    auto = lambda: plan.aggregate(ptr, ind, X, degE, degV, None, out=Ya, workspace=ws_auto)  # noqa: E731

    par, mine = [], []
    for _ in range(3):  # alternate: a drift of the box's clocks lands on both
        par.append(parent_ms(shape, replicas, F, args.steps, args.warmup, args.parent_lib))
        mine.append(timed(weighted, args.steps, args.warmup))
    t_parent, t_w = statistics.median(par), statistics.median(mine)
    m = max((max(par) - min(par)) / t_parent, 0.03)
    b_pull = bench.b_alg(inc.N, inc.M, inc.nnz, F, 2, True) + 8 * inc.M * F  # n_w = 2: as bench.py --weighted counts it
    dB = 4 * inc.nnz + 4 * inc.nnz + 64 * inc.nnz
    limit = t_parent * (1 + dB / b_pull) * (1 + m)
    t_auto = timed(auto, args.steps, args.warmup)
    # hop 2's weights: staged through perm inside the panels (what the library does) against the alternative of a
    # separate permute pass.  The in-kernel cost is at most the difference to the call without e2v; the pass costs at
    # least what torch's gather e2v[perm] takes (one launch, 12 nnz bytes), before its 8 nnz bytes of copy traffic.
    t_no_e2v = timed(lambda: plan.aggregate_incidence(ptr, ind, X, v2e, None, degE, degV, None, out=Y, workspace=ws),
                     args.steps, args.warmup)
    perm = torch.from_numpy(plan.incidence_perm()).to(dev).long()
    t_perm_pass = timed(lambda: e2v[perm], args.steps, args.warmup)
    del perm

    # torch's formulation of the same forward
    V = ind.long()
    E = torch.repeat_interleave(torch.arange(inc.M, device=dev), ptr[1:] - ptr[:-1])

    def torch_fwd():
        xe = torch.zeros(inc.M, F, device=dev).index_add_(0, E, X[V] * v2e[:, None]) * degE[:, None]
        return torch.zeros(inc.N, F, device=dev).index_add_(0, V, xe[E] * e2v[:, None]) * degV[:, None]
    tsteps = max(3, args.steps // 10)
    t_torch = timed(torch_fwd, tsteps, 2)
    B = torch.randn(inc.M, F, device=dev, generator=g)
    out = torch.empty(inc.nnz, device=dev)
    t_dot = timed(lambda: plan.incidence_dot(ptr, ind, X, B, out=out), args.steps, args.warmup)
    t_dot_torch = timed(lambda: (X[V] * B[E]).sum(1), tsteps, 2)
    del V, E
    torch.cuda.synchronize()
    r = {"cell": name, "workload": "%s x%d F=%d" % (shape, replicas, F), "N": inc.N, "M": inc.M, "nnz": inc.nnz,
         "parent_ms_runs": [round(t, 5) for t in par], "weighted_ms_runs": [round(t, 5) for t in mine],
         "t_parent_ms": round(t_parent, 5), "t_weighted_ms": round(t_w, 5), "B_pull": b_pull, "dB": dB,
         "dB_over_B_pull": round(dB / b_pull, 4), "m": round(m, 4), "limit_ms": round(limit, 5),
         "forward_ok": t_w <= limit, "t_auto_unweighted_ms": round(t_auto, 5),
         "weighted_over_auto": round(t_w / t_auto, 3), "t_without_e2v_ms": round(t_no_e2v, 5),
         "hop2_weights_in_kernel_ms": round(t_w - t_no_e2v, 5), "t_torch_perm_pass_ms": round(t_perm_pass, 5), "t_torch_ms": round(t_torch, 5),
         "torch_over_weighted": round(t_torch / t_w, 2), "t_dot_ms": round(t_dot, 5), "t_dot_torch_ms": round(t_dot_torch, 5),
         "torch_dot_over_dot": round(t_dot_torch / t_dot, 2)}
    r["ok"] = r["forward_ok"] and t_torch > t_w and t_dot_torch > t_dot
    return r


def trace_cell(name, steps, dev):
    """Only the weighted forward and incidence_dot of one cell, `steps` times each: the body of a run under
    `rocprofv3 --kernel-trace --stats -- python tools/incidence_probe.py --trace-cell NAME`."""
    import bench
    import hypergef_amd as hg
    from hypergef_amd import plan as planmod
    _, shape, replicas, F = next(c for c in CELLS if c[0] == name)
    _, inc = bench.make_workload(shape, replicas)
    ptr = torch.from_numpy(inc.csrptr).to(dev)
    ind = torch.from_numpy(inc.colind).to(dev)
    plan = planmod.Plan.from_tensors(inc.N, ptr, ind)
    hyperg = hg.HyperGraph.from_incidence(inc, dev, ngs=1 << 30)
    degE, degV = hyperg.degE.reshape(-1), hyperg.degV.reshape(-1)
    degE = torch.where(torch.isinf(degE), torch.zeros_like(degE), degE)
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(inc.N, F, device=dev, generator=g)
    v2e = torch.rand(inc.nnz, device=dev, generator=g) + 0.5
    e2v = torch.rand(inc.nnz, device=dev, generator=g) + 0.5
    B = torch.randn(inc.M, F, device=dev, generator=g)
    Y = torch.empty(inc.N, F, device=dev)
    out = torch.empty(inc.nnz, device=dev)
    for _ in range(steps):
        plan.aggregate_incidence(ptr, ind, X, v2e, e2v, degE, degV, None, out=Y)
    for _ in range(steps):
        plan.incidence_dot(ptr, ind, X, B, out=out)
    torch.cuda.synchronize()
    print("traced %s: %d weighted forwards, %d incidence_dot calls" % (name, steps, steps))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parent-lib", default=None, help="libhgaggr.so built from the parent commit (required unless --trace-cell)")
    p.add_argument("--trace-cell", default=None, help="run only the weighted forward and incidence_dot of this cell")
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--cells", default="all")
    p.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("incidence_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    if args.trace_cell:
        trace_cell(args.trace_cell, args.steps, dev)
        return
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("incidence_probe: --parent-lib %s not found" % args.parent_lib)
    want = None if args.cells == "all" else set(args.cells.split(","))
    res = []
    for cell in CELLS:
        if want is not None and cell[0] not in want:
            continue
        r = run_cell(*cell, args, dev)
        res.append(r)
        print("%-14s %-22s parent %.4f ms (runs %s, m %.3f)  weighted %.4f ms  limit %.4f (dB/B %.3f)  %s | "
              "auto %.4f (x%.2f)  torch %.3f ms (%.1fx)  dot %.4f ms, torch %.3f ms (%.1fx)" % (
                  r["cell"], r["workload"], r["t_parent_ms"], r["parent_ms_runs"], r["m"], r["t_weighted_ms"],
                  r["limit_ms"], r["dB_over_B_pull"], "ok" if r["forward_ok"] else "OVER", r["t_auto_unweighted_ms"],
                  r["weighted_over_auto"], r["t_torch_ms"], r["torch_over_weighted"], r["t_dot_ms"],
                  r["t_dot_torch_ms"], r["torch_dot_over_dot"]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out + ".json", "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": args.steps, "cells": res}, f, indent=1)
        with open(args.out + ".md", "w") as f:
            f.write("# Incidence-weighted aggregation (tools/incidence_probe.py, %d steps per timing)\n\n" % args.steps)
            f.write("| cell | parent pull ms (3 runs) | weighted ms (3 runs) | dB/B_pull | m | limit ms | fwd | "
                    "weighted / auto | torch fwd / weighted | torch dot / incidence_dot |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in res:
                f.write("| %s | %s | %s | %.3f | %.3f | %.4f | %s | %.2f | %.1fx | %.1fx |\n" % (
                    r["workload"], " / ".join("%.4f" % t for t in r["parent_ms_runs"]),
                    " / ".join("%.4f" % t for t in r["weighted_ms_runs"]), r["dB_over_B_pull"], r["m"], r["limit_ms"],
                    "ok" if r["forward_ok"] else "OVER", r["weighted_over_auto"], r["torch_over_weighted"],
                    r["torch_dot_over_dot"]))
            f.write("\nHop 2's weights: staged per panel through perm (the library) vs a separate permute pass:\n\n"
                    "| cell | weighted ms | without e2v ms | in-kernel cost ms | torch e2v[perm] alone ms |\n|---|---|---|---|---|\n")
            for r in res:
                f.write("| %s | %.4f | %.4f | %.4f | %.4f |\n" % (r["workload"], r["t_weighted_ms"], r["t_without_e2v_ms"],
                                                               r["hop2_weights_in_kernel_ms"], r["t_torch_perm_pass_ms"]))
    ok = all(r["ok"] for r in res)
    for r in res:
        print("%-14s hop-2 weights in the panels: +%.4f ms over no e2v;  a separate permute pass alone (torch e2v[perm]): "
              "%.4f ms" % (r["cell"], r["hop2_weights_in_kernel_ms"], r["t_torch_perm_pass_ms"]))
    print("criteria: %s" % ("met on every cell" if ok else "NOT met"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
