"""q[e] = <sum_{u in e} A[u], sum_{v in e} B[v]>, the hot path of the degE / W gradients, three ways (GPU only; no GPU is
an error):

  * fused:    Plan.hyperedge_dot, one kernel that gathers both member rows and writes one float per hyperedge;
  * two-step: what the entries before it allow -- Plan.gather_rows hop 0 twice (two [M, F] tables written and read back),
              then (S * G).sum(1) in torch;
  * torch:    index_add_ of A[V] and B[V] into two [M, F] tables, then the same product-sum.

Per cell the three results are compared first, then each form is timed in three alternating runs.  The expectation is "fused
no slower than two-step" (2 M F 4 bytes of writes and re-reads go away); the probe reports whatever it measures.

    python tools/scale_grad_probe.py [--steps 20] [--out profiles/r11_scale_grads]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

CELLS = [(shape, rep, F) for shape, rep in (("cora", 64), ("citeseer", 64), ("pubmed", 64), ("powerlaw", 1)) for F in (32, 128)]


def timed(fn, steps, warmup=2):
    import bench
    for _ in range(warmup):
        fn()
    wall, _ = bench.timed_steps(fn, steps, torch.cuda.synchronize, lambda: None)
    return wall / steps * 1e3


def run_cell(shape, replicas, F, args, dev):
    import bench
    import numpy as np
    from hypergef_amd.plan import Plan
    _, inc = bench.make_workload(shape, replicas)
    ptr, ind = torch.from_numpy(inc.csrptr).to(dev), torch.from_numpy(inc.colind).to(dev)
    plan = Plan.from_tensors(inc.N, ptr, ind)
    g = torch.Generator(device=dev).manual_seed(0)
    A = torch.randn(inc.N, F, device=dev, generator=g)
    B = torch.randn(inc.N, F, device=dev, generator=g)
    V = ind.long()
    E = torch.from_numpy(np.repeat(np.arange(inc.M, dtype=np.int64), np.diff(inc.csrptr))).to(dev)

    def fused():
        return plan.hyperedge_dot(ptr, ind, A, B)

    def two_step():
        return (plan.gather_rows(0, ptr, ind, A) * plan.gather_rows(0, ptr, ind, B)).sum(1)

    def torch_form():
        S = torch.zeros(inc.M, F, device=dev).index_add_(0, E, A[V])
        G = torch.zeros(inc.M, F, device=dev).index_add_(0, E, B[V])
        return (S * G).sum(1)

    ref = (torch.zeros(inc.M, F, device=dev, dtype=torch.float64).index_add_(0, E, A.double()[V]) *
           torch.zeros(inc.M, F, device=dev, dtype=torch.float64).index_add_(0, E, B.double()[V])).sum(1)
    scale = float(ref.abs().max())
    err = {k: float((f().double() - ref).abs().max()) / scale for k, f in (("fused", fused), ("two_step", two_step), ("torch", torch_form))}
    runs = {"fused": [], "two_step": [], "torch": []}
    for _ in range(3):
        for k, f in (("fused", fused), ("two_step", two_step), ("torch", torch_form)):
            runs[k].append(timed(f, args.steps))
    best = {k: min(v) for k, v in runs.items()}
    return {"shape": shape, "replicas": replicas, "F": F, "N": inc.N, "M": inc.M, "nnz": int(inc.nnz), "max_err_rel": err,
            "ms": runs, "best_ms": best, "two_step_over_fused": best["two_step"] / best["fused"],
            "torch_over_fused": best["torch"] / best["fused"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="path prefix: writes <out>.json and <out>.md")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scale_grad_probe needs a GPU")
    dev = "cuda:0"
    rows = []
    for shape, rep, F in CELLS:
        r = run_cell(shape, rep, F, args, dev)
        rows.append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    lines = ["| shape | F | M | nnz | fused ms | two-step ms | torch ms | two-step / fused | torch / fused |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s x%d | %d | %d | %d | %.4f | %.4f | %.4f | %.2f | %.2f |" % (
            r["shape"], r["replicas"], r["F"], r["M"], r["nnz"], r["best_ms"]["fused"], r["best_ms"]["two_step"],
            r["best_ms"]["torch"], r["two_step_over_fused"], r["torch_over_fused"]))
    table = "\n".join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out + ".json", "w") as f:
            json.dump(rows, f, indent=1)
        with open(args.out + ".md", "w") as f:
            f.write("# hyperedge_dot against the two-step and the index_add_ forms (tools/scale_grad_probe.py, %d steps, best of "
                    "three alternating runs)\n\n%s\n" % (args.steps, table))


if __name__ == "__main__":
    main()
