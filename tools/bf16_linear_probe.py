"""The bf16 linear layer on the bf16 MFMA (Plan.aggregate_linear_bf16) against what a bf16 model runs today and against the
fp32 fused layer (GPU only; no GPU is an error).  Forward only, HIP events, one process.

Cells (bench.make_workload): pubmed x64 128 -> 128; cora x1024 32 -> 32, 64 -> 64, 128 -> 128.  Every cell's tables (X, Y and
the fp32 forms' twice as wide ones) lie beyond the 256 MiB Infinity Cache.  Forms per cell:
  new     hg_aggr_linear_res_bf16, variant auto (the kernels it ran: hg_aggr_linear_bf16_path)
  (a)     today's bf16 layer: torch's GEMM X . W^T, then the bf16 aggregation at F_out (ops._SumAggrLinear, linear_bf16='torch')
  (b)     the fp32 fused layer hg_aggr_linear_f32 on the widened operands, math f32 and (F_in = 128) bf16x6
Each round times every form `--iters` calls between two events after `--warmup` calls, first in the order listed, then in the
reverse order; the table gives the median and the minimum over all rounds and both orders, and new's ratio to each other form
(below 1: new is faster).  Before timing, each cell checks new's T_out against the fp32 form's rounded row (bit for bit) and
its Y against the float64 product on 4096 sampled rows (the bound of tests/test_bf16_linear_gpu.py).

    python tools/bf16_linear_probe.py [--iters 20] [--rounds 3] [--out profiles/r12_bf16_linear.md]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

CELLS = [  # (name, shape, replicas, F_in, F_out)
    ("pubmed x64 128->128", "pubmed", 64, 128, 128),
    ("cora x1024 32->32", "cora", 1024, 32, 32),
    ("cora x1024 64->64", "cora", 1024, 64, 64),
    ("cora x1024 128->128", "cora", 1024, 128, 128),
]
PATHS = {1: "panels", 2: "rows kernel", 3: "panels + rows kernel"}


def event_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def check(plan, ptr, ind, X, Wl, F_in, dev):
    """T_out bit for bit and Y within the contract's bound (sampled rows), at the cell's scale."""
    N = X.shape[0]
    T = torch.empty_like(X)
    Y = plan.aggregate_linear_bf16(ptr, ind, X, Wl, t_out=T)
    T32 = torch.empty(N, F_in, device=dev)
    plan.aggregate_linear(ptr, ind, X.float(), Wl.float(), t_out=T32)
    t_same = bool(torch.equal(T.view(torch.int16), T32.to(torch.bfloat16).view(torch.int16)))
    del T32
    rows = torch.randint(0, N, (4096,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    t, w = T[rows].double(), Wl.double()
    yref = t @ w.t()
    e = 2 * F_in * 2.0 ** -24 * (t.abs() @ w.abs().t())
    y_ok = bool(((Y[rows].double() - yref).abs() <= 2.0 ** -8 * (yref.abs() + e) + e).all())
    return t_same, y_ok


def run_cell(cell, args, dev):
    import bench
    from hypergef_amd import plan as planmod
    name, shape, replicas, F_in, F_out = cell
    _, inc = bench.make_workload(shape, replicas)
    ptr, ind = torch.from_numpy(inc.csrptr).to(dev), torch.from_numpy(inc.colind).to(dev)
    plan = planmod.Plan.from_tensors(inc.N, ptr, ind)
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(inc.N, F_in, device=dev, generator=g).to(torch.bfloat16)
    Wl = (torch.randn(F_out, F_in, device=dev, generator=g) / F_in ** 0.5).to(torch.bfloat16)
    X32, W32 = X.float(), Wl.float()
    Yb = torch.empty(inc.N, F_out, device=dev, dtype=torch.bfloat16)
    Y32 = torch.empty(inc.N, F_out, device=dev)
    ws_lin = torch.empty(max(plan.linear_workspace_bytes(F_in), 256), dtype=torch.uint8, device=dev)
    ws_out = torch.empty(max(plan.workspace_bytes(F_out), 256), dtype=torch.uint8, device=dev)
    packed_b = planmod.pack_linear_bf16(Wl)
    packed_f = planmod.pack_linear(W32, bf16x6=True)
    path = plan.linear_bf16_path(F_in, F_out, "auto")
    t_same, y_ok = check(plan, ptr, ind, X, Wl, F_in, dev)

    forms = [
        ("new", lambda: plan.aggregate_linear_bf16(ptr, ind, X, Wl, out=Yb, workspace=ws_lin, packed=packed_b)),
        ("(a) torch GEMM + bf16 aggregation",
         lambda: plan.aggregate(ptr, ind, torch.nn.functional.linear(X, Wl), out=Yb, workspace=ws_out)),
        ("(b) fp32 fused, f32", lambda: plan.aggregate_linear(ptr, ind, X32, W32, out=Y32, workspace=ws_lin, packed=packed_f)),
    ]
    if F_in == 128:
        forms.append(("(b) fp32 fused, bf16x6",
                      lambda: plan.aggregate_linear(ptr, ind, X32, W32, out=Y32, workspace=ws_lin, packed=packed_f, math="bf16x6")))
    times = {n: [] for n, _ in forms}
    for _ in range(args.rounds):
        for order in (forms, forms[::-1]):
            for n, fn in order:
                times[n].append(event_ms(fn, args.iters, args.warmup))
    return dict(name=name, N=inc.N, nnz=inc.nnz, path=path, t_same=t_same, y_ok=y_ok,
                times={n: (statistics.median(v), min(v)) for n, v in times.items()}, order=[n for n, _ in forms])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells", type=str, default="")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "r12_bf16_linear.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bf16_linear_probe needs a GPU")
    dev = "cuda:0"
    want = [c for c in CELLS if not args.cells or any(k in c[0] for k in args.cells.split(","))]
    lines = ["# bf16 linear layer on the bf16 MFMA: forward, ms per call (median / min)", "",
             "`tools/bf16_linear_probe.py --iters %d --warmup %d --rounds %d` on %s; HIP events, both orders per round, one "
             "process.  Ratios are new / other on the medians (below 1: new is faster)." % (
                 args.iters, args.warmup, args.rounds, torch.cuda.get_device_name(0)), "",
             "| cell | rows | kernels of new | form | median ms | min ms | new / form |", "|---|---|---|---|---|---|---|"]
    for cell in want:
        r = run_cell(cell, args, dev)
        new = r["times"]["new"][0]
        for n in r["order"]:
            med, mn = r["times"][n]
            lines.append("| %s | %d | %s | %s | %.3f | %.3f | %s |" % (
                r["name"], r["N"], PATHS.get(r["path"], str(r["path"])), n, med, mn, "" if n == "new" else "%.2f" % (new / med)))
        lines.append("| %s | | | check: T_out == round_bf16(fp32 row) %s; Y within the contract's bound on 4096 rows %s | | | |" % (
            r["name"], "yes" if r["t_same"] else "NO", "yes" if r["y_ok"] else "NO"))
        print("\n".join(lines[-(len(r["order"]) + 1):]), flush=True)
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
