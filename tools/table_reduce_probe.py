"""Max over a kNN neighbour table against the sum over it, the planned max and torch (GPU only; no GPU is an error).

Per cell -- N in {2708, 12311, 50000} x F in {32, 128}, k = 10, X randn [N, F], the table of ops.knn(X, k), and one hubby
cell as in tools/table_aggr_probe.py (50000 rows of F = 1024 for the search, their first 32 columns for the hops) -- device
ms between events per call over 10 * steps calls, medians of three rounds, candidates in turn, no scale anywhere:
  hop 0 (to='hyperedge') and hop 1 (to='vertex'), forward and backward (torch.autograd.grad on a kept graph) of
    max    ops.knn_gather(reduce='max'): hg_table_reduce_* forward, hg_table_select_* backward
    sum    ops.knn_gather(reduce='sum'): the sum gathers, which read the same rows; max also writes arg
    plan   ops.incidence_gather(reduce='max') on the prebuilt plan of the same hypergraph
    torch  src[idx].amax(1) / scatter_reduce('amax') over the repeated rows
  each forward and select beside its bytes floor: the gathered rows (for a select gs and arg), the written rows (for a max
  dst and arg) and idx / pos_v / ptr_v, over the same run's device copy rate.
One training step of DynamicHypergraphConv(F, F, k, first_aggr='max'), wall ms between synchronisations: device_graph=False,
device_graph=True eager, and the latter replayed from a hipGraph.

    python tools/table_reduce_probe.py [--steps 20] [--cells 2708x32,...] [--out profiles/r22_table_reduce]
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

from table_aggr_probe import K, SIZES, WIDTHS, captured, copy_rate, device_ms, rounds, wall_ms  # noqa: E402


def fwd_bwd(make, src, G):
    """(forward, backward) closures of y = make(src): the backward alone, on a graph that is kept."""
    x = src.detach().clone().requires_grad_(True)
    y = make(x)

    def fwd():
        with torch.no_grad():
            make(src)
    return fwd, lambda: torch.autograd.grad(y, x, G, retain_graph=True)


def run_cell(hg, name, P, X, rate, steps, with_layer):
    from hypergef_amd import knn_graph as kg
    ops = hg.ops
    N, F = X.shape
    out = {"cell": name, "N": N, "F": F, "k": K}
    g = kg.KnnHypergraph.build(P, K)
    deg = g.ptr_v[1:] - g.ptr_v[:-1]
    out["max_in_degree"], out["rows_above_seq_max"] = int(deg.max()), int((deg > kg.table_seq_max()).sum())
    tp = (g.ptr_v, g.pos_v)
    hyperg = hg.HyperGraph.from_knn(P, K, X.device)
    ptr_t, ind_t = hyperg.H_T_csrptr, hyperg.H_T_colind
    long_idx = g.idx.long()
    flat = long_idx.reshape(-1, 1).expand(-1, F).contiguous()
    G = torch.randn(N, F, device=X.device)
    forms = {}
    for hop, to in ((0, "hyperedge"), (1, "vertex")):
        makers = {
            "max": lambda x, to=to: ops.knn_gather(g.idx, x, to=to, reduce="max", transpose=tp),
            "sum": lambda x, to=to: ops.knn_gather(g.idx, x, to=to, reduce="sum", transpose=tp),
            "plan": lambda x, to=to: ops.incidence_gather(ptr_t, ind_t, x, to=to, reduce="max", num_nodes=N),
            "torch": (lambda x: x[long_idx].amax(1)) if hop == 0 else
                     (lambda x: torch.zeros_like(x).scatter_reduce(0, flat, x.repeat_interleave(K, 0), "amax", include_self=False)),
        }
        for f, make in makers.items():
            forms["%s%d" % (f, hop)], forms["%s%d_bwd" % (f, hop)] = fwd_bwd(make, X, G)
    out["device_ms"], out["device_ms_runs"] = rounds(forms, 10 * steps, device_ms)  # windows of several ms
    row, ent = 4 * F, N * K
    floor = {"max0": (ent * row + 2 * N * row + 4 * ent) / rate, "sum0": (ent * row + N * row + 4 * ent) / rate,
             "max0_bwd": (2 * ent * row + N * row + 4 * ent + 4 * N) / rate}
    floor.update({"max1": floor["max0"] + 4 * N / rate, "sum1": floor["sum0"] + 4 * N / rate,
                  "max1_bwd": (2 * ent * row + N * row + 4 * ent) / rate})
    out["bytes_floor_ms"] = {f: round(v, 4) for f, v in floor.items()}
    out["times_the_floor"] = {f: round(out["device_ms"][f] / v, 2) for f, v in floor.items()}
    if with_layer:
        host = hg.DynamicHypergraphConv(F, F, k=K, first_aggr="max").to(X.device)
        table = hg.DynamicHypergraphConv(F, F, k=K, first_aggr="max", device_graph=True).to(X.device)
        table.load_state_dict(host.state_dict())
        replay, _ = captured(table, X, True)

        def train(layer):
            def f():
                layer.lin.weight.grad = None
                layer(X).backward(G)
            return f
        out["step_wall_ms"], out["step_wall_ms_runs"] = rounds({"host": train(host), "device": train(table), "graph": replay},
                                                               steps, wall_ms)
    return out


def fig(v, bold):
    return ("**%.4f**" if bold else "%.4f") % v


def write_md(path, device, rate, res, notes):
    with open(path, "w") as f:
        f.write("# Max over a kNN neighbour table (tools/table_reduce_probe.py, %s, k = %d, medians of 3 rounds)\n\n" % (device, K))
        f.write("Device ms between events per call; copy rate of this run %.2f TB/s (read + write).  `max` = ops.knn_gather("
                "reduce='max'), `sum` = the sum gather of the same hop on the same table, `plan` = ops.incidence_gather(reduce="
                "'max') on the prebuilt plan, `torch` = amax of the gathered rows / scatter_reduce.  `x floor`: over the bytes "
                "floor (a max also writes arg).  In bold: a `max` slower than the `sum`, a `plan` or `torch` faster than the `max`.\n\n"
                % (rate / 1e9))
        for hop in (0, 1):
            for tail, what in (("", "forward"), ("_bwd", "backward (the select kernel; the sum's is the other sum gather)")):
                f.write("Hop %d, %s\n\n| cell | max in-degree | rows > SEQ_MAX | max | x floor | sum |%s plan | torch |\n"
                        "|---|---|---|---|---|---|%s---|---|\n" % (hop, what, " x floor |" if not tail else "", "---|" if not tail else ""))
                for r in res:
                    d, tf = r["device_ms"], r["times_the_floor"]
                    mx, sm, pl, to = (d["%s%d%s" % (c, hop, tail)] for c in ("max", "sum", "plan", "torch"))
                    f.write("| %s | %d | %d | %s | %.2f | %.4f |%s %s | %s |\n" % (
                        r["cell"], r["max_in_degree"], r["rows_above_seq_max"], fig(mx, mx > sm), tf["max%d%s" % (hop, tail)], sm,
                        " %.2f |" % tf["sum%d" % hop] if not tail else "", fig(pl, pl < mx), fig(to, to < mx)))
                f.write("\n")
        f.write("One training step of DynamicHypergraphConv(F, F, k, first_aggr='max'), wall ms between synchronisations: `host` = "
                "device_graph=False (ops.reduce_aggr on the plan), `device` = device_graph=True eager, `graph` = that replayed "
                "from a hipGraph.\n\n| cell | host | device | graph | host / graph |\n|---|---|---|---|---|\n")
        for r in res:
            if "step_wall_ms" in r:
                s = r["step_wall_ms"]
                f.write("| %s | %.3f | %s | %s | %.1f |\n" % (r["cell"], s["host"], fig(s["device"], s["device"] > s["host"]),
                                                             fig(s["graph"], s["graph"] > s["host"]), s["host"] / s["graph"]))
        for n in notes:
            f.write("\n%s\n" % n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cells", default="all")
    ap.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("table_reduce_probe: no GPU (this probe measures the device; there is no CPU fallback)")
    import hypergef_amd as hg
    dev = torch.device("cuda:0")
    want = None if args.cells == "all" else set(args.cells.split(","))
    gen = torch.Generator(device=dev).manual_seed(0)
    rate = copy_rate()
    res, notes = [], []
    print(json.dumps({"copy_TB_per_s": round(rate / 1e9, 3)}), flush=True)
    cells = [("%dx%d" % (N, F), N, F, None) for N in SIZES for F in WIDTHS] + [("hub50000x1024to32", 50000, 32, 1024)]
    for name, N, F, search_F in cells:
        if want is not None and name not in want:
            continue
        P = torch.randn(N, search_F or F, device=dev, generator=gen)  # an error ends the probe: nothing runs after a fault
        X = P if search_F is None else P[:, :F].contiguous()
        r = run_cell(hg, name, P, X, rate, args.steps, with_layer=search_F is None)
        res.append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out + ".json", "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": args.steps, "k": K, "copy_bytes_per_ms": rate,
                       "cells": res, "not_measured": notes}, f, indent=1)
        write_md(args.out + ".md", torch.cuda.get_device_name(0), rate, res, notes)


if __name__ == "__main__":
    main()
