"""A dynamic-hypergraph layer with and without the host in its forward (GPU only; no GPU is an error).

Per cell -- N in {2708, 12311, 50000} x F in {32, 128}, k = 10, X randn [N, F] -- medians of three rounds, candidates in turn:
  wall ms per forward (no grad) and per training step (forward + backward) of DynamicHypergraphConv(F, F, k), measured by
  the host clock between two synchronisations, because the host's work is the point:
    host     device_graph=False: HyperGraph.from_knn + the planned operator (the only path before this operator)
    device   device_graph=True, eager
    graph    device_graph=True, the step replayed from a hipGraph (torch.cuda.graph)
  device ms between events of hg_table_transpose and of each gather, each gather beside its bytes floor: the gathered rows,
  the written rows and idx / pos_v (no weights here) over the same run's device copy rate (the read + write rate of a
  plain copy, as tools/copy_ceiling.py measures it); and the two-hop aggregation alone, knn_aggr with a given transpose
  against Plan.aggregate on the prebuilt plan of the same hypergraph (ratio printed whichever way it falls).
A hubby cell: 50000 rows of F = 1024 randn for the search, their first 32 columns for the aggregation; its largest
in-degree is reported.

    python tools/table_aggr_probe.py [--steps 20] [--cells 2708x32,...] [--out profiles/r17_table_aggr]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

K = 10
SIZES = (2708, 12311, 50000)
WIDTHS = (32, 128)


def wall_ms(fn, steps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def device_ms(fn, steps):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def copy_rate():
    """Bytes per ms of a plain device copy (read + write) of 355 MB."""
    X = torch.rand(2708 * 1024, 32, device="cuda:0")
    Y = torch.empty_like(X)
    ms = device_ms(lambda: Y.copy_(X), 20)
    return 2 * X.numel() * 4 / ms


def rounds(forms, steps, timer):
    runs = {f: [] for f in forms}
    for _ in range(3):
        for f, fn in forms.items():
            runs[f].append(round(timer(fn, steps), 4))
    return {f: round(statistics.median(v), 4) for f, v in runs.items()}, runs


def captured(layer, X, train):
    """The layer's forward (and backward) on a static input as a replayable hipGraph."""
    G = torch.ones(X.shape[0], layer.out_channels, device=X.device)

    def step():
        if train:
            layer.lin.weight.grad = None
            layer(X).backward(G)
        else:
            with torch.no_grad():
                layer(X)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph.replay, step


def run_cell(hg, name, P, X, rate, steps):
    """P: the points the neighbours are searched in; X [N, F]: the layer's input (its first columns)."""
    from hypergef_amd import knn_graph as kg
    from hypergef_amd.plan import Plan
    N, F = X.shape
    out = {"cell": name, "N": N, "F": F, "k": K}
    # wall time of the layer.  P == X for the plain cells; the hubby cell searches in P and feeds X through a layer of width F
    # by giving the layers X and measuring the aggregation part separately below
    old = hg.DynamicHypergraphConv(F, F, k=K).to(X.device)
    new = hg.DynamicHypergraphConv(F, F, k=K, device_graph=True).to(X.device)
    new.load_state_dict(old.state_dict())
    if P is X:
        G = torch.ones(N, F, device=X.device)

        def fwd(layer):
            def f():
                with torch.no_grad():
                    layer(X)
            return f

        def train(layer):
            def f():
                layer.lin.weight.grad = None
                layer(X).backward(G)
            return f
        replay_f, _ = captured(new, X, False)
        replay_t, _ = captured(new, X, True)
        out["forward_wall_ms"], out["forward_wall_ms_runs"] = rounds(
            {"host": fwd(old), "device": fwd(new), "graph": replay_f}, steps, wall_ms)
        out["step_wall_ms"], out["step_wall_ms_runs"] = rounds(
            {"host": train(old), "device": train(new), "graph": replay_t}, steps, wall_ms)
    # device time of the pieces
    g = kg.KnnHypergraph.build(P, K)
    deg = (g.ptr_v[1:] - g.ptr_v[:-1])
    out["max_in_degree"] = int(deg.max())
    out["rows_above_seq_max"] = int((deg > kg.table_seq_max()).sum())
    Xe = kg.table_gather(g.idx, X, None, None, g.degE)
    pieces = {
        "transpose": lambda: kg.knn_transpose(g.idx),
        "gather": lambda: kg.table_gather(g.idx, X, None, None, g.degE),
        "gather_t": lambda: kg.table_gather_t(g.ptr_v, g.pos_v, K, Xe, None, None, g.degV),
        "knn_aggr": lambda: hg.ops.knn_aggr(g.idx, X, None, g.degE, g.degV, transpose=(g.ptr_v, g.pos_v)),
    }
    hyperg = hg.HyperGraph.from_knn(P, K, X.device)
    plan = Plan.from_tensors(N, hyperg.H_T_csrptr, hyperg.H_T_colind)
    plan.prepare(F)
    pieces["plan_aggregate"] = lambda: plan.aggregate(hyperg.H_T_csrptr, hyperg.H_T_colind, X, hyperg.degE, hyperg.degV)
    out["device_ms"], out["device_ms_runs"] = rounds(pieces, steps, device_ms)
    row_bytes = 4 * F
    floor = {"gather": (N * K * row_bytes + N * row_bytes + 4 * N * K + 4 * N) / rate,
             "gather_t": (N * K * row_bytes + N * row_bytes + 4 * N * K + 8 * N) / rate}
    out["bytes_floor_ms"] = {f: round(v, 4) for f, v in floor.items()}
    out["times_the_floor"] = {f: round(out["device_ms"][f] / floor[f], 2) for f in floor}
    out["knn_aggr_over_plan_aggregate"] = round(out["device_ms"]["knn_aggr"] / out["device_ms"]["plan_aggregate"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cells", default="all")
    ap.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("table_aggr_probe: no GPU (this probe measures the device and the host around it; there is no CPU fallback)")
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
        try:
            if search_F is None:
                X = torch.randn(N, F, device=dev, generator=gen)
                P = X
            else:
                P = torch.randn(N, search_F, device=dev, generator=gen)
                X = P[:, :F].contiguous()
            r = run_cell(hg, name, P, X, rate, args.steps)
        except Exception as e:  # the note says which cell could not be measured and why
            notes.append("%s: not measured: %s: %s" % (name, type(e).__name__, str(e).split("\n")[0][:200]))
            print(json.dumps({"cell": name, "not_measured": notes[-1]}), flush=True)
            torch.cuda.synchronize()
            continue
        res.append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out + ".json", "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": args.steps, "k": K, "copy_bytes_per_ms": rate,
                       "cells": res, "not_measured": notes}, f, indent=1)
        with open(args.out + ".md", "w") as f:
            f.write("# A dynamic-hypergraph layer with and without the host in its forward (tools/table_aggr_probe.py, %s, "
                    "k = %d, medians of 3 rounds)\n\n" % (torch.cuda.get_device_name(0), K))
            f.write("Wall ms between synchronisations of DynamicHypergraphConv(F, F, k): `host` = device_graph=False (the "
                    "planned path), `device` = device_graph=True eager, `graph` = the same replayed from a hipGraph.  "
                    "Device copy rate of this run: %.2f TB/s (read + write).\n\n" % (rate / 1e9))
            f.write("| cell | forward host | forward device | forward graph | step host | step device | step graph | host / graph, step |\n"
                    "|---|---|---|---|---|---|---|---|\n")
            for r in res:
                if "step_wall_ms" not in r:
                    continue
                a, b = r["forward_wall_ms"], r["step_wall_ms"]
                f.write("| %s | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.1f |\n" % (
                    r["cell"], a["host"], a["device"], a["graph"], b["host"], b["device"], b["graph"], b["host"] / b["graph"]))
            f.write("\nDevice ms between events.  Floor: gathered rows + written rows + idx / pos_v over the copy rate.  "
                    "`aggr / plan`: ops.knn_aggr with a given transpose over Plan.aggregate on the prebuilt plan (above 1: the "
                    "scheduled kernels are ahead).\n\n")
            f.write("| cell | max in-degree | rows > SEQ_MAX | transpose | gather | floor | x floor | gather_t | floor | x floor | "
                    "knn_aggr | plan.aggregate | aggr / plan |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in res:
                d, fl, tf = r["device_ms"], r["bytes_floor_ms"], r["times_the_floor"]
                f.write("| %s | %d | %d | %.4f | %.4f | %.4f | %.2f | %.4f | %.4f | %.2f | %.4f | %.4f | %.2f |\n" % (
                    r["cell"], r["max_in_degree"], r["rows_above_seq_max"], d["transpose"], d["gather"], fl["gather"],
                    tf["gather"], d["gather_t"], fl["gather_t"], tf["gather_t"], d["knn_aggr"], d["plan_aggregate"],
                    r["knn_aggr_over_plan_aggregate"]))
            for n in notes:
                f.write("\n%s\n" % n)


if __name__ == "__main__":
    main()
