"""Several heads over a kNN neighbour table: one H-head call against the loop of H single-head calls it replaces and against
the planned heads=H operators (GPU only; no GPU is an error).

Per cell -- 2708 x 32, 50000 x 32, 50000 x 128, k = 10, the table of ops.knn(randn [N, F], k), and the hubby cell of
tools/table_aggr_probe.py (50000 rows of F = 1024 for the search) -- and H in (4, 8), Ch = F / H: device ms between events
per call over 10 * steps calls, warm, medians of three rounds, candidates in turn, no gradient:
  softmax (both groups), the hyperedge gather, the vertex gather and the dot products, each as
    heads  the H-head call: ops.knn_softmax(heads=H) / knn_graph.table_gather(heads=H) / table_gather_t / table_dot
    loop   H single-head calls on contiguous column slices made beforehand (the slicing is not timed)
    one    one of those H calls
    plan   ops.incidence_softmax / incidence_gather / incidence_dot (heads=H) on the prebuilt plan of the same hypergraph
One training step of the layer F -> H x (F / H), wall ms between synchronisations: HyperGraph.from_knn +
HypergraphAttnConv(heads=H) rebuilt every forward (`host`), DynamicHypergraphConv(device_graph=True, attention=, heads=H)
eager (`device`) and replayed from a hipGraph (`graph`).

    python tools/table_heads_probe.py [--steps 20] [--cells 2708x32,...] [--out profiles/r24_table_heads]
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

from table_aggr_probe import K, device_ms, rounds, wall_ms  # noqa: E402

CELLS = (("2708x32", 2708, 32, None), ("50000x32", 50000, 32, None), ("50000x128", 50000, 128, None),
         ("hub50000x1024to32", 50000, 32, 1024))
GROUPS = ("hyperedge", "vertex")
HEADS = (4, 8)
OPS = ("softmax_hyperedge", "softmax_vertex", "gather", "gather_t", "dot")


def captured_step(layer, X, G):
    """The layer's training step on a static input: (replay of its hipGraph, the eager step)."""
    def step():
        for p in layer.parameters():
            p.grad = None
        layer(X).backward(G)

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


def run_cell(hg, name, P, X, H, steps):
    from hypergef_amd import knn_graph as kg
    ops = hg.ops
    N, F = X.shape
    dev = X.device
    out = {"cell": name, "N": N, "F": F, "k": K, "heads": H}
    g = kg.KnnHypergraph.build(P, K)
    tp = (g.ptr_v, g.pos_v)
    hyperg = hg.HyperGraph.from_knn(P, K, dev)
    ptr_t, ind_t = hyperg.H_T_csrptr, hyperg.H_T_colind
    sv, se, w = torch.randn(N, H, device=dev), torch.randn(N, H, device=dev), torch.rand(N * K, H, device=dev) + 0.5
    B = torch.randn(N, F, device=dev)
    cols = [slice(h * (F // H), (h + 1) * (F // H)) for h in range(H)]
    sv1, se1, w1 = ([t[:, h].contiguous() for h in range(H)] for t in (sv, se, w))
    X1, B1 = ([t[:, c].contiguous() for c in cols] for t in (X, B))
    single = {
        "softmax_hyperedge": lambda h: ops.knn_softmax(g.idx, sv1[h], se1[h], "hyperedge", transpose=tp),
        "softmax_vertex": lambda h: ops.knn_softmax(g.idx, sv1[h], se1[h], "vertex", transpose=tp),
        "gather": lambda h: kg.table_gather(g.idx, X1[h], w1[h]),
        "gather_t": lambda h: kg.table_gather_t(g.ptr_v, g.pos_v, K, X1[h], w1[h]),
        "dot": lambda h: kg.table_dot(g.idx, X1[h], B1[h]),
    }
    forms = {
        "softmax_hyperedge_heads": lambda: ops.knn_softmax(g.idx, sv, se, "hyperedge", transpose=tp, heads=H),
        "softmax_vertex_heads": lambda: ops.knn_softmax(g.idx, sv, se, "vertex", transpose=tp, heads=H),
        "gather_heads": lambda: kg.table_gather(g.idx, X, w, heads=H),
        "gather_t_heads": lambda: kg.table_gather_t(g.ptr_v, g.pos_v, K, X, w, heads=H),
        "dot_heads": lambda: kg.table_dot(g.idx, X, B, heads=H),
        "softmax_hyperedge_plan": lambda: ops.incidence_softmax(ptr_t, ind_t, sv, se, group="hyperedge", num_nodes=N, heads=H),
        "softmax_vertex_plan": lambda: ops.incidence_softmax(ptr_t, ind_t, sv, se, group="vertex", num_nodes=N, heads=H),
        "gather_plan": lambda: ops.incidence_gather(ptr_t, ind_t, X, w, to="hyperedge", heads=H),
        "gather_t_plan": lambda: ops.incidence_gather(ptr_t, ind_t, X, w, to="vertex", heads=H, num_nodes=N),
        "dot_plan": lambda: ops.incidence_dot(ptr_t, ind_t, X, B, heads=H),
    }
    for op, call in single.items():
        forms[op + "_loop"] = lambda call=call: [call(h) for h in range(H)]
        forms[op + "_one"] = lambda call=call: call(0)
    with torch.no_grad():
        out["device_ms"], out["device_ms_runs"] = rounds(forms, 10 * steps, device_ms)
    if name != "hub50000x1024to32":
        steps_ms = {}
        G = torch.ones(N, F, device=dev)
        for group in GROUPS:
            table = hg.DynamicHypergraphConv(F, F // H, k=K, device_graph=True, attention=group, heads=H).to(dev)

            def host_step(group=group, table=table):
                hy = hg.HyperGraph.from_knn(X, K, dev)
                layer = hg.HypergraphAttnConv(hy, F, F // H, group=group, heads=H).to(dev)
                layer.load_state_dict(dict(table.state_dict(), bias=torch.zeros(F)))
                layer(X).backward(G)
            replay, eager = captured_step(table, X, G)
            steps_ms.update({"host_" + group: host_step, "device_" + group: eager, "graph_" + group: replay})
        out["step_wall_ms"], out["step_wall_ms_runs"] = rounds(steps_ms, steps, wall_ms)
    return out


def fig(v, bold):
    return ("**%.4f**" if bold else "%.4f") % v


def write_md(path, device, res, notes):
    with open(path, "w") as f:
        f.write("# Several heads over a kNN neighbour table (tools/table_heads_probe.py, %s, k = %d, medians of 3 rounds)\n\n" % (device, K))
        f.write("Device ms between events per call, warm, no gradient.  `heads` = the one H-head call, `loop` = H single-head calls "
                "on contiguous column slices, `one` = one of them, `plan` = the planned heads=H operator on the prebuilt plan of the "
                "same hypergraph.  In bold: a `loop` or `plan` faster than `heads`.\n\n"
                "| cell | H | operator | heads | loop | one | plan | loop / heads | heads / one |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in res:
            d = r["device_ms"]
            for op in OPS:
                hd, lp, on, pl = (d["%s_%s" % (op, s)] for s in ("heads", "loop", "one", "plan"))
                f.write("| %s | %d | %s | %.4f | %s | %.4f | %s | %.2f | %.2f |\n"
                        % (r["cell"], r["heads"], op, hd, fig(lp, lp < hd), on, fig(pl, pl < hd), lp / hd, hd / on))
        f.write("\nOne training step of the layer (F -> H x F / H, k = %d), wall ms between synchronisations: `host` = "
                "HyperGraph.from_knn + HypergraphAttnConv(heads=H) rebuilt every forward, `device` = DynamicHypergraphConv("
                "device_graph=True, attention=, heads=H) eager, `graph` = that replayed from a hipGraph.  In bold: a `device` or "
                "`graph` slower than `host`.\n\n| cell | H | group | host | device | graph | host / graph |\n|---|---|---|---|---|---|---|\n" % K)
        for r in res:
            for group in GROUPS:
                if "step_wall_ms" in r:
                    s = r["step_wall_ms"]
                    h, d, gr = (s["%s_%s" % (w, group)] for w in ("host", "device", "graph"))
                    f.write("| %s | %d | %s | %.3f | %s | %s | %.1f |\n"
                            % (r["cell"], r["heads"], group, h, fig(d, d > h), fig(gr, gr > h), h / gr))
        for line in notes:
            f.write("\n%s\n" % line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cells", default="all")
    ap.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    ap.add_argument("--note", action="append", default=[], help="a line appended to STEM.md")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("table_heads_probe: no GPU (this probe measures the device; there is no CPU fallback)")
    import hypergef_amd as hg
    dev = torch.device("cuda:0")
    want = None if args.cells == "all" else set(args.cells.split(","))
    gen = torch.Generator(device=dev).manual_seed(0)
    res = []
    for name, N, F, search_F in CELLS:
        if want is not None and name not in want:
            continue
        P = torch.randn(N, search_F or F, device=dev, generator=gen)  # an error ends the probe: nothing runs after a fault
        X = P if search_F is None else P[:, :F].contiguous()
        for H in HEADS:
            r = run_cell(hg, name, P, X, H, args.steps)
            res.append(r)
            print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out + ".json", "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": args.steps, "k": K, "cells": res, "notes": args.note}, f,
                      indent=1)
        write_md(args.out + ".md", torch.cuda.get_device_name(0), res, args.note)


if __name__ == "__main__":
    main()
