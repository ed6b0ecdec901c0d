"""The attention softmax over a kNN neighbour table against the planned softmax and torch (GPU only; no GPU is an error).

Per cell -- 2708 x 32, 12311 x 32, 50000 x 32, 50000 x 128, k = 10, the table of ops.knn(randn [N, F], k), and the hubby cell of
tools/table_aggr_probe.py (50000 rows of F = 1024 for the search) -- device ms between events per call over 10 * steps calls,
warm, medians of three rounds, candidates in turn; scores sv [N], se [N] randn:
  both groups, forward and backward (torch.autograd.grad of both scores on a kept graph) of
    table  ops.knn_softmax(idx, sv, se, group) with the transpose given: hg_table_softmax_f32; backward hg_table_softmax_bwd_f32
           and hg_table_sum_f32
    plan   ops.incidence_softmax on the prebuilt plan of the same hypergraph
    torch  softmax(leaky_relu(sv[idx] + se[:, None]), 1) for 'hyperedge'; the scatter_reduce('amax') / exp / index_add_ chain for
           'vertex'
  beside the bytes floor of `table` over the same run's device copy rate: forward rows k 8 + (n + rows) 4 bytes for
  'hyperedge' (idx, alpha, the scores), rows k 12 + (2 n + rows) 4 for 'vertex' (pos_v, the sweep of idx, alpha, ptr_v, the
  scores); backward the arrays its two launches read and write once.
One training step of the attention layer, wall ms between synchronisations: HyperGraph.from_knn + HypergraphAttnConv rebuilt
every forward (`host`), DynamicHypergraphConv(device_graph=True, attention=) eager (`device`) and replayed from a hipGraph.

    python tools/table_softmax_probe.py [--steps 20] [--cells 2708x32,...] [--out profiles/r23_table_softmax]
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

from table_aggr_probe import K, captured, copy_rate, device_ms, rounds, wall_ms  # noqa: E402

CELLS = (("2708x32", 2708, 32, None), ("12311x32", 12311, 32, None), ("50000x32", 50000, 32, None),
         ("50000x128", 50000, 128, None), ("hub50000x1024to32", 50000, 32, 1024))
GROUPS = ("hyperedge", "vertex")


def torch_softmax(idx_long, sv, se, group, slope=0.2):
    x = F_.leaky_relu(sv[idx_long] + se[:, None], slope)
    if group == "hyperedge":
        return torch.softmax(x, 1)
    flat, xf = idx_long.reshape(-1), x.reshape(-1)
    m = torch.full_like(sv, float("-inf")).scatter_reduce(0, flat, xf.detach(), "amax", include_self=True)
    ex = torch.exp(xf - m[flat])
    return (ex / torch.zeros_like(sv).index_add_(0, flat, ex)[flat]).view_as(x)


def fwd_bwd(make, sv, se, G):
    a, b = sv.detach().clone().requires_grad_(True), se.detach().clone().requires_grad_(True)
    y = make(a, b)

    def fwd():
        with torch.no_grad():
            make(sv, se)
    return fwd, lambda: torch.autograd.grad(y, (a, b), G, retain_graph=True)


def run_cell(hg, name, P, X, rate, steps):
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
    sv, se = torch.randn(N, device=X.device), torch.randn(N, device=X.device)
    G = torch.randn(N, K, device=X.device)
    forms = {}
    for group in GROUPS:
        makers = {
            "table": lambda a, b, group=group: ops.knn_softmax(g.idx, a, b, group, transpose=tp),
            "plan": lambda a, b, group=group: ops.incidence_softmax(ptr_t, ind_t, a, b, group=group, num_nodes=N).view(N, K),
            "torch": lambda a, b, group=group: torch_softmax(long_idx, a, b, group),
        }
        for f, make in makers.items():
            forms["%s_%s" % (f, group)], forms["%s_%s_bwd" % (f, group)] = fwd_bwd(make, sv, se, G)
    out["device_ms"], out["device_ms_runs"] = rounds(forms, 10 * steps, device_ms)
    ent = N * K
    floor = {"table_hyperedge": ent * 8 + 8 * N, "table_vertex": ent * 12 + 12 * N,
             "table_hyperedge_bwd": ent * 16 + 12 * N + ent * 8 + 8 * N, "table_vertex_bwd": ent * 20 + 16 * N + ent * 8 + 4 * N}
    out["bytes_floor_ms"] = {f: round(v / rate, 5) for f, v in floor.items()}
    out["times_the_floor"] = {f: round(out["device_ms"][f] * rate / v, 2) for f, v in floor.items()}
    if name != "hub50000x1024to32":
        steps_ms = {}
        for group in GROUPS:
            table = hg.DynamicHypergraphConv(F, F, k=K, device_graph=True, attention=group).to(X.device)
            G2 = torch.ones(N, F, device=X.device)

            def host_step(group=group, table=table):
                hy = hg.HyperGraph.from_knn(X, K, X.device)
                layer = hg.HypergraphAttnConv(hy, F, F, group=group).to(X.device)
                layer.load_state_dict(dict(table.state_dict(), bias=torch.zeros(F)))
                layer(X).backward(G2)
            replay, eager = captured(table, X, True)
            steps_ms.update({"host_" + group: host_step, "device_" + group: eager, "graph_" + group: replay})
        out["step_wall_ms"], out["step_wall_ms_runs"] = rounds(steps_ms, steps, wall_ms)
    return out


def fig(v, bold):
    return ("**%.4f**" if bold else "%.4f") % v


def write_md(path, device, rate, res, errors):
    with open(path, "w") as f:
        f.write("# Attention softmax over a kNN neighbour table (tools/table_softmax_probe.py, %s, k = %d, medians of 3 rounds)\n\n"
                % (device, K))
        f.write("Device ms between events per call, warm; copy rate of this run %.2f TB/s (read + write).  `table` = ops.knn_softmax, "
                "`plan` = ops.incidence_softmax on the prebuilt plan of the same hypergraph, `torch` = softmax(dim=1) / the "
                "scatter_reduce chain.  `x floor`: `table` over its bytes floor.  In bold: a `plan` or `torch` faster than `table`.\n\n"
                % (rate / 1e9))
        for group in GROUPS:
            for tail, what in (("", "forward"), ("_bwd", "backward (both score gradients)")):
                f.write("Group '%s', %s\n\n| cell | max in-degree | rows > SEQ_MAX | table | floor ms | x floor | plan | torch |\n"
                        "|---|---|---|---|---|---|---|---|\n" % (group, what))
                for r in res:
                    d = r["device_ms"]
                    key = "table_%s%s" % (group, tail)
                    tb, pl, to = d[key], d["plan_%s%s" % (group, tail)], d["torch_%s%s" % (group, tail)]
                    f.write("| %s | %d | %d | %.4f | %.5f | %.2f | %s | %s |\n" % (
                        r["cell"], r["max_in_degree"], r["rows_above_seq_max"], tb, r["bytes_floor_ms"][key], r["times_the_floor"][key],
                        fig(pl, pl < tb), fig(to, to < tb)))
                f.write("\n")
        f.write("One training step of the attention layer (F -> F, k = %d), wall ms between synchronisations: `host` = "
                "HyperGraph.from_knn + HypergraphAttnConv rebuilt every forward, `device` = DynamicHypergraphConv(device_graph=True, "
                "attention=) eager, `graph` = that replayed from a hipGraph.  In bold: a `device` or `graph` slower than `host`.\n\n"
                "| cell | group | host | device | graph | host / graph |\n|---|---|---|---|---|---|\n" % K)
        for r in res:
            for group in GROUPS:
                if "step_wall_ms" in r:
                    s = r["step_wall_ms"]
                    h, d, gr = (s["%s_%s" % (w, group)] for w in ("host", "device", "graph"))
                    f.write("| %s | %s | %.3f | %s | %s | %.1f |\n" % (r["cell"], group, h, fig(d, d > h), fig(gr, gr > h), h / gr))
        for line in errors:
            f.write("\n%s\n" % line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cells", default="all")
    ap.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    ap.add_argument("--note", action="append", default=[], help="a line appended to STEM.md (measured errors of the tests)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("table_softmax_probe: no GPU (this probe measures the device; there is no CPU fallback)")
    import hypergef_amd as hg
    dev = torch.device("cuda:0")
    want = None if args.cells == "all" else set(args.cells.split(","))
    gen = torch.Generator(device=dev).manual_seed(0)
    rate = copy_rate()
    res = []
    print(json.dumps({"copy_TB_per_s": round(rate / 1e9, 3)}), flush=True)
    for name, N, F, search_F in CELLS:
        if want is not None and name not in want:
            continue
        P = torch.randn(N, search_F or F, device=dev, generator=gen)  # an error ends the probe: nothing runs after a fault
        X = P if search_F is None else P[:, :F].contiguous()
        r = run_cell(hg, name, P, X, rate, args.steps)
        res.append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out + ".json", "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": args.steps, "k": K, "copy_bytes_per_ms": rate,
                       "cells": res, "notes": args.note}, f, indent=1)
        write_md(args.out + ".md", torch.cuda.get_device_name(0), rate, res, args.note)


if __name__ == "__main__":
    main()
