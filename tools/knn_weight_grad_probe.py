"""Training through the weights of a kNN hypergraph: what learn_distances costs (GPU only; no GPU is an error).

Per cell -- N in {2708, 12311, 50000} x F in {32, 128}, k = 10, X randn [N, F] -- medians of three rounds, candidates in turn:
  wall ms per training step (forward + backward, gradients of X and of the linear's weight) of
  DynamicHypergraphConv(F, F, 10, probabilistic=True, device_graph=True), by the host clock between two synchronisations:
    off      learn_distances=False (the layer as it was: it runs no new code), with the spread of its three rounds
    on       learn_distances=True
    torch    the same gradient in torch over the same search: index_select, difference, exp, index_add_
  device ms between events of hg_table_dist_f32, the two difference gathers and hg_table_dot_f32, each beside its bytes
  floor over the same run's device copy rate (read + write of a plain copy, as tools/copy_ceiling.py measures it):
    dist       rows k F 4 gathered + Q + the output
    dot        twice that gathered + B and D + the output
    gathers    the plain gathers' floor (gathered rows, written rows, idx / pos_v, w) + ctr

    python tools/knn_weight_grad_probe.py [--steps 20] [--cells 2708x32,...] [--out profiles/r19_knn_weight_grad]
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
DEV = "cuda:0"


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
    X = torch.rand(2708 * 1024, 32, device=DEV)
    Y = torch.empty_like(X)
    ms = statistics.median(device_ms(lambda: Y.copy_(X), 10) for _ in range(3))
    return 2 * X.numel() * 4 / ms


def torch_step(hg, lin, X, G, k):
    """The learning layer's step with the weights and both hops in torch, over the device search's table."""
    x = X.clone().requires_grad_(True)
    g = hg.KnnHypergraph.build(x, k)
    flat = g.idx.reshape(-1).long()
    N = x.shape[0]
    nb = x.index_select(0, flat).view(N, k, -1)
    d2 = ((x[:, None, :] - nb) ** 2).sum(-1)
    w = torch.exp(-d2 / (g.mean[:, None]) ** 2)
    Z = lin(x)
    Xe = g.degE * (w[:, :, None] * Z.index_select(0, flat).view(N, k, -1)).sum(1)
    Y = torch.zeros_like(Z).index_add_(0, flat, (w[:, :, None] * Xe[:, None, :]).reshape(N * k, -1))
    (g.degV * Y).backward(G)
    return x.grad


def layer_step(layer, X, G):
    x = X.clone().requires_grad_(True)
    layer.lin.weight.grad = None
    layer(x).backward(G)
    return x.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cells", default=",".join("%dx%d" % (n, f) for n in SIZES for f in WIDTHS))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_weight_grad_probe needs a GPU")
    import hypergef_amd as hg
    from hypergef_amd import knn_graph as kg

    rate = copy_rate()
    results = {"copy_bytes_per_ms": rate, "cells": []}
    print("device copy rate %.0f GB/s (read + write)" % (rate / 1e6))
    print("%-10s | %-26s %8s %8s | %s" % ("cell", "step ms: off (3 rounds)", "on", "torch", "device ms (floor): dist, gather_diff, gather_t_diff, dot"))
    for cell in a.cells.split(","):
        N, F = (int(v) for v in cell.split("x"))
        torch.manual_seed(N + F)
        X = torch.randn(N, F, device=DEV)
        G = torch.randn(N, F, device=DEV)
        off = hg.DynamicHypergraphConv(F, F, K, probabilistic=True, device_graph=True).to(DEV)
        on = hg.DynamicHypergraphConv(F, F, K, probabilistic=True, device_graph=True, learn_distances=True).to(DEV)
        on.load_state_dict(off.state_dict())
        cands = {"off": lambda: layer_step(off, X, G), "on": lambda: layer_step(on, X, G),
                 "torch": lambda: torch_step(hg, on.lin, X, G, K)}
        rounds = {name: [] for name in cands}
        for _ in range(3):
            for name, fn in cands.items():
                rounds[name].append(wall_ms(fn, a.steps))
        # the kernels alone
        g = hg.KnnHypergraph.build(X, K)
        w = g.weights()
        gw = torch.randn(N * K, device=DEV)
        Xe = kg.table_gather(g.idx, X, w, None, g.degE)
        Gh = kg.table_gather(g.idx, G, w, g.degV, g.degE)
        rows_b, ent_b = N * F * 4, N * K * 4
        kern = {
            "dist": (lambda: hg.ops.knn_dist(g.idx, X), ent_b * F + rows_b + 2 * ent_b),
            "gather_diff": (lambda: kg.table_gather(g.idx, X, gw, ctr=X), ent_b * F + 2 * rows_b + 2 * ent_b),
            "gather_t_diff": (lambda: kg.table_gather_t(g.ptr_v, g.pos_v, K, X, gw, ctr=X), ent_b * F + 2 * rows_b + 2 * ent_b),
            "dot": (lambda: kg.table_dot(g.idx, G, Xe, g.degV, X, Gh), 2 * ent_b * F + 2 * rows_b + 2 * ent_b),
        }
        kms = {}
        for name, (fn, nbytes) in kern.items():
            kms[name] = (statistics.median(device_ms(fn, a.steps) for _ in range(3)), nbytes / rate)
        med = {name: statistics.median(v) for name, v in rounds.items()}
        print("%-10s | %6.3f [%6.3f .. %6.3f]  %8.3f %8.3f | %s"
              % (cell, med["off"], min(rounds["off"]), max(rounds["off"]), med["on"], med["torch"],
                 ", ".join("%.4f (%.4f)" % kms[name] for name in ("dist", "gather_diff", "gather_t_diff", "dot"))))
        results["cells"].append({"N": N, "F": F, "k": K, "step_ms_rounds": rounds, "step_ms": med,
                                 "kernel_ms": {name: {"ms": v[0], "floor_ms": v[1]} for name, v in kms.items()}})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out + ".json", "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
