"""The hypergraph attention coefficients against torch's formulation and against a bytes floor (GPU only; no GPU is an error).

Cells (bench.make_workload, the four of tools/incidence_probe.py): cora x1024, pubmed x256, pubmed x64, power-law 1M/4M.  The
coefficients have no feature width; F = 32 matters only for the layer row.  Scores: randn sv [N], se [M]; slope 0.2.

Per cell and group ('hyperedge' / 'vertex'), all in this process, ours and torch alternating three times (medians):
  * forward: Plan.incidence_attention against leaky_relu(sv[V] + se[E]) -> scatter_reduce(amax) -> gather -> exp ->
    index_add_ -> gather -> divide; outputs compared first (relative to alpha);
  * backward: Plan.incidence_attention_backward (ds, dsv, dse) against torch.autograd.grad through that torch forward
    (retain_graph, so only the backward is timed); dsv / dse compared first;
  * the bytes floor: every streamed [nnz] / [N] / [M] array counted once at 4 bytes per element, every scattered 4-byte
    access as a whole 64-byte line (as DESIGN 3.8 counts hop 2's weights), divided by the copy rate measured in the same
    run (a device copy of a 355 MB tensor, read + write, as tools/copy_ceiling.py measures it);
  * one training step (forward + backward, F = 32 -> 32) of models.HypergraphAttnConv against the same layer with torch's
    coefficients around the same incidence_aggr, and the coefficient path alone (forward + backward) in both forms: its
    share of the step before and after.

The condition: our forward and our backward are each faster than torch's on every cell and group.

    python tools/attention_probe.py [--steps 30] [--cells headline,...] [--out profiles/r07_attention]
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

CELLS = [  # (name, shape, replicas)
    ("headline", "cora", 1024),
    ("pubmed256", "pubmed", 256),
    ("pubmed64", "pubmed", 64),
    ("powerlaw", "powerlaw", 1),
]
GROUPS = ("hyperedge", "vertex")
SLOPE = 0.2
F = 32


def timed(fn, steps, warmup=3):
    import bench
    for _ in range(warmup):
        fn()
    wall, _ = bench.timed_steps(fn, steps, torch.cuda.synchronize, lambda: None)
    return wall / steps * 1e3


def alternate(a, b, steps, tsteps):
    ta, tb = [], []
    for _ in range(3):  # alternate: a drift of the box's clocks lands on both
        ta.append(timed(a, steps))
        tb.append(timed(b, tsteps, 2))
    return statistics.median(ta), statistics.median(tb)


def copy_rate():
    """Bytes per second of a plain device copy (read + write)."""
    X = torch.rand(2708 * 1024, 32, device="cuda:0")
    Y = torch.empty_like(X)
    ms = timed(lambda: Y.copy_(X), 50, 5)
    return 2 * X.numel() * 4 / (ms * 1e-3)


def floor_bytes(N, M, nnz, group):
    """(forward, backward) bytes: streamed arrays once, scattered 4-byte accesses as 64-byte lines."""
    if group == "hyperedge":
        fwd = 4 * (M + 1) + 4 * M + 4 * nnz + 4 * nnz + 64 * nnz  # ptr, se, colind, alpha out; sv[u] scattered
        bwd = (4 * (M + 1) + 4 * M + 4 * nnz + 3 * 4 * nnz + 64 * nnz + 4 * M  # + alpha, dalpha, ds; sv[u]; dse
               + 4 * (N + 1) + 4 * nnz + 64 * nnz + 4 * N)                     # dsv: ptr_v, perm, ds[perm] scattered, out
    else:
        fwd = 4 * (N + 1) + 4 * N + 2 * 4 * nnz + 2 * 64 * nnz  # ptr_v, sv, perm, ind_v; se[e] and the alpha store scattered
        bwd = (4 * (N + 1) + 4 * N + 2 * 4 * nnz + 4 * 64 * nnz + 4 * N  # alpha, dalpha, ds through perm, se[e] scattered; dsv
               + 4 * (M + 1) + 4 * nnz + 4 * M)                          # dse: ptr, ds streamed, out
    return fwd, bwd


def torch_alpha(sv, se, V, E, idx, n, slope=SLOPE):
    s = torch.nn.functional.leaky_relu(sv[V] + se[E], slope)
    m = torch.full((n,), -float("inf"), device=s.device).scatter_reduce(0, idx, s.detach(), "amax")
    e = torch.exp(s - m[idx])
    return e / torch.zeros(n, device=s.device).index_add_(0, idx, e)[idx]


def run_cell(name, shape, replicas, args, dev, rate):
    import bench
    import hypergef_amd as hg
    from hypergef_amd import models, plan as planmod
    _, inc = bench.make_workload(shape, replicas)
    N, M, nnz = inc.N, inc.M, inc.nnz
    hyperg = hg.HyperGraph.from_incidence(inc, dev, ngs=1 << 30)
    ptr, ind = hyperg.H_T_csrptr, hyperg.H_T_colind
    plan = planmod.cached_plan(N, ptr, ind)
    g = torch.Generator(device=dev).manual_seed(0)
    sv = torch.randn(N, device=dev, generator=g)
    se = torch.randn(M, device=dev, generator=g)
    dalpha = torch.randn(nnz, device=dev, generator=g)
    V = ind.long()
    E = plan.segment_ids(ptr, ind, "hyperedge")
    tsteps = max(3, args.steps // 5)
    r = {"cell": name, "workload": "%s x%d" % (shape, replicas), "N": N, "M": M, "nnz": nnz, "groups": {}}
    for group in GROUPS:
        idx, n = (E, M) if group == "hyperedge" else (V, N)
        info = plan.segment_info(group)
        alpha = torch.empty(nnz, device=dev)
        ours_fwd = lambda: plan.incidence_attention(ptr, ind, sv, se, group, SLOPE, out=alpha)  # noqa: E731
        ours_fwd()
        ref = torch_alpha(sv, se, V, E, idx, n)
        err_fwd = float(((alpha - ref).abs() / ref).max())
        ours_bwd = lambda: plan.incidence_attention_backward(ptr, ind, alpha, dalpha, sv, se, group, SLOPE)  # noqa: E731
        _, dsv, dse = ours_bwd()
        svl, sel = sv.clone().requires_grad_(True), se.clone().requires_grad_(True)
        at = torch_alpha(svl, sel, V, E, idx, n)
        torch_bwd = lambda: torch.autograd.grad(at, (svl, sel), dalpha, retain_graph=True)  # noqa: E731
        tv, te = torch_bwd()
        err_bwd = max(float((dsv - tv).abs().max() / tv.abs().max()), float((dse - te).abs().max() / te.abs().max()))
        t_fwd, t_fwd_torch = alternate(ours_fwd, lambda: torch_alpha(sv, se, V, E, idx, n), args.steps, tsteps)
        t_bwd, t_bwd_torch = alternate(ours_bwd, torch_bwd, args.steps, tsteps)
        del at, svl, sel, tv, te, ref
        fb, bb = floor_bytes(N, M, nnz, group)
        r["groups"][group] = {
            "width": info["width"], "long_rows": int(len(info["long_rows"])),
            "fwd_ms": round(t_fwd, 5), "fwd_torch_ms": round(t_fwd_torch, 5), "fwd_speedup": round(t_fwd_torch / t_fwd, 2),
            "bwd_ms": round(t_bwd, 5), "bwd_torch_ms": round(t_bwd_torch, 5), "bwd_speedup": round(t_bwd_torch / t_bwd, 2),
            "fwd_floor_ms": round(fb / rate * 1e3, 5), "bwd_floor_ms": round(bb / rate * 1e3, 5),
            "fwd_over_floor": round(t_fwd / (fb / rate * 1e3), 2), "bwd_over_floor": round(t_bwd / (bb / rate * 1e3), 2),
            "fwd_max_rel_diff_vs_torch": err_fwd, "bwd_max_diff_vs_torch": err_bwd,
            "ok": t_fwd < t_fwd_torch and t_bwd < t_bwd_torch}
        torch.cuda.empty_cache()

    # one training step of the layer, our coefficients against torch's around the same incidence_aggr
    class TorchCoefficients(models.HypergraphAttnConv):
        def coefficients(self, Z):
            sv_ = Z @ self.a_v
            ze = (Z @ self.a_e)[self._members]
            se_ = torch.zeros(M, device=Z.device).index_add_(0, E, ze) * self._inv_size
            return torch_alpha(sv_, se_, V, E, E if self.group == "hyperedge" else V, M if self.group == "hyperedge" else N,
                               self.negative_slope)
    X = torch.randn(N, F, device=dev, generator=g)
    dY = torch.randn(N, F, device=dev, generator=g)
    torch.manual_seed(0)
    ours = models.HypergraphAttnConv(hyperg, F, F).to(dev)
    theirs = TorchCoefficients(hyperg, F, F).to(dev)
    theirs.load_state_dict(ours.state_dict())

    def step(layer):
        def run():
            for p in layer.parameters():
                p.grad = None
            layer(X).backward(dY)
        return run

    def coeff(layer):
        Z = layer.lin(X).detach().requires_grad_(True)

        def run():
            for p in (layer.a_v, layer.a_e):
                p.grad = None
            Z.grad = None
            layer.coefficients(Z).backward(dalpha)
        return run
    step(ours)()
    step(theirs)()
    diff = max(float((a.grad - b.grad).abs().max() / b.grad.abs().max()) for a, b in zip(ours.parameters(), theirs.parameters()))
    t_step, t_step_torch = alternate(step(ours), step(theirs), max(3, args.steps // 3), tsteps)
    t_co, t_co_torch = alternate(coeff(ours), coeff(theirs), max(3, args.steps // 3), tsteps)
    r["layer"] = {"F": F, "step_ms": round(t_step, 4), "step_torch_coeff_ms": round(t_step_torch, 4),
                  "coeff_ms": round(t_co, 4), "coeff_torch_ms": round(t_co_torch, 4),
                  "coeff_share_before": round(t_co_torch / t_step_torch, 3), "coeff_share_after": round(t_co / t_step, 3),
                  "grad_max_diff_vs_torch": diff}
    r["ok"] = all(v["ok"] for v in r["groups"].values())
    return r


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--cells", default="all")
    p.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attention_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    rate = copy_rate()
    print("copy rate %.2f TB/s" % (rate / 1e12), flush=True)
    want = None if args.cells == "all" else set(args.cells.split(","))
    res = []
    for cell in CELLS:
        if want is not None and cell[0] not in want:
            continue
        r = run_cell(*cell, args, dev, rate)
        res.append(r)
        for group, v in r["groups"].items():
            print("%-10s %-9s fwd %.4f ms (torch %.3f, %.1fx; floor %.4f, x%.2f)  bwd %.4f ms (torch %.3f, %.1fx; floor %.4f, "
                  "x%.2f)  width %d, %d long rows" % (r["cell"], group, v["fwd_ms"], v["fwd_torch_ms"], v["fwd_speedup"],
                                                     v["fwd_floor_ms"], v["fwd_over_floor"], v["bwd_ms"], v["bwd_torch_ms"],
                                                     v["bwd_speedup"], v["bwd_floor_ms"], v["bwd_over_floor"], v["width"],
                                                     v["long_rows"]), flush=True)
        la = r["layer"]
        print("%-10s layer step %.3f ms (torch coefficients %.3f)  coefficient path %.3f ms = %.0f %% of the step (torch: %.3f ms "
              "= %.0f %%)" % (r["cell"], la["step_ms"], la["step_torch_coeff_ms"], la["coeff_ms"], 100 * la["coeff_share_after"],
                             la["coeff_torch_ms"], 100 * la["coeff_share_before"]), flush=True)
        if args.out:  # after every cell: a run cut short keeps what it measured
            write(args.out, res, rate, args.steps)
        torch.cuda.empty_cache()
    ok = all(r["ok"] for r in res)
    print("condition (forward and backward each faster than torch on every cell and group): %s" % ("met" if ok else "NOT met"))
    sys.exit(0 if ok else 1)


def write(stem, res, rate, steps):
    with open(stem + ".json", "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "steps": steps, "copy_rate_TBps": round(rate / 1e12, 3),
                   "cells": res}, f, indent=1)
    with open(stem + ".md", "w") as f:
        f.write("# Hypergraph attention coefficients (tools/attention_probe.py, %d steps per timing, copy rate %.2f TB/s)\n\n"
                % (steps, rate / 1e12))
        f.write("| cell | group | width / long rows | fwd ms | torch fwd ms | x | fwd / floor | bwd ms | torch bwd ms | x | "
                "bwd / floor |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in res:
            for group, v in r["groups"].items():
                f.write("| %s | %s | %d / %d | %.4f | %.3f | %.1fx | %.2f | %.4f | %.3f | %.1fx | %.2f |\n" % (
                    r["workload"], group, v["width"], v["long_rows"], v["fwd_ms"], v["fwd_torch_ms"], v["fwd_speedup"],
                    v["fwd_over_floor"], v["bwd_ms"], v["bwd_torch_ms"], v["bwd_speedup"], v["bwd_over_floor"]))
        f.write("\nOne training step of HypergraphAttnConv (F = %d -> %d, group hyperedge), coefficients ours / torch's:\n\n"
                "| cell | step ms | step ms, torch coefficients | coefficient path ms | torch's ms | share of the step after | "
                "before |\n|---|---|---|---|---|---|---|\n" % (F, F))
        for r in res:
            la = r["layer"]
            f.write("| %s | %.3f | %.3f | %.3f | %.3f | %.0f %% | %.0f %% |\n" % (
                r["workload"], la["step_ms"], la["step_torch_coeff_ms"], la["coeff_ms"], la["coeff_torch_ms"],
                100 * la["coeff_share_after"], 100 * la["coeff_share_before"]))


if __name__ == "__main__":
    main()
