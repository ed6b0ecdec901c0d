"""Attention dropout fused into the coefficient kernels against what the tree offered before it: ops.incidence_softmax followed
by torch.nn.functional.dropout (GPU only; no GPU is an error).

Cells (bench.make_workload, the four of tools/attention_probe.py): cora x1024, pubmed x256, pubmed x64, power-law 1M/4M, at
H = 1 and 8 heads, both groups, p = 0.5, slope 0.2.  Scores: randn sv [N, H], se [M, H].

Per cell, H and group, all in this process, the two forms alternating three times (each run a mean over --steps calls):
  * first the undropped coefficients of the fused call are compared, bit for bit, with Plan.incidence_attention, and the
    dropped ones with where(keep, alpha * scale, 0) for the mask of hg_dropout_keep_host (on the first 2^20 positions);
  * training step of the coefficients, forward + backward through autograd with both score vectors as leaves:
    ops.incidence_softmax(dropout=p, rng_state=r) against dropout(ops.incidence_softmax(...), p).
    Condition i: the slowest fused run is faster than the fastest composed run (the margin is the spread of the runs);
  * forward alone: Plan.incidence_attention_dropout (two outputs) against Plan.incidence_attention (one).
    Condition ii: fused <= plain * (1 + dB / B) * (1 + m), dB = 4 nnz H the second output's bytes, B the bytes
    tools/attention_probe.py counts for the plain forward (streamed arrays once, every scattered access as the 64-byte lines
    it touches), m = (max - min) / min of the plain forward's own runs on that cell.

    python tools/attention_dropout_probe.py [--steps 20] [--cells headline,...] [--out profiles/r09_attention_dropout]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import torch  # noqa: E402

from attention_probe import CELLS, GROUPS, SLOPE, timed  # noqa: E402

HEADS = (1, 8)
P_DROP = 0.5


def fwd_bytes(N, M, nnz, H, group):
    """attention_probe.floor_bytes' forward with H columns: a scattered access reads 4 H contiguous bytes."""
    lines = 64 * ((4 * H + 63) // 64)
    if group == "hyperedge":
        return 4 * (M + 1) + 4 * M * H + 4 * nnz + 4 * nnz * H + lines * nnz  # ptr, se, colind, alpha out; sv[u] scattered
    return 4 * (N + 1) + 4 * N * H + 2 * 4 * nnz + 2 * lines * nnz  # ptr_v, sv, perm, ind_v; se[e] and the store scattered


def alternate(a, b, steps):
    ta, tb = [], []
    for _ in range(3):  # alternate: a drift of the box's clocks lands on both
        ta.append(timed(a, steps))
        tb.append(timed(b, steps))
    return ta, tb


def run_cell(name, shape, replicas, args, dev):
    import bench
    import _dropout_ref as dr
    import hypergef_amd as hg
    from hypergef_amd import ops, plan as planmod
    _, inc = bench.make_workload(shape, replicas)
    N, M, nnz = inc.N, inc.M, inc.nnz
    hyperg = hg.HyperGraph.from_incidence(inc, dev, ngs=1 << 30)
    ptr, ind = hyperg.H_T_csrptr, hyperg.H_T_colind
    plan = planmod.cached_plan(N, ptr, ind)
    g = torch.Generator(device=dev).manual_seed(0)
    rng = torch.tensor([0x0123456789ABCDEF, 42], dtype=torch.int64, device=dev)
    r = {"cell": name, "workload": "%s x%d" % (shape, replicas), "N": N, "M": M, "nnz": nnz, "rows": []}
    for H in HEADS:
        shp = (lambda n: (n,)) if H == 1 else (lambda n: (n, H))
        sv = torch.randn(shp(N), device=dev, generator=g)
        se = torch.randn(shp(M), device=dev, generator=g)
        dout = torch.randn(shp(nnz), device=dev, generator=g)
        for group in GROUPS:
            plain = plan.incidence_attention(ptr, ind, sv, se, group, SLOPE, heads=H)
            alpha, drop = plan.incidence_attention_dropout(ptr, ind, sv, se, group, SLOPE, P_DROP, rng, heads=H)
            torch.cuda.synchronize()
            same = torch.equal(alpha.view(torch.int32), plain.view(torch.int32))
            n = min(nnz, 1 << 20)
            keep = torch.from_numpy(dr.keep_of_state(rng, P_DROP, n, H)).to(dev).reshape(drop[:n].shape)
            want = torch.where(keep, plain[:n] * float(dr.scale(P_DROP)), torch.zeros_like(plain[:n]))
            same_drop = torch.equal(drop[:n].view(torch.int32), want.view(torch.int32))
            del alpha, drop, keep, want, plain
            svl, sel = sv.clone().requires_grad_(True), se.clone().requires_grad_(True)
            kw = dict(group=group, negative_slope=SLOPE, num_nodes=N, heads=H)

            def fused():
                out = ops.incidence_softmax(ptr, ind, svl, sel, dropout=P_DROP, rng_state=rng, **kw)
                torch.autograd.grad(out, (svl, sel), dout)

            def composed():
                out = torch.nn.functional.dropout(ops.incidence_softmax(ptr, ind, svl, sel, **kw), P_DROP, True)
                torch.autograd.grad(out, (svl, sel), dout)
            t_fused, t_comp = alternate(fused, composed, args.steps)
            f_fused, f_plain = alternate(
                lambda: plan.incidence_attention_dropout(ptr, ind, sv, se, group, SLOPE, P_DROP, rng, heads=H),
                lambda: plan.incidence_attention(ptr, ind, sv, se, group, SLOPE, heads=H), args.steps)
            B, dB = fwd_bytes(N, M, nnz, H, group), 4 * nnz * H
            m = (max(f_plain) - min(f_plain)) / min(f_plain)
            limit = statistics.median(f_plain) * (1 + dB / B) * (1 + m)
            r["rows"].append({
                "heads": H, "group": group, "width": plan.segment_info(group)["width"],
                "alpha_bits_equal_plain": same, "dropped_bits_equal_reference": same_drop,
                "step_fused_ms": [round(t, 5) for t in t_fused], "step_composed_ms": [round(t, 5) for t in t_comp],
                "step_speedup": round(statistics.median(t_comp) / statistics.median(t_fused), 3),
                "ok_i": same and same_drop and max(t_fused) < min(t_comp),
                "fwd_fused_ms": [round(t, 5) for t in f_fused], "fwd_plain_ms": [round(t, 5) for t in f_plain],
                "fwd_bytes": B, "fwd_extra_bytes": dB, "plain_spread": round(m, 4), "fwd_limit_ms": round(limit, 5),
                "fwd_ratio": round(statistics.median(f_fused) / statistics.median(f_plain), 3),
                "ok_ii": statistics.median(f_fused) <= limit})
            torch.cuda.empty_cache()
    r["ok_i"] = all(v["ok_i"] for v in r["rows"])
    r["ok_ii"] = all(v["ok_ii"] for v in r["rows"])
    return r


def write(stem, res, steps):
    with open(stem + ".json", "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "steps": steps, "p_drop": P_DROP, "cells": res}, f, indent=1)
    med = statistics.median
    with open(stem + ".md", "w") as f:
        f.write("# Attention dropout fused into the coefficient kernels (tools/attention_dropout_probe.py, %d steps per run, "
                "three alternating runs, medians; p = %g)\n\n" % (steps, P_DROP))
        f.write("| cell | H | group | step fused ms | softmax + torch dropout ms | x | i | fwd fused ms | plain softmax fwd ms | "
                "ratio | limit ms (1 + dB/B, spread m) | ii |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in res:
            for v in r["rows"]:
                f.write("| %s | %d | %s | %.4f | %.4f | %.2fx | %s | %.4f | %.4f | %.2f | %.4f (%.2f, %.1f %%) | %s |\n" % (
                    r["workload"], v["heads"], v["group"], med(v["step_fused_ms"]), med(v["step_composed_ms"]),
                    v["step_speedup"], "met" if v["ok_i"] else "NOT met", med(v["fwd_fused_ms"]), med(v["fwd_plain_ms"]),
                    v["fwd_ratio"], v["fwd_limit_ms"], 1 + v["fwd_extra_bytes"] / v["fwd_bytes"], 100 * v["plain_spread"],
                    "met" if v["ok_ii"] else "NOT met"))
        f.write("\nEvery row: the fused call's undropped coefficients equal Plan.incidence_attention bit for bit: %s; its dropped "
                "ones equal where(keep, alpha * scale, 0) for the host statement of the mask: %s.\n" % (
                    all(v["alpha_bits_equal_plain"] for r in res for v in r["rows"]),
                    all(v["dropped_bits_equal_reference"] for r in res for v in r["rows"])))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--cells", default="all")
    p.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attention_dropout_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    want = None if args.cells == "all" else set(args.cells.split(","))
    res = []
    for cell in CELLS:
        if want is not None and cell[0] not in want:
            continue
        r = run_cell(*cell, args, dev)
        res.append(r)
        for v in r["rows"]:
            print("%-10s H %d %-9s step %.4f ms (softmax + torch dropout %.4f, %.2fx) i %s | fwd %.4f ms (plain %.4f, limit %.4f) "
                  "ii %s | bits %s %s" % (r["cell"], v["heads"], v["group"], statistics.median(v["step_fused_ms"]),
                                          statistics.median(v["step_composed_ms"]), v["step_speedup"], v["ok_i"],
                                          statistics.median(v["fwd_fused_ms"]), statistics.median(v["fwd_plain_ms"]),
                                          v["fwd_limit_ms"], v["ok_ii"], v["alpha_bits_equal_plain"],
                                          v["dropped_bits_equal_reference"]), flush=True)
        if args.out:  # after every cell: a run cut short keeps what it measured
            write(args.out, res, args.steps)
        torch.cuda.empty_cache()
    ok_i, ok_ii = all(r["ok_i"] for r in res), all(r["ok_ii"] for r in res)
    print("condition i (fused step faster than softmax + torch dropout on every cell): %s" % ("met" if ok_i else "NOT met"))
    print("condition ii (fused forward within the byte-scaled limit of the plain forward): %s" % ("met" if ok_ii else "NOT met"))
    sys.exit(0 if ok_i and ok_ii else 1)


if __name__ == "__main__":
    main()
