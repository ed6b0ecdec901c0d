"""The coefficient path of HypergraphAttnConv(score="dot") against torch's formulation and against the additive path (GPU
only; no GPU is an error).

Cells: those of tools/attention_probe.py (cora x1024, pubmed x256, pubmed x64, power-law 1M/4M).  Inputs: Z, Kv [N, H C]
(randn / sqrt(C)), both requiring a gradient; C = 32, H = 1 unless --heads; slope 0.2.  Per cell and group, ours and the
comparators alternating three times (medians):
  * ours: Ke = incidence_gather(Kv, None, 'hyperedge', 1 / |e|), logits = incidence_dot(Z, Ke) C^-1/2,
    alpha = incidence_softmax(incidence_score=logits) -- the forward, and the training step (forward + backward to Z, Kv);
  * (a) torch: the member mean by index_add_, gather Z[members] and Ke[eid] ([nnz, H C] in memory), multiply-sum,
    leaky_relu, scatter_reduce(amax) softmax; outputs and gradients compared first;
  * (b) the additive path on the same cell: incidence_softmax(sv, se) with sv [N, H], se [M, H] requiring a gradient --
    the kernels of the instances without an entry logit, which this library's builds keep instruction for instruction.
Also the two softmax launches alone (entry logit against additive), forward and backward: what the per-incidence logit
costs in the kernel itself.  Nothing is asserted about the timings; the exit status is 0 when every output agreed.

    python tools/dot_attention_probe.py [--steps 30] [--heads 1] [--cells headline,...] [--out profiles/r10_dot_attention]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from attention_probe import CELLS, GROUPS, SLOPE, alternate  # noqa: E402

C = 32


def run_cell(name, shape, replicas, args, dev):
    import bench
    import hypergef_amd as hg
    from hypergef_amd import ops, plan as planmod
    H = args.heads
    _, inc = bench.make_workload(shape, replicas)
    N, M, nnz = inc.N, inc.M, inc.nnz
    hyperg = hg.HyperGraph.from_incidence(inc, dev, ngs=1 << 30)
    ptr, ind = hyperg.H_T_csrptr, hyperg.H_T_colind
    plan = planmod.cached_plan(N, ptr, ind)
    inv = torch.nan_to_num(hyperg.degE.reshape(-1), posinf=0.0)
    g = torch.Generator(device=dev).manual_seed(0)
    Z = (torch.randn(N, H * C, device=dev, generator=g) / C ** 0.5).requires_grad_(True)
    Kv = torch.randn(N, H * C, device=dev, generator=g).requires_grad_(True)
    sv = torch.randn(N, H, device=dev, generator=g).requires_grad_(True)
    se = torch.randn(M, H, device=dev, generator=g).requires_grad_(True)
    dalpha = torch.randn(nnz, H, device=dev, generator=g)
    V = ind.long()
    E = plan.segment_ids(ptr, ind, "hyperedge")
    tsteps = max(3, args.steps // 5)
    r = {"cell": name, "workload": "%s x%d" % (shape, replicas), "N": N, "M": M, "nnz": nnz, "heads": H, "C": C, "groups": {}}
    for group in GROUPS:
        idx, n = (E, M) if group == "hyperedge" else (V, N)

        def ours():
            ke = ops.incidence_gather(ptr, ind, Kv, None, to="hyperedge", scale_a=inv)
            logits = ops.incidence_dot(ptr, ind, Z, ke, heads=H).reshape(nnz, H) * C ** -0.5
            return ops.incidence_softmax(ptr, ind, None, None, group=group, negative_slope=SLOPE, num_nodes=N, heads=H,
                                         incidence_score=logits).reshape(nnz, H)

        def torch_form():
            ke = torch.zeros(M, H * C, device=dev).index_add_(0, E, Kv[V]) * inv.reshape(-1, 1)
            logits = (Z[V] * ke[E]).view(nnz, H, C).sum(2) * C ** -0.5
            s = torch.nn.functional.leaky_relu(logits, SLOPE)
            m = torch.full((n, H), -float("inf"), device=dev).scatter_reduce(0, idx.reshape(-1, 1).expand(nnz, H), s.detach(), "amax")
            e = torch.exp(s - m[idx])
            return e / torch.zeros(n, H, device=dev).index_add_(0, idx, e)[idx]

        def additive():
            return ops.incidence_softmax(ptr, ind, sv, se, group=group, negative_slope=SLOPE, num_nodes=N, heads=H).reshape(nnz, H)

        def step(fwd, leaves):
            def run():
                torch.autograd.grad(fwd(), leaves, dalpha)
            return run

        def forward(fwd):
            def run():
                with torch.no_grad():
                    fwd()
            return run
        a, b = ours(), torch_form()
        err_fwd = float(((a - b).abs() / b).max().detach())
        ga, gb = torch.autograd.grad(a, (Z, Kv), dalpha), torch.autograd.grad(b, (Z, Kv), dalpha)
        # in the 2-norm: a logit within rounding of 0 may take the other leaky branch in torch's order of summation, which
        # changes one ds by the factor `slope` and the rows it feeds with it -- a few elements, not the gradient
        err_bwd = max(float((x - y).norm() / y.norm()) for x, y in zip(ga, gb))
        err_bwd_max = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(ga, gb))
        del a, b, ga, gb
        t_fwd, t_fwd_torch = alternate(forward(ours), forward(torch_form), args.steps, tsteps)
        t_step, t_step_torch = alternate(step(ours, (Z, Kv)), step(torch_form, (Z, Kv)), args.steps, tsteps)
        t_add_fwd, t_add_step = alternate(forward(additive), step(additive, (sv, se)), args.steps, args.steps)
        # the softmax launches alone: entry logit against additive
        t = torch.randn(nnz, H, device=dev, generator=g)
        alpha = torch.empty(nnz, H, device=dev)
        svd, sed = sv.detach(), se.detach()
        k_fwd, k_fwd_add = alternate(
            lambda: plan.incidence_attention(ptr, ind, None, None, group, SLOPE, out=alpha, heads=H, entry=t),
            lambda: plan.incidence_attention(ptr, ind, svd, sed, group, SLOPE, out=alpha, heads=H), args.steps, args.steps)
        k_bwd, k_bwd_add = alternate(
            lambda: plan.incidence_attention_backward(ptr, ind, alpha, dalpha, None, None, group, SLOPE, need_sv=False,
                                                      need_se=False, heads=H, entry=t),
            lambda: plan.incidence_attention_backward(ptr, ind, alpha, dalpha, svd, sed, group, SLOPE, heads=H),
            args.steps, args.steps)
        r["groups"][group] = {
            "fwd_ms": round(t_fwd, 5), "fwd_torch_ms": round(t_fwd_torch, 5), "fwd_additive_ms": round(t_add_fwd, 5),
            "step_ms": round(t_step, 5), "step_torch_ms": round(t_step_torch, 5), "step_additive_ms": round(t_add_step, 5),
            "softmax_entry_fwd_ms": round(k_fwd, 5), "softmax_additive_fwd_ms": round(k_fwd_add, 5),
            "softmax_entry_bwd_ms": round(k_bwd, 5), "softmax_additive_bwd_ms": round(k_bwd_add, 5),
            "fwd_max_rel_diff_vs_torch": err_fwd, "bwd_l2_diff_vs_torch": err_bwd, "bwd_max_diff_vs_torch": err_bwd_max,
            "ok": err_fwd < 1e-2 and err_bwd < 1e-2}  # torch's own fp32 atomics sum 25k-entry groups in any order
        torch.cuda.empty_cache()
    r["ok"] = all(v["ok"] for v in r["groups"].values())
    return r


def write(stem, res, steps):
    with open(stem + ".json", "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "steps": steps, "cells": res}, f, indent=1)
    with open(stem + ".md", "w") as f:
        f.write("# Dot-product hypergraph attention coefficients (tools/dot_attention_probe.py, %d steps per timing)\n\n" % steps)
        f.write("Forward and training step (forward + backward to Z, Kv) of the score=\"dot\" coefficient path; (a) torch's "
                "formulation, (b) the additive path (incidence_softmax(sv, se)) on the same cell.  ms.\n\n")
        f.write("| cell | group | fwd | (a) torch | (b) additive | step | (a) torch | (b) additive |\n|---|---|---|---|---|---|---|---|\n")
        for r in res:
            for group, v in r["groups"].items():
                f.write("| %s H=%d | %s | %.4f | %.3f | %.4f | %.4f | %.3f | %.4f |\n" % (
                    r["workload"], r["heads"], group, v["fwd_ms"], v["fwd_torch_ms"], v["fwd_additive_ms"], v["step_ms"],
                    v["step_torch_ms"], v["step_additive_ms"]))
        f.write("\nThe softmax launches alone, with a logit per incidence (sv = se = NULL) and additive (sv, se; its backward "
                "includes the second segment sum).  ms.\n\n| cell | group | entry fwd | additive fwd | entry bwd | additive bwd |\n"
                "|---|---|---|---|---|---|\n")
        for r in res:
            for group, v in r["groups"].items():
                f.write("| %s H=%d | %s | %.4f | %.4f | %.4f | %.4f |\n" % (
                    r["workload"], r["heads"], group, v["softmax_entry_fwd_ms"], v["softmax_additive_fwd_ms"],
                    v["softmax_entry_bwd_ms"], v["softmax_additive_bwd_ms"]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--heads", type=int, default=1)
    p.add_argument("--cells", default="all")
    p.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dot_attention_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    want = None if args.cells == "all" else set(args.cells.split(","))
    res = []
    for cell in CELLS:
        if want is not None and cell[0] not in want:
            continue
        r = run_cell(*cell, args, dev)
        res.append(r)
        for group, v in r["groups"].items():
            print("%-10s %-9s fwd %.4f ms (torch %.3f, additive %.4f)  step %.4f ms (torch %.3f, additive %.4f)  softmax alone: "
                  "fwd %.4f / %.4f, bwd %.4f / %.4f  diff %.2g / %.2g" % (
                      r["cell"], group, v["fwd_ms"], v["fwd_torch_ms"], v["fwd_additive_ms"], v["step_ms"], v["step_torch_ms"],
                      v["step_additive_ms"], v["softmax_entry_fwd_ms"], v["softmax_additive_fwd_ms"], v["softmax_entry_bwd_ms"],
                      v["softmax_additive_bwd_ms"], v["fwd_max_rel_diff_vs_torch"], v["bwd_l2_diff_vs_torch"]), flush=True)
        if args.out:  # after every cell: a run cut short keeps what it measured
            write(args.out, res, args.steps)
        torch.cuda.empty_cache()
    sys.exit(0 if all(r["ok"] for r in res) else 1)


if __name__ == "__main__":
    main()
