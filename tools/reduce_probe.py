"""The max row gather and its select-gather backward against the kernels behind ops.hgnnaggr_max and against torch
(GPU only; no GPU is an error).

Cells (bench.make_workload): cora x64, citeseer x64, pubmed x64 and the power-law graph, each at F = 32 and 128; X randn.
Per cell, device time per call between two events (bench.timed_steps), the three candidates of a group timed in turn,
three rounds, medians:
  forward, hop 0 (hyperedge maxima, scaled by degE):
    reduce   Plan.gather_rows_reduce(0, 'max', degE)      hg_gather_rows_reduce_f32
    old      hg_gather_max_f32                            the kernel behind hgnnaggr_max (same values on this input)
    torch    zeros.scatter_reduce(0, E, X[V], 'amax', include_self=False) * degE
  backward of that hop, from T = the gradient of the hyperedge table:
    select   Plan.gather_rows_select(0, T, arg)           hg_gather_rows_select_f32
    old      hg_scatter_record_f32                        memset + fp32 atomics
  and each with the row gather that forms T in front (Plan.gather_rows(0, dY, degE)), which both backwards need.
Bytes floors (compulsory traffic computed from the shapes, over the 6.29 TB/s a float4 copy reaches on this part):
    forward   4 (N F + 2 M F + nnz + 2 M)       X once, value and arg written, indices, row pointers and degE
    select    4 (2 M F + N F + 2 nnz + N)       gs and arg once, dX written, H's indices and the permutation, row pointers
    scatter   4 (2 M F + 2 N F)                 T and record once, dX zeroed and written
A gather re-reads rows (nnz F elements pass through the lanes); what of that the caches absorb is what the ratio to the
floor shows.

    python tools/reduce_probe.py [--steps 30] [--cells cora,...] [--out profiles/r15_reduce]
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

CELLS = [("cora", 64), ("citeseer", 64), ("pubmed", 64), ("powerlaw", 1)]
WIDTHS = (32, 128)
COPY_BYTES_PER_S = 6.29e12


def device_ms(fn, steps, warmup):
    import bench
    for _ in range(warmup):
        fn()
    _, dev_s = bench.timed_steps(fn, steps, torch.cuda.synchronize, lambda: None)
    return dev_s / steps * 1e3


def run_cell(shape, replicas, F, args, dev):
    import bench
    import hypergef_amd as hg
    from hypergef_amd import _lib, plan as planmod
    _, inc = bench.make_workload(shape, replicas)
    N, M, nnz = inc.N, inc.M, inc.nnz
    ptr = torch.from_numpy(inc.csrptr).to(dev)
    ind = torch.from_numpy(inc.colind).to(dev)
    plan = planmod.Plan.from_tensors(N, ptr, ind)
    hyperg = hg.HyperGraph.from_incidence(inc, dev, ngs=1 << 30)
    degE = hyperg.degE.reshape(-1).contiguous()
    degE = torch.where(torch.isinf(degE), torch.zeros_like(degE), degE)
    del hyperg
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(N, F, device=dev, generator=g)
    dY = torch.randn(N, F, device=dev, generator=g)
    Xe, arg = torch.empty(M, F, device=dev), torch.empty(M, F, dtype=torch.int32, device=dev)
    Xo, rec = torch.empty(M, F, device=dev), torch.empty(M, F, dtype=torch.int32, device=dev)
    dX, dXo = torch.empty(N, F, device=dev), torch.empty(N, F, device=dev)
    ws = torch.empty(plan.reduce_workspace_bytes(F), dtype=torch.uint8, device=dev)
    L, p, stream = _lib.lib(), planmod._ptr, planmod._stream_handle(dev)
    V = ind.long()
    E = torch.repeat_interleave(torch.arange(M, device=dev), (ptr[1:] - ptr[:-1]).long())
    Eidx = E.reshape(-1, 1).expand(nnz, F)

    def reduce():
        plan.gather_rows_reduce(0, ptr, ind, X, "max", degE, None, out=Xe, arg_out=arg, workspace=ws)

    def old_fwd():
        _lib.check(L.hg_gather_max_f32(M, F, p(ptr), p(ind), p(X), p(degE), None, p(Xo), p(rec), stream))

    def torch_fwd():
        return torch.zeros(M, F, device=dev).scatter_reduce(0, Eidx, X[V], "amax", include_self=False) * degE[:, None]

    T = plan.gather_rows(0, ptr, ind, dY, degE, None)

    def select():
        plan.gather_rows_select(0, ptr, ind, T, arg, out=dX, workspace=ws)

    def old_bwd():
        _lib.check(L.hg_scatter_record_f32(N, M, F, p(T), p(rec), None, p(dXo), stream))

    def gather_T():
        plan.gather_rows(0, ptr, ind, dY, degE, None)

    reduce(), old_fwd(), select(), old_bwd()
    torch.cuda.synchronize()
    nonempty = (ptr[1:] != ptr[:-1])
    same_fwd = bool(torch.equal(Xe[nonempty], Xo[nonempty])) and bool(torch.equal(ind[arg[nonempty].long()], rec[nonempty]))
    bwd_err = float((dX - dXo).abs().max())  # the atomic sum's order differs: not bits, a size

    t = {k: [] for k in ("reduce", "old_fwd", "torch_fwd", "select", "old_bwd", "gather_T")}
    tsteps = max(3, args.steps // 5)
    for _ in range(3):  # in turn: a drift of the clocks lands on all candidates
        t["reduce"].append(device_ms(reduce, args.steps, args.warmup))
        t["old_fwd"].append(device_ms(old_fwd, args.steps, args.warmup))
        t["torch_fwd"].append(device_ms(torch_fwd, tsteps, 2))
        t["select"].append(device_ms(select, args.steps, args.warmup))
        t["old_bwd"].append(device_ms(old_bwd, args.steps, args.warmup))
        t["gather_T"].append(device_ms(gather_T, args.steps, args.warmup))
    med = {k: statistics.median(v) for k, v in t.items()}
    floors = {"fwd": 4 * (N * F + 2 * M * F + nnz + 2 * M), "select": 4 * (2 * M * F + N * F + 2 * nnz + N),
              "scatter": 4 * (2 * M * F + 2 * N * F)}
    floor_ms = {k: b / COPY_BYTES_PER_S * 1e3 for k, b in floors.items()}
    del V, E, Eidx
    return {"workload": "%s x%d F=%d" % (shape, replicas, F), "N": N, "M": M, "nnz": nnz, "F": F,
            "max_len": int(plan.info["max_len"][0]), "ms_runs": {k: [round(x, 5) for x in v] for k, v in t.items()},
            "ms": {k: round(v, 5) for k, v in med.items()}, "floor_bytes": floors,
            "floor_ms": {k: round(v, 5) for k, v in floor_ms.items()},
            "old_over_reduce": round(med["old_fwd"] / med["reduce"], 2), "torch_over_reduce": round(med["torch_fwd"] / med["reduce"], 2),
            "old_bwd_over_select": round(med["old_bwd"] / med["select"], 2),
            "old_bwd_with_gather_over_select_with_gather": round((med["old_bwd"] + med["gather_T"]) / (med["select"] + med["gather_T"]), 2),
            "reduce_over_floor": round(med["reduce"] / floor_ms["fwd"], 2), "select_over_floor": round(med["select"] / floor_ms["select"], 2),
            "old_bwd_over_floor": round(med["old_bwd"] / floor_ms["scatter"], 2),
            "forward_same_bits": same_fwd, "backward_max_abs_diff": bwd_err}


def words(ratio):
    return "%.2fx faster" % ratio if ratio >= 1 else "%.2fx slower" % (1 / ratio)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cells", default="all")
    ap.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reduce_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    want = None if args.cells == "all" else set(args.cells.split(","))
    res = []
    for shape, replicas in CELLS:
        if want is not None and shape not in want:
            continue
        for F in WIDTHS:
            r = run_cell(shape, replicas, F, args, dev)
            res.append(r)
            m = r["ms"]
            print("%-22s fwd: reduce %.4f ms (floor %.4f)  old %.4f  torch %.4f | bwd: select %.4f ms (floor %.4f)  scatter %.4f "
                  "(floor %.4f)  gather T %.4f | same bits %s" % (r["workload"], m["reduce"], r["floor_ms"]["fwd"], m["old_fwd"],
                                                                  m["torch_fwd"], m["select"], r["floor_ms"]["select"], m["old_bwd"],
                                                                  r["floor_ms"]["scatter"], m["gather_T"], r["forward_same_bits"]), flush=True)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out + ".json", "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": args.steps, "cells": res}, f, indent=1)
        with open(args.out + ".md", "w") as f:
            f.write("# Max row gather and select-gather backward (tools/reduce_probe.py, %s, %d steps per timing, medians of 3)\n\n"
                    % (torch.cuda.get_device_name(0), args.steps))
            f.write("Device ms per call.  `old`: hg_gather_max_f32 / hg_scatter_record_f32, the kernels behind hgnnaggr_max.  "
                    "Floors: compulsory bytes over 6.29 TB/s (the docstring of the tool).\n\n")
            f.write("Forward, hop 0:\n\n| cell | longest row | reduce ms | floor ms | x floor | old ms | reduce vs old | torch amax ms | "
                    "reduce vs torch | same bits |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in res:
                m = r["ms"]
                f.write("| %s | %d | %.4f | %.4f | %.1f | %.4f | %s | %.4f | %s | %s |\n" % (
                    r["workload"], r["max_len"], m["reduce"], r["floor_ms"]["fwd"], r["reduce_over_floor"], m["old_fwd"],
                    words(r["old_over_reduce"]), m["torch_fwd"], words(r["torch_over_reduce"]), r["forward_same_bits"]))
            f.write("\nBackward of that hop:\n\n| cell | select ms | floor ms | x floor | scatter_record ms | floor ms | x floor | select vs "
                    "scatter | row gather of T ms | with it in front |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in res:
                m = r["ms"]
                f.write("| %s | %.4f | %.4f | %.1f | %.4f | %.4f | %.1f | %s | %.4f | %s |\n" % (
                    r["workload"], m["select"], r["floor_ms"]["select"], r["select_over_floor"], m["old_bwd"], r["floor_ms"]["scatter"],
                    r["old_bwd_over_floor"], words(r["old_bwd_over_select"]), m["gather_T"],
                    words(r["old_bwd_with_gather_over_select_with_gather"])))


if __name__ == "__main__":
    main()
