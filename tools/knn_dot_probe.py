"""ops.knn(form="dot") against form="difference" and the two torch forms of tools/knn_probe.py (GPU only; no GPU is an error).

Per cell, device ms per call between two events, the forms timed in turn, three rounds, medians (tools/knn_probe.py's
run_cell), and each form's peak allocation above what is live before the call:
    dot          ops.knn(X, k, form="dot", return_mean=True)          hg_knn_dot_f32, cand_slices = 0
    difference   ops.knn(X, k, return_mean=True)                      hg_knn_f32 (hg_knn.hip, the kernel as it was), cand_slices = 0
    cdist_exact  torch.cdist(X, X, compute_mode="donot_use_mm_for_euclid_dist").topk(k, largest=False)
    cdist_mm     torch.cdist(X, X).topk(k, largest=False)
and the share of rows that were not certified and took the exhaustive path, on randn rows and on relu(randn + 0.5) rows
(non-negative, far from the origin: the norms, and so the bound, are large against the distances).  The timed input is the
randn one; with --relu-times the non-negative one is timed too (dot only).  idx and dist of the two forms are compared on
every cell that is run.
Cells: N in {2012, 2708, 12311, 50000} x F in {64, 256, 1024, 2048, 4096}, k = 10.

    python tools/knn_dot_probe.py [--steps 5] [--cells 2012x64,...] [--out profiles/r18_knn_dot]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import knn_probe  # noqa: E402

K = 10
SIZES = (2012, 2708, 12311, 50000)
WIDTHS = (64, 256, 1024, 2048, 4096)


def write_md(path, device, res):
    with open(path, "w") as f:
        f.write("# ops.knn(form=\"dot\") against form=\"difference\" and torch.cdist + topk (tools/knn_dot_probe.py, %s, k = %d, "
                "medians of 3 rounds)\n\n" % (device, K))
        f.write("Device ms per call, randn rows; `fallback`: the share of rows that were not certified, on randn rows / on "
                "relu(randn + 0.5) rows; peak allocation above the live set.  **Bold**: `dot` is the slower of the two forms.\n\n")
        f.write("| cell | dot ms | difference ms | cdist exact ms | cdist mm ms | fallback randn | fallback relu | dot ms relu | "
                "dot peak MB | difference peak MB | same idx, dist |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in res:
            m, p = r["ms"], r["peak_bytes"]

            def cell(form, table, scale=1.0, fmt="%.3f"):
                return fmt % (table[form] * scale) if form in table else r["note"].get(form, "-")
            dot = "%.3f" % m["dot"]
            if m["dot"] > m["difference"]:
                dot = "**%s**" % dot
            f.write("| %s | %s | %.3f | %s | %s | %.4f | %.4f | %s | %.2f | %.2f | %s |\n" % (
                r["cell"], dot, m["difference"], cell("cdist_exact", m), cell("cdist_mm", m), r["fallback_share"]["randn"],
                r["fallback_share"]["relu"], cell("dot_relu", m), p["dot"] / 1e6, p["difference"] / 1e6, r["same_bits"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--slow-ms", type=float, default=200.0)
    ap.add_argument("--cells", default="all")
    ap.add_argument("--relu-times", action="store_true")
    ap.add_argument("--no-torch", action="store_true", help="skip the two cdist forms")
    ap.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md (cells already in STEM.json are kept)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_dot_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    import hypergef_amd as hg
    dev = torch.device("cuda:0")
    want = None if args.cells == "all" else set(args.cells.split(","))
    g = torch.Generator(device=dev).manual_seed(0)
    res = []
    if args.out and os.path.exists(args.out + ".json"):
        res = json.load(open(args.out + ".json"))["cells"]
    for N in SIZES:
        for F in WIDTHS:
            name = "%dx%d" % (N, F)
            if want is not None and name not in want:
                continue
            X = torch.randn(N, F, device=dev, generator=g)
            R = torch.relu(torch.randn(N, F, device=dev, generator=g) + 0.5)
            forms = {"dot": lambda X=X: hg.ops.knn(X, K, return_mean=True, form="dot"),
                     "difference": lambda X=X: hg.ops.knn(X, K, return_mean=True)}
            if args.relu_times:
                forms["dot_relu"] = lambda R=R: hg.ops.knn(R, K, return_mean=True, form="dot")
            if not args.no_torch:
                forms["cdist_exact"] = lambda X=X: torch.cdist(X, X, compute_mode="donot_use_mm_for_euclid_dist").topk(K, largest=False)
                forms["cdist_mm"] = lambda X=X: torch.cdist(X, X).topk(K, largest=False)
            r = knn_probe.run_cell(name, X, forms, args)
            r.update(N=N, F=F, fallback_share={}, same_bits=True)
            for kind, Y in (("randn", X), ("relu", R)):
                a = hg.ops.knn(Y, K, form="dot", return_fallback=True)
                b = hg.ops.knn(Y, K)
                r["fallback_share"][kind] = round(float(a[2].float().mean()), 6)
                r["same_bits"] = r["same_bits"] and bool(torch.equal(a[0], b[0])) and bool(torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
            res = [c for c in res if c["cell"] != name] + [r]
            print(json.dumps(r), flush=True)
            del X, R, forms
            torch.cuda.empty_cache()
            if args.out:  # after every cell: a run that is cut short keeps what it measured
                order = {"%dx%d" % (n, f): i for i, (n, f) in enumerate((n, f) for n in SIZES for f in WIDTHS)}
                res.sort(key=lambda c: order[c["cell"]])
                with open(args.out + ".json", "w") as f:
                    json.dump({"device": torch.cuda.get_device_name(0), "steps": args.steps, "k": K, "cells": res}, f, indent=1)
                write_md(args.out + ".md", torch.cuda.get_device_name(0), res)


if __name__ == "__main__":
    main()
