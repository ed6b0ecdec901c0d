"""ops.knn(form="dot") on bfloat16 rows against what a bfloat16 user had to do before it (GPU only; no GPU is an error).

Per cell, device ms per call between two events, the forms timed in turn, three rounds, medians (tools/knn_probe.py's
run_cell), and each form's peak allocation above what is live before the call:
    bf16_dot          ops.knn(Xb, k, form="dot", return_mean=True)                      hg_knn_dot_bf16
    widen_dot         ops.knn(Xb.float(), k, form="dot", return_mean=True)              the widening included
    widen_difference  ops.knn(Xb.float(), k, return_mean=True)                          likewise
    cdist             torch.cdist(Xb.float(), Xb.float()).topk(k, largest=False)
Xb is randn rounded to bfloat16.  Also per cell: the rows that fell back, and whether idx and dist equal the float32
difference form's.  Then the matrix unit against the bound: hg_knn_dot_estimates_bf16 on the adversarial kinds of
tests/_knn_bf16_ref.py, nq = n = 128, the largest |est - d2_f64| / e1 per kind over the widths.
Cells: N in {2012, 12311, 50000} x F in {64, 256, 1024, 4096}, k = 10.

    python tools/knn_bf16_probe.py [--steps 5] [--cells 2012x64,...] [--out profiles/r20_knn_bf16]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import knn_probe  # noqa: E402

K = 10
SIZES = (2012, 12311, 50000)
WIDTHS = (64, 256, 1024, 4096)
FORMS = ("bf16_dot", "widen_dot", "widen_difference", "cdist")
ERR_WIDTHS = (1, 15, 16, 17, 33, 1024, 4096)


def bound_ratios(dev):
    """kind -> the largest |est - d2_f64| / e1 over ERR_WIDTHS, from the diagnostic entry."""
    import _knn_bf16_ref as br
    from hypergef_amd import _lib
    L = _lib.lib()
    out = {}
    n = 128
    for kind in br.KINDS:
        worst = 0.0
        for F in ERR_WIDTHS:
            X, Q = br.rows(kind, n, F, 100 + F), br.rows(kind, n, F, 200 + F)
            Xb, Qb = torch.from_numpy(X).to(dev).bfloat16(), torch.from_numpy(Q).to(dev).bfloat16()
            est, e1 = torch.empty((n, n), device=dev), torch.empty(n, device=dev)
            with torch.cuda.device(dev):
                _lib.check(L.hg_knn_dot_estimates_bf16(ctypes.c_void_p(Qb.data_ptr()), n, ctypes.c_void_p(Xb.data_ptr()), n, F,
                                                       ctypes.c_void_p(est.data_ptr()), ctypes.c_void_p(e1.data_ptr()),
                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            err = np.abs(est.double().cpu().numpy() - br.distances(Q, X))
            worst = max(worst, float((err / e1.double().cpu().numpy()[:, None]).max()))
        out[kind] = round(worst, 6)
    return out


def write_md(path, device, res, ratios):
    with open(path, "w") as f:
        f.write("# ops.knn(form=\"dot\") on bfloat16 rows against widening first (tools/knn_bf16_probe.py, %s, k = %d, medians of 3 "
                "rounds)\n\n" % (device, K))
        f.write("Device ms per call, randn rows rounded to bfloat16; the `widen` columns include `Xb.float()`; peak allocation "
                "above the live set, MB.  **Bold**: `bf16 dot` is slower than the faster of the two widened searches.  Every width "
                "here is a multiple of 8 on an aligned base, so every cell takes the 16-byte loads: the element-by-element path "
                "of rows that are not 16-byte aligned is not measured.\n\n")
        f.write("| cell | bf16 dot ms | widen + dot ms | widen + difference ms | cdist + topk ms | rows fallen back | bf16 dot peak | "
                "widen + dot peak | widen + difference peak | cdist peak | same idx, dist |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in res:
            m, p = r["ms"], r["peak_bytes"]

            def cell(form, table, scale=1.0, fmt="%.3f"):
                return fmt % (table[form] * scale) if form in table else r["note"].get(form, "-")
            new = "%.3f" % m["bf16_dot"]
            if m["bf16_dot"] > min(m["widen_dot"], m["widen_difference"]):
                new = "**%s**" % new
            f.write("| %s | %s | %.3f | %.3f | %s | %d | %.2f | %.2f | %.2f | %s | %s |\n" % (
                r["cell"], new, m["widen_dot"], m["widen_difference"], cell("cdist", m), r["fallback_rows"], p["bf16_dot"] / 1e6,
                p["widen_dot"] / 1e6, p["widen_difference"] / 1e6, cell("cdist", p, 1e-6, "%.2f"), r["same_bits"]))
        if ratios:
            f.write("\nThe matrix unit against the bound (hg_knn_dot_estimates_bf16, nq = n = 128, widths %s): the largest "
                    "|est - d2_f64| / e1 per kind of row.\n\n| kind | max err / e1 |\n|---|---|\n" % ", ".join(map(str, ERR_WIDTHS)))
            for kind, v in ratios.items():
                f.write("| %s | %.4g |\n" % (kind, v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--slow-ms", type=float, default=200.0)
    ap.add_argument("--cells", default="all")
    ap.add_argument("--no-torch", action="store_true", help="skip the cdist form")
    ap.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md (cells already in STEM.json are kept)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_bf16_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    import hypergef_amd as hg
    dev = torch.device("cuda:0")
    name_dev = torch.cuda.get_device_name(0)
    want = None if args.cells == "all" else set(args.cells.split(","))
    g = torch.Generator(device=dev).manual_seed(0)
    res, ratios = [], {}
    if args.out and os.path.exists(args.out + ".json"):
        res = json.load(open(args.out + ".json"))["cells"]

    def save():
        if args.out:
            order = {"%dx%d" % (n, f): i for i, (n, f) in enumerate((n, f) for n in SIZES for f in WIDTHS)}
            res.sort(key=lambda c: order[c["cell"]])
            with open(args.out + ".json", "w") as f:
                json.dump({"device": name_dev, "steps": args.steps, "k": K, "cells": res, "bound_ratios": ratios}, f, indent=1)
            write_md(args.out + ".md", name_dev, res, ratios)

    ratios = bound_ratios(dev)
    print(json.dumps({"bound_ratios": ratios}), flush=True)
    save()
    for N in SIZES:
        for F in WIDTHS:
            name = "%dx%d" % (N, F)
            if want is not None and name not in want:
                continue
            Xb = torch.randn(N, F, device=dev, generator=g).bfloat16()
            forms = {"bf16_dot": lambda Xb=Xb: hg.ops.knn(Xb, K, return_mean=True, form="dot"),
                     "widen_dot": lambda Xb=Xb: hg.ops.knn(Xb.float(), K, return_mean=True, form="dot"),
                     "widen_difference": lambda Xb=Xb: hg.ops.knn(Xb.float(), K, return_mean=True)}
            if not args.no_torch:
                forms["cdist"] = lambda Xb=Xb: torch.cdist(Xb.float(), Xb.float()).topk(K, largest=False)
            r = knn_probe.run_cell(name, Xb, forms, args)
            a = hg.ops.knn(Xb, K, form="dot", return_fallback=True)
            b = hg.ops.knn(Xb.float(), K)
            r.update(N=N, F=F, fallback_rows=int(a[2].sum()),
                     same_bits=bool(torch.equal(a[0], b[0])) and bool(torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))))
            res = [c for c in res if c["cell"] != name] + [r]
            print(json.dumps(r), flush=True)
            del Xb, forms, a, b
            torch.cuda.empty_cache()
            save()  # after every cell: a run that is cut short keeps what it measured


if __name__ == "__main__":
    main()
