"""ops.knn(form="dot_split") against the other searches of float32 rows (GPU only; no GPU is an error).

Per cell and per kind of rows (randn, relu(randn + 0.5)), device ms per call between two events, the forms timed in turn,
three rounds, medians (tools/knn_probe.py's run_cell), and each form's peak allocation above what is live before the call:
    dot_split   ops.knn(X, k, form="dot_split", return_mean=True)      hg_knn_dot_split_f32
    dot         ops.knn(X, k, form="dot", return_mean=True)            hg_knn_dot_f32
    difference  ops.knn(X, k, return_mean=True)                        hg_knn_f32
    bf16_dot    ops.knn(X.bfloat16(), k, form="dot", return_mean=True) another problem (rounded rows): the bf16 unit's pace
    cdist       torch.cdist(X, X).topk(k, largest=False)
Also per cell: the rows that fell back under "dot_split", and whether its idx and dist equal the difference form's.
Then the layer: one training step (forward, backward) of the float32 DynamicHypergraphConv(device_graph=True) at 50000 x 32
and 50000 x 128 under each of the three forms, and the matrix unit against the bound: hg_knn_dot_estimates_split_f32 on the
kinds of tests/_knn_split_ref.py, nq = n = 128, the largest |est - d2_f64| / e1 per kind over the widths.
Cells: N in {2012, 12311, 50000} x F in {64, 128, 256, 1024, 4096}, k = 10.

    python tools/knn_split_probe.py [--steps 5] [--cells 2012x64,...] [--kinds randn,relu] [--no-layer] [--out profiles/r27_knn_split]
"""
import argparse
import ctypes
import json
import os
import statistics
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
WIDTHS = (64, 128, 256, 1024, 4096)
KINDS = ("randn", "relu")
LAYER_CELLS = ((50000, 32), (50000, 128))
LAYER_FORMS = ("dot_split", "dot", "difference")


def bound_ratios(dev):
    """kind -> the largest |est - d2_f64| / e1 over the widths, from the diagnostic entry."""
    import _knn_bf16_ref as br
    import _knn_split_ref as sr
    from hypergef_amd import _lib
    L = _lib.lib()
    out, n = {}, 128
    for kind in sr.KINDS:
        worst = 0.0
        for F in sr.WIDTHS:
            Xn, Qn = sr.rows(kind, n, F, 100 + F), sr.rows(kind, n, F, 200 + F)
            X, Q = torch.from_numpy(Xn).to(dev), torch.from_numpy(Qn).to(dev)
            est, e1 = torch.empty((n, n), device=dev), torch.empty(n, device=dev)
            with torch.cuda.device(dev):
                _lib.check(L.hg_knn_dot_estimates_split_f32(ctypes.c_void_p(Q.data_ptr()), n, ctypes.c_void_p(X.data_ptr()), n, F,
                                                            ctypes.c_void_p(est.data_ptr()), ctypes.c_void_p(e1.data_ptr()),
                                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            err = np.abs(est.double().cpu().numpy() - br.distances(Qn, Xn))
            worst = max(worst, float((err / e1.double().cpu().numpy()[:, None]).max()))
        out[kind] = round(worst, 6)
    return out


def layer_steps(hg, dev, steps):
    """cell -> form -> device ms of one forward and backward, medians of three rounds."""
    out = {}
    for N, F in LAYER_CELLS:
        X = torch.randn(N, F, device=dev)
        G = torch.randn(N, F, device=dev)
        out["%dx%d" % (N, F)] = row = {}
        for form in LAYER_FORMS:
            torch.manual_seed(5)
            layer = hg.DynamicHypergraphConv(F, F, K, device_graph=True, knn_form=form).to(dev)

            def step(layer=layer):
                layer.lin.weight.grad = None
                layer(X).backward(G)
            step()
            row[form] = round(statistics.median(knn_probe.device_ms(step, steps, 1) for _ in range(3)), 4)
    return out


def write_md(path, device, res, ratios, layer):
    with open(path, "w") as f:
        f.write("# ops.knn(form=\"dot_split\") against the other searches of float32 rows (tools/knn_split_probe.py, %s, k = %d, "
                "medians of 3 rounds)\n\n" % (device, K))
        f.write("Device ms per call, `return_mean` on; peak allocation above the live set, MB.  `bf16 dot` searches the rows "
                "rounded to bfloat16 (another problem: the bf16 unit's pace, the conversion included).  **Bold**: `dot_split` is "
                "slower than the faster of `dot` and `difference`.\n\n")
        f.write("| rows | cell | dot_split ms | dot ms | difference ms | bf16 dot ms | cdist + topk ms | rows fallen back | dot_split peak | "
                "dot peak | difference peak | cdist peak | same idx, dist |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in res:
            m, p = r["ms"], r["peak_bytes"]

            def cell(form, table, scale=1.0, fmt="%.3f"):
                return fmt % (table[form] * scale) if form in table else r["note"].get(form, "-")
            new = "%.3f" % m["dot_split"]
            if m["dot_split"] > min(m["dot"], m["difference"]):
                new = "**%s**" % new
            f.write("| %s | %s | %s | %.3f | %.3f | %s | %s | %d | %.2f | %.2f | %.2f | %s | %s |\n" % (
                r["kind"], r["cell"], new, m["dot"], m["difference"], cell("bf16_dot", m), cell("cdist", m), r["fallback_rows"],
                p["dot_split"] / 1e6, p["dot"] / 1e6, p["difference"] / 1e6, cell("cdist", p, 1e-6, "%.2f"), r["same_bits"]))
        if layer:
            f.write("\nOne training step (forward, backward) of the float32 `DynamicHypergraphConv(device_graph=True)`, device ms.\n\n"
                    "| cell | dot_split | dot | difference |\n|---|---|---|---|\n")
            for name, row in layer.items():
                f.write("| %s | %.3f | %.3f | %.3f |\n" % (name, row["dot_split"], row["dot"], row["difference"]))
        if ratios:
            f.write("\nThe matrix unit against the bound (hg_knn_dot_estimates_split_f32, nq = n = 128): the largest "
                    "|est - d2_f64| / e1 per kind of row over the widths of tests/_knn_split_ref.py.\n\n| kind | max err / e1 |\n|---|---|\n")
            for kind, v in ratios.items():
                f.write("| %s | %.4g |\n" % (kind, v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--slow-ms", type=float, default=200.0)
    ap.add_argument("--cells", default="all")
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--no-torch", action="store_true", help="skip the cdist form")
    ap.add_argument("--no-layer", action="store_true", help="skip the layer steps")
    ap.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md (cells already in STEM.json are kept)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_split_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    import hypergef_amd as hg
    dev = torch.device("cuda:0")
    name_dev = torch.cuda.get_device_name(0)
    want = None if args.cells == "all" else set(args.cells.split(","))
    g = torch.Generator(device=dev).manual_seed(0)
    res, ratios, layer = [], {}, {}
    if args.out and os.path.exists(args.out + ".json"):
        old = json.load(open(args.out + ".json"))
        res, layer = old["cells"], old.get("layer_step_ms", {})

    def save():
        if args.out:
            order = {"%dx%d" % (n, f): i for i, (n, f) in enumerate((n, f) for n in SIZES for f in WIDTHS)}
            res.sort(key=lambda c: (c["kind"], order[c["cell"]]))
            with open(args.out + ".json", "w") as f:
                json.dump({"device": name_dev, "steps": args.steps, "k": K, "cells": res, "layer_step_ms": layer,
                           "bound_ratios": ratios}, f, indent=1)
            write_md(args.out + ".md", name_dev, res, ratios, layer)

    ratios = bound_ratios(dev)
    print(json.dumps({"bound_ratios": ratios}), flush=True)
    save()
    if not args.no_layer:
        layer = layer_steps(hg, dev, args.steps)
        print(json.dumps({"layer_step_ms": layer}), flush=True)
        save()
    for kind in args.kinds.split(","):
        for N in SIZES:
            for F in WIDTHS:
                name = "%dx%d" % (N, F)
                if want is not None and name not in want:
                    continue
                X = torch.randn(N, F, device=dev, generator=g)
                if kind == "relu":
                    X = torch.relu(X + 0.5)
                forms = {"dot_split": lambda X=X: hg.ops.knn(X, K, return_mean=True, form="dot_split"),
                         "dot": lambda X=X: hg.ops.knn(X, K, return_mean=True, form="dot"),
                         "difference": lambda X=X: hg.ops.knn(X, K, return_mean=True),
                         "bf16_dot": lambda X=X: hg.ops.knn(X.bfloat16(), K, return_mean=True, form="dot")}
                if not args.no_torch:
                    forms["cdist"] = lambda X=X: torch.cdist(X, X).topk(K, largest=False)
                r = knn_probe.run_cell(name, X, forms, args)
                a = hg.ops.knn(X, K, form="dot_split", return_fallback=True)
                b = hg.ops.knn(X, K)
                r.update(kind=kind, N=N, F=F, fallback_rows=int(a[2].sum()),
                         same_bits=bool(torch.equal(a[0], b[0])) and bool(torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))))
                res = [c for c in res if (c["cell"], c["kind"]) != (name, kind)] + [r]
                print(json.dumps(r), flush=True)
                del X, forms, a, b
                torch.cuda.empty_cache()
                save()  # after every cell: a run that is cut short keeps what it measured


if __name__ == "__main__":
    main()
