"""The table kernels on bfloat16 rows against what a bfloat16 model had to do before them (GPU only; no GPU is an error).

Per cell, device ms per call between two events, the forms timed in turn, three rounds, medians (tools/knn_probe.py's
run_cell).  Per kernel -- hop 0, hop 1, dist, the two difference gathers, the dot -- three forms:
    bf16    the hg_table_*_bf16 entry on bfloat16 rows
    widen   what a bfloat16 model did before: widen the rows, the float32 entry, round where the result is bfloat16
    f32     the float32 entry on float32 rows (no conversion)
and a bytes floor: the bytes the bf16 call must move (gathered rows, centre rows, result, table, weights) over the HBM peak.
Per layer, one training step (forward, backward) of DynamicHypergraphConv(F, F, k, probabilistic=True, knn_form="dot"):
    bf16_device   the bfloat16 layer, device_graph=True
    bf16_host     the bfloat16 layer, device_graph=False (the host plan)
    f32_device    the float32 layer, device_graph=True
The table is ops.knn's own (k = 10, self first) on randn rows rounded to bfloat16.
Cells: N in {2708, 12311, 50000} x F in {32, 128}.

    python tools/table_bf16_probe.py [--steps 200] [--cells 2708x32,...] [--no-layer] [--out profiles/r21_table_bf16]
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
SIZES = (2708, 12311, 50000)
WIDTHS = (32, 128)
KERNELS = ("hop0", "hop1", "dist", "diff", "diff_t", "dot")
LAYERS = ("bf16_device", "bf16_host", "f32_device")
HBM_PEAK = 8.0e12  # bytes / s, MI355X
BF = torch.bfloat16


def kernel_forms(hg, Xb, dYb):
    """kernel -> {form -> callable}, and kernel -> the bytes of the bf16 call."""
    kg = hg.knn_graph
    N, F = Xb.shape
    dev = Xb.device
    idx = hg.ops.knn(Xb, K, form="dot")[0]
    ptr_v, pos_v = hg.ops.knn_transpose(idx, N)
    gen = torch.Generator(device=dev).manual_seed(1)
    w = torch.rand(N * K, device=dev, generator=gen) + 0.5
    degE, degV = (torch.rand(N, device=dev, generator=gen) + 0.5 for _ in range(2))
    Xf, dYf = Xb.float(), dYb.float()
    Xe = kg.table_gather(idx, Xf, w, None, degE)
    G = kg.table_gather(idx, dYf, w, degV, degE)
    rows = hg.ops.current_options().replace(incidence_bf16="rows")
    forms = {
        "hop0": {"bf16": lambda: kg.table_gather(idx, Xb, w, None, degE),
                 "widen": lambda: kg.table_gather(idx, Xb.float(), w, None, degE),
                 "f32": lambda: kg.table_gather(idx, Xf, w, None, degE)},
        "hop1": {"bf16": lambda: kg.table_gather_t(ptr_v, pos_v, K, Xe, w, None, degV, dst_dtype=BF),
                 "widen": lambda: kg.table_gather_t(ptr_v, pos_v, K, Xe, w, None, degV).to(BF),
                 "f32": lambda: kg.table_gather_t(ptr_v, pos_v, K, Xe, w, None, degV)},
        "dist": {"bf16": lambda: hg.ops.knn_dist(idx, Xb, options=rows),
                 "widen": lambda: hg.ops.knn_dist(idx, Xb.float()),
                 "f32": lambda: hg.ops.knn_dist(idx, Xf)},
        "diff": {"bf16": lambda: kg.table_gather(idx, Xb, w, ctr=Xb),
                 "widen": lambda: (lambda x: kg.table_gather(idx, x, w, ctr=x))(Xb.float()),
                 "f32": lambda: kg.table_gather(idx, Xf, w, ctr=Xf)},
        "diff_t": {"bf16": lambda: kg.table_gather_t(ptr_v, pos_v, K, Xb, w, ctr=Xb),
                   "widen": lambda: (lambda x: kg.table_gather_t(ptr_v, pos_v, K, x, w, ctr=x))(Xb.float()),
                   "f32": lambda: kg.table_gather_t(ptr_v, pos_v, K, Xf, w, ctr=Xf)},
        "dot": {"bf16": lambda: kg.table_dot(idx, dYb, Xe, degV, Xb, G),
                "widen": lambda: kg.table_dot(idx, dYb.float(), Xe, degV, Xb.float(), G),
                "f32": lambda: kg.table_dot(idx, dYf, Xe, degV, Xf, G)},
    }
    e, r = N * K, N * F
    table = e * 8  # a position's index and weight
    nbytes = {"hop0": e * F * 2 + r * 4 + table + N * 4, "hop1": e * F * 4 + r * 2 + table + e * 4 + N * 8,
              "dist": e * F * 2 + r * 2 + e * 8, "diff": e * F * 2 + r * 2 + r * 4 + table,
              "diff_t": e * F * 2 + r * 2 + r * 4 + table + e * 4 + N * 4, "dot": e * F * 4 + r * 8 + table + N * 4}
    return forms, nbytes


def layer_forms(hg, Xb):
    F = Xb.shape[1]
    out = {}
    for name, dtype, device_graph in (("bf16_device", BF, True), ("bf16_host", BF, False), ("f32_device", torch.float32, True)):
        torch.manual_seed(0)
        layer = hg.DynamicHypergraphConv(F, F, K, probabilistic=True, device_graph=device_graph, knn_form="dot").to(Xb.device).to(dtype)
        X = Xb.to(dtype).clone().requires_grad_(True)

        def step(layer=layer, X=X):
            X.grad = None
            layer.zero_grad(set_to_none=True)
            layer(X).float().sum().backward()
        out[name] = step
    return out


def write_md(path, device, steps, res):
    def bold(v, lost):
        return ("**%.4f**" if lost else "%.4f") % v

    with open(path, "w") as f:
        f.write("# The table kernels on bfloat16 rows (tools/table_bf16_probe.py, %s, k = %d, %d steps a round, medians of 3 "
                "rounds)\n\n" % (device, K, steps))
        f.write("Device ms per call.  `widen`: the rows widened, the float32 entry, the result rounded where it is bfloat16 -- what "
                "a bfloat16 model did before.  `f32`: the float32 entry on float32 rows.  floor: the bf16 call's bytes over %.0f "
                "TB/s.  **Bold**: the bf16 entry is slower than that comparison.\n\n" % (HBM_PEAK / 1e12))
        f.write("| cell | kernel | bf16 ms | widen ms | f32 ms | floor ms | bf16 / floor |\n|---|---|---|---|---|---|---|\n")
        for r in res:
            for kern in KERNELS:
                m = r.get("kernels", {}).get(kern)
                if m:
                    f.write("| %s | %s | %.4f | %s | %s | %.4f | %.1f |\n" % (
                        r["cell"], kern, m["bf16"], bold(m["widen"], m["bf16"] > m["widen"]), bold(m["f32"], m["bf16"] > m["f32"]),
                        m["floor"], m["bf16"] / m["floor"]))
        f.write("\nOne training step of `DynamicHypergraphConv(F, F, %d, probabilistic=True, knn_form=\"dot\")`, device ms.  "
                "**Bold**: the bfloat16 `device_graph=True` layer is slower than that comparison.\n\n" % K)
        f.write("| cell | bf16 device_graph=True | bf16 device_graph=False | f32 device_graph=True |\n|---|---|---|---|\n")
        for r in res:
            m = r.get("layer")
            if m:
                f.write("| %s | %.3f | %s | %s |\n" % (r["cell"], m["bf16_device"], bold(m["bf16_host"], m["bf16_device"] > m["bf16_host"]),
                                                      bold(m["f32_device"], m["bf16_device"] > m["f32_device"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="calls a round per kernel form; a tenth of it per layer form")
    ap.add_argument("--slow-ms", type=float, default=200.0)
    ap.add_argument("--cells", default="all")
    ap.add_argument("--no-layer", action="store_true", help="skip the layer's training step")
    ap.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md (cells already in STEM.json are kept)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("table_bf16_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    import hypergef_amd as hg
    dev = torch.device("cuda:0")
    name_dev = torch.cuda.get_device_name(0)
    want = None if args.cells == "all" else set(args.cells.split(","))
    res = []
    if args.out and os.path.exists(args.out + ".json"):
        res = json.load(open(args.out + ".json"))["cells"]

    def save():
        if args.out:
            order = {"%dx%d" % (n, f): i for i, (n, f) in enumerate((n, f) for n in SIZES for f in WIDTHS)}
            res.sort(key=lambda c: order[c["cell"]])
            with open(args.out + ".json", "w") as f:
                json.dump({"device": name_dev, "steps": args.steps, "k": K, "cells": res}, f, indent=1)
            write_md(args.out + ".md", name_dev, args.steps, res)

    gen = torch.Generator(device=dev).manual_seed(0)
    for N in SIZES:
        for F in WIDTHS:
            name = "%dx%d" % (N, F)
            if want is not None and name not in want:
                continue
            Xb = torch.randn(N, F, device=dev, generator=gen).to(BF)
            dYb = torch.randn(N, F, device=dev, generator=gen).to(BF)
            r = {"cell": name, "N": N, "F": F, "kernels": {}}
            with torch.no_grad():
                forms, nbytes = kernel_forms(hg, Xb, dYb)
                for kern in KERNELS:
                    m = knn_probe.run_cell(name, Xb, forms[kern], args)["ms"]
                    m["floor"] = round(nbytes[kern] / HBM_PEAK * 1e3, 5)
                    r["kernels"][kern] = m
                del forms
            if not args.no_layer:
                few = argparse.Namespace(steps=max(args.steps // 10, 3), slow_ms=args.slow_ms)  # a step is many launches
                r["layer"] = knn_probe.run_cell(name, Xb, layer_forms(hg, Xb), few)["ms"]
            res = [c for c in res if c["cell"] != name] + [r]
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
            save()  # after every cell: a run that is cut short keeps what it measured


if __name__ == "__main__":
    main()
