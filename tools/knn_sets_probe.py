"""ops.knn(set_rows=m) -- B point sets of m rows in one tensor -- against what a batch had to do before it (GPU only; no GPU
is an error).

Per cell and k, device ms per call between two events, the forms timed in turn, three rounds, medians (tools/knn_probe.py's
run_cell), and each form's peak allocation above what is live before the call:
    sets_difference   ops.knn(X, k, set_rows=m, return_mean=True)                          hg_knn_sets_f32
    sets_dot          ops.knn(X, k, set_rows=m, form="dot", return_mean=True)              hg_knn_dot_sets_f32
    sets_dot_bf16     ops.knn(Xb, k, set_rows=m, form="dot", return_mean=True)             hg_knn_dot_sets_bf16
    segments          ops.knn(X, k, segments=range(0, n + 1, m), return_mean=True)         the call before set_rows; it waits once
    widen_segments    ops.knn(Xb.float(), k, segments=..., return_mean=True)               what bfloat16 rows had to do
    cdist             torch.cdist(X.view(B, m, F), X.view(B, m, F)).topk(k, largest=False)
X is randn, Xb = X rounded to bfloat16.  Also per cell: the rows that fell back under "dot", and whether every set_rows form
returns the segments call's idx and dist.  Then one training step (forward, backward) of
DynamicHypergraphConv(F, F, k=10, set_rows=m) with device_graph=False, device_graph=True run eagerly, and device_graph=True
recorded by torch.cuda.graph and replayed.
Cells B x m x F: 32 x 1024 x {64, 256, 1024}, 8 x 4096 x {64, 256}, 1024 x 32 x 64 (every set a partly empty 128-row tile).

    python tools/knn_sets_probe.py [--steps 5] [--cells 32x1024x64,...] [--out profiles/r25_knn_sets]
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

KS = (10, 20)
CELLS = ((32, 1024, 64), (32, 1024, 256), (32, 1024, 1024), (8, 4096, 64), (8, 4096, 256), (1024, 32, 64))
NEW = ("sets_difference", "sets_dot", "sets_dot_bf16")
OLD = {"sets_difference": ("segments", "cdist"), "sets_dot": ("segments", "cdist"), "sets_dot_bf16": ("widen_segments", "cdist")}
MODES = ("planned", "device_eager", "device_captured")


def layer_steps(hg, X, m, args):
    """ms of one training step per mode of the layer (k = 10, knn_form="difference")."""
    F = X.shape[1]
    G = torch.randn_like(X)
    fns = {}
    for mode in MODES:
        torch.manual_seed(0)
        layer = hg.DynamicHypergraphConv(F, F, 10, device_graph=mode != "planned", set_rows=m).to(X.device)

        def step(layer=layer):
            layer.lin.weight.grad = None
            layer(X).backward(G)
        if mode == "device_captured":
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            fns[mode] = graph.replay
        else:
            fns[mode] = step
    return knn_probe.run_cell("layer", X, fns, args)["ms"]


def write_md(path, device, res):
    with open(path, "w") as f:
        f.write("# ops.knn(set_rows=) on batches of equal point sets (tools/knn_sets_probe.py, %s, medians of 3 rounds)\n\n" % device)
        f.write("Device ms per call, randn rows; `widen + segments` includes `Xb.float()`; peak allocation above the live set, "
                "MB, in brackets.  **Bold**: the set_rows form is slower than `segments` (for bfloat16 rows: `widen + segments`) "
                "or than `cdist + topk`.\n\n")
        f.write("| B x m x F | k | sets difference | sets dot | sets dot bf16 | segments | widen + segments | cdist + topk | "
                "rows fallen back (dot, bf16) | same idx, dist |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in res:
            m, p = r["ms"], r["peak_bytes"]

            def cell(form):
                if form not in m:
                    return r["note"].get(form, "-")
                s = "%.3f" % m[form]
                if form in OLD and any(o in m and m[form] > m[o] for o in OLD[form]):
                    s = "**%s**" % s
                return "%s (%.1f)" % (s, p[form] / 1e6)
            f.write("| %s | %d | %s | %s | %s | %s | %s | %s | %d, %d | %s |\n" % (
                (r["cell"], r["k"]) + tuple(cell(x) for x in NEW + ("segments", "widen_segments", "cdist")) +
                (r["fallback_rows"][0], r["fallback_rows"][1], r["same_bits"])))
        f.write("\nOne training step of `DynamicHypergraphConv(F, F, 10, set_rows=m)`, float32, `knn_form=\"difference\"`, ms.  "
                "**Bold**: slower than `device_graph=False`.\n\n| B x m x F | device_graph=False | device_graph=True, eager | "
                "device_graph=True, captured |\n|---|---|---|---|\n")
        for r in res:
            if "layer_ms" in r:
                s = r["layer_ms"]
                f.write("| %s | %.3f | %s | %s |\n" % ((r["cell"], s["planned"]) + tuple(
                    ("**%.3f**" if s[x] > s["planned"] else "%.3f") % s[x] for x in MODES[1:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--slow-ms", type=float, default=200.0)
    ap.add_argument("--cells", default="all")
    ap.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md (cells already in STEM.json are kept)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_sets_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    import hypergef_amd as hg
    dev = torch.device("cuda:0")
    name_dev = torch.cuda.get_device_name(0)
    want = None if args.cells == "all" else set(args.cells.split(","))
    g = torch.Generator(device=dev).manual_seed(0)
    res = []
    if args.out and os.path.exists(args.out + ".json"):
        res = json.load(open(args.out + ".json"))["cells"]

    def save():
        if args.out:
            order = {"%dx%dx%d" % c: i for i, c in enumerate(CELLS)}
            res.sort(key=lambda c: (order[c["cell"]], c["k"]))
            with open(args.out + ".json", "w") as f:
                json.dump({"device": name_dev, "steps": args.steps, "cells": res}, f, indent=1)
            write_md(args.out + ".md", name_dev, res)

    for B, m, F in CELLS:
        name = "%dx%dx%d" % (B, m, F)
        if want is not None and name not in want:
            continue
        n = B * m
        X = torch.randn(n, F, device=dev, generator=g)
        Xb = X.bfloat16()
        seg = list(range(0, n + 1, m))
        for k in KS:
            kw = dict(return_mean=True)
            forms = {"sets_difference": lambda: hg.ops.knn(X, k, set_rows=m, **kw),
                     "sets_dot": lambda: hg.ops.knn(X, k, set_rows=m, form="dot", **kw),
                     "sets_dot_bf16": lambda: hg.ops.knn(Xb, k, set_rows=m, form="dot", **kw),
                     "segments": lambda: hg.ops.knn(X, k, segments=seg, **kw),
                     "widen_segments": lambda: hg.ops.knn(Xb.float(), k, segments=seg, **kw),
                     "cdist": lambda: torch.cdist(X.view(B, m, F), X.view(B, m, F)).topk(k, largest=False)}
            r = knn_probe.run_cell(name, X, forms, args)
            old, oldb = hg.ops.knn(X, k, segments=seg), hg.ops.knn(Xb.float(), k, segments=seg)
            a = hg.ops.knn(X, k, set_rows=m)
            b = hg.ops.knn(X, k, set_rows=m, form="dot", return_fallback=True)
            c = hg.ops.knn(Xb, k, set_rows=m, form="dot", return_fallback=True)
            same = all(torch.equal(u[0], v[0]) and torch.equal(u[1].view(torch.int32), v[1].view(torch.int32))
                       for u, v in ((a, old), (b, old), (c, oldb)))
            r.update(k=k, B=B, m=m, F=F, fallback_rows=[int(b[2].sum()), int(c[2].sum())], same_bits=bool(same))
            if k == 10:
                r["layer_ms"] = layer_steps(hg, X, m, args)
            res = [x for x in res if (x["cell"], x["k"]) != (name, k)] + [r]
            print(json.dumps(r), flush=True)
            del forms, old, oldb, a, b, c
            torch.cuda.empty_cache()
            save()  # after every cell: a run that is cut short keeps what it measured
        del X, Xb


if __name__ == "__main__":
    main()
