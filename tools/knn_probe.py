"""ops.knn against the two torch forms a user writes today (GPU only; no GPU is an error).

Per cell, device ms per call between two events (bench.timed_steps), the candidates timed in turn, three rounds, medians;
and each form's peak allocation above what is live before the call (torch.cuda.max_memory_allocated):
    knn          ops.knn(X, k)                                                   hg_knn_f32, cand_slices = 0
    knn_best     the fastest of cand_slices in {1, 2, 4, 8, 16} (reported with its count)
    cdist_exact  torch.cdist(X, X, compute_mode="donot_use_mm_for_euclid_dist").topk(k, largest=False)
                 the form with the same arithmetic (differences, then the root)
    cdist_mm     torch.cdist(X, X).topk(k, largest=False)                        torch's default: |x|^2 + |y|^2 - 2 x.y
Cells: N in {2708, 12311, 50000} x F in {64, 1024}, k = 10, X randn; and 1024 point sets of 2708 rows (the cora shape) in
one tensor at F = 32 -- ops.knn(segments=...) against the batched cdist on [1024, 2708, 32].  Where a torch form cannot
allocate, the cell says so instead of a time.  A form whose single call takes longer than --slow-ms is timed once per
round, not --steps times; one that takes twenty times that is timed once.

    python tools/knn_probe.py [--steps 10] [--cells 2708x64,...] [--out profiles/r16_knn]
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

K = 10
SIZES = (2708, 12311, 50000)
WIDTHS = (64, 1024)
BATCH = (1024, 2708, 32)
SLICES = (1, 2, 4, 8, 16)


def device_ms(fn, steps, warmup):
    import bench
    for _ in range(warmup):
        fn()
    _, dev_s = bench.timed_steps(fn, steps, torch.cuda.synchronize, lambda: None)
    return dev_s / steps * 1e3


def first_call(fn):
    """(ms of one call, peak bytes above the live set) or (None, the refusal) where it cannot allocate."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    try:
        fn()  # the first call may build caches: not timed
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        return device_ms(fn, 1, 0), peak
    except torch.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return None, "cannot allocate: " + str(e).split("\n")[0][:160]


def run_cell(name, X, forms, args):
    """forms: name -> callable.  Times every form that can allocate; three rounds in turn."""
    out = {"cell": name, "k": K, "ms_runs": {}, "ms": {}, "peak_bytes": {}, "note": {}}
    live = {}
    for f, fn in forms.items():
        one, peak = first_call(fn)
        if one is None:
            out["note"][f] = peak
            continue
        out["peak_bytes"][f] = int(peak)
        if one > 20 * args.slow_ms:  # seconds per call: that one call is the figure
            out["ms_runs"][f], out["ms"][f] = [round(one, 4)], round(one, 4)
            continue
        live[f] = (fn, 1 if one > args.slow_ms else args.steps)
        out["ms_runs"][f] = []
    for _ in range(3):
        for f, (fn, steps) in live.items():
            out["ms_runs"][f].append(round(device_ms(fn, steps, 1 if steps > 1 else 0), 4))
    for f in live:
        out["ms"][f] = round(statistics.median(out["ms_runs"][f]), 4)
    return out


def knn_forms(hg, X, segments=None):
    forms = {"knn": lambda: hg.ops.knn(X, K, segments=segments, return_mean=True)}
    for cs in SLICES:
        forms["knn_slices_%d" % cs] = (lambda cs=cs: hg.ops.knn(X, K, segments=segments, return_mean=True, cand_slices=cs))
    return forms


def agreement(hg, X, Xb=None):
    """How many rows' neighbour sets ops.knn and the exact cdist form share (ties and the last bits aside they are the same)."""
    idx = hg.ops.knn(X, K, self_first=False)[0].long()
    ref = torch.cdist(X, X, compute_mode="donot_use_mm_for_euclid_dist").topk(K, largest=False).indices
    same = (idx.sort(1).values == ref.sort(1).values).all(1).float().mean()
    return round(float(same), 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--slow-ms", type=float, default=200.0)
    ap.add_argument("--cells", default="all")
    ap.add_argument("--out", default=None, help="path stem: writes STEM.json and STEM.md")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    import hypergef_amd as hg
    dev = torch.device("cuda:0")
    want = None if args.cells == "all" else set(args.cells.split(","))
    g = torch.Generator(device=dev).manual_seed(0)
    res = []
    for N in SIZES:
        for F in WIDTHS:
            name = "%dx%d" % (N, F)
            if want is not None and name not in want:
                continue
            X = torch.randn(N, F, device=dev, generator=g)
            forms = knn_forms(hg, X)
            forms["cdist_exact"] = lambda X=X: torch.cdist(X, X, compute_mode="donot_use_mm_for_euclid_dist").topk(K, largest=False)
            forms["cdist_mm"] = lambda X=X: torch.cdist(X, X).topk(K, largest=False)
            r = run_cell(name, X, forms, args)
            r.update(N=N, F=F, matrix_bytes=4 * N * N)
            if N <= 12311:
                r["rows_with_the_same_neighbours_as_cdist_exact"] = agreement(hg, X)
            res.append(r)
            print(json.dumps(r), flush=True)
            del X, forms
            torch.cuda.empty_cache()
    name = "%dx%dx%d" % BATCH
    if want is None or name in want:
        B, n, F = BATCH
        X = torch.randn(B * n, F, device=dev, generator=g)
        seg = list(range(0, B * n + 1, n))
        forms = knn_forms(hg, X, seg)
        Xb = X.view(B, n, F)
        forms["cdist_exact"] = lambda: torch.cdist(Xb, Xb, compute_mode="donot_use_mm_for_euclid_dist").topk(K, largest=False)
        forms["cdist_mm"] = lambda: torch.cdist(Xb, Xb).topk(K, largest=False)
        r = run_cell(name, X, forms, args)
        r.update(N=B * n, F=F, segments=B, matrix_bytes=4 * B * n * n)
        res.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out + ".json", "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": args.steps, "k": K, "cells": res}, f, indent=1)
        with open(args.out + ".md", "w") as f:
            f.write("# ops.knn against torch.cdist + topk (tools/knn_probe.py, %s, k = %d, medians of 3 rounds)\n\n"
                    % (torch.cuda.get_device_name(0), K))
            f.write("Device ms per call and peak allocation above the live set.  `knn`: cand_slices = 0; `best`: the fastest of "
                    "cand_slices in %s.  `cdist exact`: compute_mode=donot_use_mm_for_euclid_dist (the same arithmetic); "
                    "`cdist mm`: torch's default.\n\n" % (SLICES,))
            f.write("| cell | knn ms | best ms (slices) | cdist exact ms | cdist mm ms | knn peak MB | cdist exact peak MB | "
                    "cdist mm peak MB |\n|---|---|---|---|---|---|---|---|\n")
            for r in res:
                m, p = r["ms"], r["peak_bytes"]
                best = min((m[k], k) for k in m if k.startswith("knn_slices_"))

                def cell(form, table, scale=1.0, fmt="%.3f"):
                    return fmt % (table[form] * scale) if form in table else r["note"].get(form, "-")
                f.write("| %s | %.3f | %.3f (%s) | %s | %s | %.2f | %s | %s |\n" % (
                    r["cell"], m["knn"], best[0], best[1].rsplit("_", 1)[1], cell("cdist_exact", m), cell("cdist_mm", m),
                    p["knn"] / 1e6, cell("cdist_exact", p, 1e-6, "%.1f"), cell("cdist_mm", p, 1e-6, "%.1f")))


if __name__ == "__main__":
    main()
