"""The fused attention aggregation against the composition it replaces (GPU only; no GPU is an error).

Composed: ops.incidence_softmax -> ops.incidence_aggr(v2e = e2v = alpha), the path before ops.incidence_attention_aggr
existed.  Fused: ops.incidence_attention_aggr.  Both on the same cached plan, the same seeded inputs, in this process.

Cells (bench.make_workload, the four of tools/attention_probe.py): cora x1024, pubmed x256, pubmed x64, power-law 1M/4M;
F = 32 and 128, H = 1 and 8, group 'hyperedge'.  Per cell:
  * outputs and gradients of the two forms compared first, as bit patterns (faster and different is not faster);
  * forward (no grad) and one training step (forward + backward for X and both scores), the two forms alternating three
    times, medians of the per-call time over `--steps` calls that end in a device synchronise;
  * torch.cuda.max_memory_allocated over one training step of each form, above what is allocated before it.
No ratio is a condition: the probe reports, slower cells included.

    python tools/fused_attention_probe.py [--steps 20] [--cells headline,...] [--out profiles/r13_fused_attention]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from attention_probe import CELLS, SLOPE, timed  # noqa: E402

WIDTHS = (32, 128)
HEADS = (1, 8)
GROUP = "hyperedge"


def alternate(a, b, steps):
    ta, tb = [], []
    for _ in range(3):  # alternate: a drift of the box's clocks lands on both
        ta.append(timed(a, steps))
        tb.append(timed(b, steps))
    return statistics.median(ta), statistics.median(tb)


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_cell(name, shape, replicas, args, dev):
    import bench
    import hypergef_amd as hg
    from hypergef_amd import ops
    _, inc = bench.make_workload(shape, replicas)
    N, M, nnz = inc.N, inc.M, inc.nnz
    hyperg = hg.HyperGraph.from_incidence(inc, dev, ngs=1 << 30)
    ptr, ind = hyperg.H_T_csrptr, hyperg.H_T_colind
    degE, degV = hyperg.degE, hyperg.degV
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for F in WIDTHS:
        for H in HEADS:
            X = torch.randn(N, F, device=dev, generator=g)
            dY = torch.randn(N, F, device=dev, generator=g)
            sv = torch.randn(N, H, device=dev, generator=g)
            se = torch.randn(M, H, device=dev, generator=g)

            def composed(x, a, b):
                alpha = ops.incidence_softmax(ptr, ind, a, b, group=GROUP, negative_slope=SLOPE, heads=H, num_nodes=N)
                return ops.incidence_aggr(ptr, ind, x, alpha, alpha, degE, degV, None, heads=H)

            def fused(x, a, b):
                return ops.incidence_attention_aggr(ptr, ind, x, a, b, group=GROUP, negative_slope=SLOPE, degE=degE,
                                                    degV=degV, heads=H)

            def step(fn):
                leaves = [t.clone().requires_grad_(True) for t in (X, sv, se)]

                def run():
                    for t in leaves:
                        t.grad = None
                    fn(*leaves).backward(dY)
                    return leaves
                return run

            same = bits_equal(fused(X, sv, se), composed(X, sv, se))
            same = same and all(bits_equal(a.grad, b.grad) for a, b in zip(step(fused)(), step(composed)()))
            t_f, t_c = alternate(lambda: fused(X, sv, se), lambda: composed(X, sv, se), args.steps)
            s_f, s_c = alternate(step(fused), step(composed), max(3, args.steps // 2))
            peak = {}
            for label, fn in (("fused", fused), ("composed", composed)):
                run = step(fn)
                run()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                run()
                torch.cuda.synchronize()
                peak[label] = torch.cuda.max_memory_allocated() - base
                del run
            rows.append({"cell": name, "workload": "%s x%d" % (shape, replicas), "N": N, "M": M, "nnz": nnz, "F": F, "H": H,
                         "bits_equal": same, "fwd_fused_ms": t_f, "fwd_composed_ms": t_c, "step_fused_ms": s_f,
                         "step_composed_ms": s_c, "peak_fused_MB": peak["fused"] / 1e6, "peak_composed_MB": peak["composed"] / 1e6,
                         "alpha_MB": nnz * H * 4 / 1e6})
            r = rows[-1]
            print("%-10s F %3d H %d  bits %s  fwd %.3f ms (composed %.3f, x%.2f)  step %.3f ms (composed %.3f, x%.2f)  "
                  "peak above the inputs %.1f MB (composed %.1f; alpha is %.1f)" % (
                      name, F, H, "equal" if same else "DIFFER", t_f, t_c, t_c / t_f, s_f, s_c, s_c / s_f, r["peak_fused_MB"],
                      r["peak_composed_MB"], r["alpha_MB"]), flush=True)
            del X, dY, sv, se
            torch.cuda.empty_cache()
    return rows


def write(path, rows, steps):
    with open(path, "w") as f:
        f.write("# Fused attention aggregation against softmax + incidence_aggr (tools/fused_attention_probe.py)\n\n"
                "%s, %d calls per timing, three alternating rounds, medians; group 'hyperedge'.  x > 1: the fused form is "
                "faster.  Peak: torch.cuda.max_memory_allocated over one training step, above what was allocated before it.\n\n"
                % (torch.cuda.get_device_name(0), steps))
        f.write("| cell | F | H | bits | fwd ms | composed | x | step ms | composed | x | peak MB | composed | alpha MB |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %d | %d | %s | %.3f | %.3f | %.2f | %.3f | %.3f | %.2f | %.1f | %.1f | %.1f |\n" % (
                r["workload"], r["F"], r["H"], "equal" if r["bits_equal"] else "DIFFER", r["fwd_fused_ms"], r["fwd_composed_ms"],
                r["fwd_composed_ms"] / r["fwd_fused_ms"], r["step_fused_ms"], r["step_composed_ms"],
                r["step_composed_ms"] / r["step_fused_ms"], r["peak_fused_MB"], r["peak_composed_MB"], r["alpha_MB"]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--cells", default="all")
    p.add_argument("--out", default=None, help="path stem: writes STEM.md")
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fused_attention_probe: no GPU (this probe measures the device kernels; there is no CPU fallback)")
    dev = torch.device("cuda:0")
    want = None if args.cells == "all" else set(args.cells.split(","))
    rows = []
    for cell in CELLS:
        if want is not None and cell[0] not in want:
            continue
        rows += run_cell(*cell, args, dev)
        if args.out:  # after every cell: a run cut short keeps what it measured
            write(args.out + ".md", rows, args.steps)
        torch.cuda.empty_cache()
    sys.exit(0 if all(r["bits_equal"] for r in rows) else 1)


if __name__ == "__main__":
    main()
