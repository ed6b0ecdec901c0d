"""The incidence, linear, table and kNN operators beyond 2^31 bytes (`B`) and 2^31 elements (`E`) of one array, on the GPU.

Method of test_gpu_parity.test_tables_beyond_2GiB_use_64bit_offsets: a block-diagonal batch of K copies of one small
hypergraph (_large_ref.base: short rows, a wave task that owns its row, a row split over partial slots with a fixup, a
segment beyond kSegLong, an empty hyperedge with degE = inf and an isolated vertex, on both sides), inputs drawn on the
device independently for every copy, and the first, the middle and the last copy plus the one in which the threshold falls
checked on their own against the float64 reference and the bound of the operator's own tests.  Every output the Python API
lets the caller provide lies between guard bands and is prefilled with a sentinel that must be gone afterwards.  One plan
serves the incidence tests of the module (its build would otherwise dominate every one of them); the linear kernels, the
table gathers and the searches take no plan and use row blocks, a block-diagonal table and a few queries instead.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attention_ref as ar  # noqa: E402
import _dropout_ref as dr  # noqa: E402
import _entry_ref as er  # noqa: E402
import _grad_ref as gr  # noqa: E402
import _heads_ref as hr  # noqa: E402
import _incidence_ref as ir  # noqa: E402
import _large_ref as lr  # noqa: E402
import _reduce_ref as rr  # noqa: E402
import _scale_grad_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV, E31, U = lr.DEV, lr.E31, ar.U
Guarded = lr.Guarded
SLOPE = 0.2
F_E = 512     # [N, 512] and [M, 512] reach 2^31 elements
H_E = 128     # [nnz, 128] does


@pytest.fixture(scope="module")
def big(hg):  # hg: the library is built before the plan is
    batch = lr.Batch()
    yield batch
    del batch
    torch.cuda.empty_cache()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _masks(c):
    return ir.hop_masks(c.plan.has_latency_schedule())


def _workspace(c, F):
    return Guarded((max(c.plan.incidence_workspace_bytes(F), 256),), torch.uint8, 0xA5)


def test_the_batch_reaches_every_path_beyond_the_threshold(big):
    c = big
    assert c.N * F_E >= E31 and c.M * F_E >= E31 and c.nnz * H_E >= E31 and c.nnz < E31
    sizes, deg = np.diff(c.one.csrptr), np.bincount(c.one.colind, minlength=c.one.N)
    assert sizes[lr.EMPTY] == 0 and deg[lr.ISOLATED] == 0 and bool(torch.isinf(c.degE[lr.EMPTY + (c.K - 1) * c.one.M]))
    for hop, n0 in ((0, c.one.M), (1, c.one.N)):
        s = c.plan.schedule(hop)
        last = s["tasks"][s["tasks"][:, 0] >= (c.K - 1) * n0]  # the last replica's rows: all beyond the thresholds
        assert len(s["panels"]) > 0 and (last[:, 3] >= 0).sum() >= 2 and (last[:, 3] < 0).sum() >= 1, (hop, last)
        assert (s["fixups"][:, 0] >= (c.K - 1) * n0).any(), hop
        info = c.plan.segment_info(hop)
        assert (sizes, deg)[hop].max() > info["long"] and (info["long_rows"] >= (c.K - 1) * n0).any(), (hop, info)


# ---- 1. aggregate_incidence -------------------------------------------------------------------------------------------------

def _check_aggr(c, r, X, v2e, e2v, heads, Y, Xe, what):
    g = c.graph(r)
    x = X[c.rows(r, 1)].float()
    a, b = (w[c.rows(r, "nnz")].reshape(-1, heads) for w in (v2e, e2v))
    out, _, mass, _ = gr.evaluate(hr.fn, g, {"x": x, "v2e": a, "e2v": b, "heads": heads}, torch.zeros(c.one.N, x.shape[1]), ())
    gr.assert_within(Y[c.rows(r, 1)], out, mass, gr.FP32_C, "%s, Y of replica %d" % (what, r))
    if Xe is not None:
        xe = er.gather(g, gr.f64(x), gr.f64(a), g.se, None, "hyperedge", heads)
        xm = er.gather(g, gr.f64(x).abs(), gr.f64(a), g.se, None, "hyperedge", heads)
        gr.assert_within(Xe[c.rows(r, 0)], xe, xm, gr.FP32_C, "%s, xe_out of replica %d" % (what, r))


def _run_aggr(c, X, v2e, e2v, heads, replicas, with_xe, what):
    F = X.shape[1]
    Y, ws = Guarded((c.N, F)), _workspace(c, F)
    Xe = Guarded((c.M, F)) if with_xe else None
    try:
        for mask in (None,) + _masks(c):
            if mask is not None:
                c.plan.pin(F, "pull", mask)
                Y.refill()
                if with_xe:
                    Xe.refill()
            c.plan.aggregate_incidence(c.ptr, c.ind, X, v2e, e2v, c.degE, c.degV, c.W, xe_out=Xe.t if with_xe else None,
                                       out=Y.t, workspace=ws.t, heads=heads)
            torch.cuda.synchronize()
            label = "%s, hop kernels %s" % (what, mask)
            for buf in (Y, Xe):
                if buf is not None:
                    buf.check(label)
            ws.check(label, written=False)
            for r in (replicas if mask is None else [c.K - 1]):
                _check_aggr(c, r, X, v2e, e2v, heads, Y.t, Xe.t if with_xe else None, label)
    finally:
        c.plan.unpin(F)


@pytest.mark.parametrize("heads", [1, 8])
def test_aggregate_incidence_rows_at_E(big, heads):
    """X, Y and xe_out [*, 512] beyond 2^31 elements, v2e / e2v [nnz] and [nnz, 8]; the last replica again under every
    pull hop-kernel pair.  Peak device memory: 31 GB."""
    c = big
    assert c.N * F_E >= E31 and c.M * F_E >= E31
    X = lr.randn(c.N, F_E, seed=1)
    shape = (c.nnz,) if heads == 1 else (c.nnz, heads)
    v2e, e2v = lr.rand_weights(*shape, seed=2), lr.rand_weights(*shape, seed=3)
    replicas = sorted(set(lr.picked(c.K, c.one.N * F_E) + lr.picked(c.K, c.one.M * F_E)))
    _run_aggr(c, X, v2e, e2v, heads, replicas, True, "aggregate_incidence heads %d" % heads)
    del X, v2e, e2v
    torch.cuda.empty_cache()


@pytest.mark.parametrize("C", [1, 4])
def test_aggregate_incidence_weights_at_E(big, C):
    """v2e and e2v [nnz, 128] beyond 2^31 elements with C = 1 (scalar lanes) and C = 4 (16-byte lanes) columns a head;
    xe_out with C = 1 only (memory).  Peak device memory: 24 GB (C = 1), 38 GB (C = 4)."""
    c = big
    assert c.nnz * H_E >= E31
    X = lr.randn(c.N, H_E * C, seed=4)
    v2e, e2v = lr.rand_weights(c.nnz, H_E, seed=5), lr.rand_weights(c.nnz, H_E, seed=6)
    _run_aggr(c, X, v2e, e2v, H_E, lr.picked(c.K, c.one.nnz * H_E), C == 1, "aggregate_incidence H %d C %d" % (H_E, C))
    del X, v2e, e2v
    torch.cuda.empty_cache()


# ---- 2. gather_rows_incidence -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", ["f32-E", "bf16-B", "bf16-E"])
@pytest.mark.parametrize("hop", [0, 1])
def test_gather_rows_incidence(big, hop, rows):
    """One weighted hop with 8 heads: fp32 rows [*, 512] beyond 2^31 elements, bf16 rows [*, 256] beyond 2^31 bytes (2^30
    elements) and bf16 rows [*, 512] beyond 2^31 elements, source and destination alike; the last replica again under
    every pull hop-kernel pair.  Bound: FP32_C of the mass, and one bf16 rounding of the result more (bf16_c(1)) for a
    bf16 destination.  Peak device memory: 21 GB."""
    c, heads = big, 8
    bf16 = rows.startswith("bf16")
    F = 256 if rows == "bf16-B" else F_E
    dtype, size = (torch.bfloat16, 2) if bf16 else (torch.float32, 4)
    nsrc, ndst, n0src, n0dst = (c.N, c.M, c.one.N, c.one.M) if hop == 0 else (c.M, c.N, c.one.M, c.one.N)
    if rows == "bf16-B":
        assert min(nsrc, ndst) * F * size >= E31 and min(nsrc, ndst) * F >= 2 ** 30
        replicas = lr.picked(c.K, n0src * F * size) + lr.picked(c.K, n0dst * F * size)
    else:
        assert min(nsrc, ndst) * F >= E31
        replicas = lr.picked(c.K, n0src * F) + lr.picked(c.K, n0dst * F)
    src = lr.randn(nsrc, F, seed=10 + hop, dtype=dtype)
    w = lr.rand_weights(c.nnz, heads, seed=12)
    sa, sb = (c.degE, c.W) if hop == 0 else (c.degV, None)
    dst, ws = Guarded((ndst, F), dtype), _workspace(c, F)
    to = "hyperedge" if hop == 0 else "vertex"
    bound = gr.bf16_c(1) if bf16 else gr.FP32_C
    try:
        for mask in (None,) + _masks(c):
            if mask is not None:
                c.plan.pin(F, "pull", mask)
                dst.refill()
            c.plan.gather_rows_incidence(hop, c.ptr, c.ind, src, w, sa, sb, heads=heads, out=dst.t, workspace=ws.t)
            torch.cuda.synchronize()
            what = "gather_rows_incidence hop %d %s, hop kernels %s" % (hop, rows, mask)
            dst.check(what)
            ws.check(what, written=False)
            for r in (sorted(set(replicas)) if mask is None else [c.K - 1]):
                s, d, p = c.rows(r, 1 - hop), c.rows(r, hop), c.rows(r, "nnz")
                a = torch.nan_to_num(gr.f64(sa[d]), posinf=0.0)  # the empty hyperedge: 1 / 0, never multiplied
                b = None if sb is None else gr.f64(sb[d])
                x, wr = gr.f64(src[s]), gr.f64(w[p])
                ref = er.gather(c.index, x, wr, a, b, to, heads)
                mass = er.gather(c.index, x.abs(), wr, a, b, to, heads)
                gr.assert_within(dst.t[d], ref, mass, bound, "%s, replica %d" % (what, r))
    finally:
        c.plan.unpin(F)
    del src, w
    torch.cuda.empty_cache()


# ---- 3. incidence_dot -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,heads,F", [("f32", 1, F_E), ("f32", 8, F_E), ("bf16", 1, F_E), ("bf16", 8, F_E),
                                          ("f32", H_E, H_E), ("bf16", H_E, 4 * H_E)])
def test_incidence_dot(big, kind, heads, F):
    """A [N, 512] and B [M, 512] beyond 2^31 elements with one head and with 8, fp32 and bf16; out [nnz, 128] beyond 2^31
    elements from fp32 rows of C = 1 and bf16 rows of C = 4.  Bound: FP32_C + (C + 1) U of the mass (test_heads_gpu).
    Peak device memory: 21 GB (fp32 rows at E), 20 GB (out at E)."""
    c = big
    dtype = torch.bfloat16 if kind == "bf16" else torch.float32
    if heads == H_E:
        assert c.nnz * heads >= E31
        replicas = lr.picked(c.K, c.one.nnz * heads)
    else:
        assert c.N * F >= E31 and c.M * F >= E31
        replicas = sorted(set(lr.picked(c.K, c.one.N * F) + lr.picked(c.K, c.one.M * F)))
    A, B = lr.randn(c.N, F, seed=20, dtype=dtype), lr.randn(c.M, F, seed=21, dtype=dtype)
    out = Guarded((c.nnz,) if heads == 1 else (c.nnz, heads))
    c.plan.incidence_dot(c.ptr, c.ind, A, B, out=out.t, heads=heads)
    torch.cuda.synchronize()
    what = "incidence_dot %s heads %d F %d" % (kind, heads, F)
    out.check(what)
    for r in replicas:
        a, b = A[c.rows(r, 1)], B[c.rows(r, 0)]
        gr.assert_within(out.t[c.rows(r, "nnz")].reshape(-1, heads), hr.dot(c.index, a, b, heads), hr.dot_mass(c.index, a, b, heads),
                         gr.FP32_C + (F // heads + 1) * U, "%s, replica %d" % (what, r))
    del A, B
    torch.cuda.empty_cache()


# ---- 4. the segment softmax -------------------------------------------------------------------------------------------------

def _raw64(c, sv, se, t=None):
    raw = gr.f64(sv)[c.index.V] + gr.f64(se)[c.index.E]
    return raw if t is None else raw + gr.f64(t)


@pytest.mark.parametrize("entry", [False, True])
@pytest.mark.parametrize("group", ar.GROUPS)
def test_softmax_and_backward_at_E(big, group, entry):
    """alpha, dalpha and ds [nnz, 128] beyond 2^31 elements, from scores sv, se [*, 128] alone and with a logit per
    incidence (also at E) added: incidence_attention and its backward.  Bounds: alpha within (L + 16 + 16 Smax) U of itself (test_heads_gpu;
    _entry_ref.bound_c with the logit), the gradients within 2 c + (L + D + 8) U of their mass.  ds, dsv and dse are
    allocated by the call: no guard bands for them.  Peak device memory: 37 GB."""
    c, H = big, H_E
    assert c.nnz * H >= E31
    sv, se = lr.scores(c.N, H, seed=30), lr.scores(c.M, H, seed=31)
    t = lr.scores(c.nnz, H, seed=32) if entry else None
    alpha = Guarded((c.nnz, H))
    c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, SLOPE, out=alpha.t, heads=H, entry=t)
    torch.cuda.synchronize()
    what = "softmax %s entry %s" % (group, entry)
    alpha.check(what)
    dalpha = t if entry else lr.randn(c.nnz, H, seed=33)  # with the logit its array serves as the gradient too: 40 GB
    ds, dsv, dse = c.plan.incidence_attention_backward(c.ptr, c.ind, alpha.t, dalpha, sv, se, group, SLOPE, heads=H, entry=t)
    torch.cuda.synchronize()
    D = {"ds": 0, "dsv": c.L["vertex"], "dse": c.L["hyperedge"]}
    for r in lr.picked(c.K, c.one.nnz * H):
        p = c.rows(r, "nnz")
        raw = _raw64(c, sv[c.rows(r, 1)], se[c.rows(r, 0)], t[p] if entry else None)
        smax = float(raw.abs().max())
        assert smax <= 8.0
        cc = er.bound_c(c.L[group], smax) if entry else (c.L[group] + 16 + 16 * smax) * U
        ref = er.softmax_raw(c.index, raw, group, SLOPE)
        gr.assert_within(alpha.t[p], ref, ref, cc, "%s, alpha of replica %d" % (what, r))
        da = gr.f64(dalpha[p])
        want = dict(zip(("ds", "dsv", "dse"), er.closed_form_backward(c.index, raw, group, SLOPE, ref, da)))
        mass = dict(zip(("ds", "dsv", "dse"), er.backward_masses(c.index, group, SLOPE, ref, da)))
        got = {"ds": ds[p], "dsv": dsv[c.rows(r, 1)], "dse": dse[c.rows(r, 0)]}
        for name in ("ds", "dsv", "dse"):
            gr.assert_within(got[name], want[name], mass[name], 2 * cc + (c.L[group] + D[name] + 8) * U,
                             "%s, %s of replica %d" % (what, name, r))
    del sv, se, t, dalpha, ds, dsv, dse
    torch.cuda.empty_cache()


@pytest.mark.parametrize("group", ar.GROUPS)
def test_statistics_and_incidence_sum_at_E(big, group):
    """incidence_attention_stats with scores and statistics [*, 128] beyond 2^31 bytes: alpha rebuilt from them within
    (L + 16 + 16 Smax + 4) U (test_fused_attention_gpu); incidence_sum of val [nnz, 128] beyond 2^31 elements within
    (L + 2) U of the mass (test_heads_gpu).  Peak device memory: 18 GB."""
    c, H = big, H_E
    nseg, n0 = (c.M, c.one.M) if group == "hyperedge" else (c.N, c.one.N)
    assert c.nnz * H >= E31 and nseg * H * 4 >= E31
    sv, se = lr.scores(c.N, H, seed=34), lr.scores(c.M, H, seed=35)
    mx, inv = Guarded((nseg, H)), Guarded((nseg, H))
    c.plan.incidence_attention_stats(c.ptr, c.ind, sv, se, group, SLOPE, heads=H, out=(mx.t, inv.t))
    val = lr.randn(c.nnz, H, seed=36)
    total = Guarded((nseg, H))
    c.plan.incidence_sum(c.ptr, c.ind, val, group, out=total.t, heads=H)
    torch.cuda.synchronize()
    for buf, name in ((mx, "seg_max"), (inv, "seg_inv"), (total, "incidence_sum")):
        buf.check("%s %s" % (name, group))
    idx, _ = ar.index_of(c.index, group)
    for r in sorted(set(lr.picked(c.K, c.one.nnz * H) + lr.picked(c.K, n0 * H * 4))):
        seg = c.rows(r, group)
        raw = _raw64(c, sv[c.rows(r, 1)], se[c.rows(r, 0)])
        ref = er.softmax_raw(c.index, raw, group, SLOPE)
        raw32 = raw.float().double()  # the kernel's raw: one fp32 addition of two fp32 scores
        rebuilt = torch.exp(torch.nn.functional.leaky_relu(raw32, SLOPE) - gr.f64(mx.t[seg])[idx]) * gr.f64(inv.t[seg])[idx]
        gr.assert_within(rebuilt, ref, ref, (c.L[group] + 16 + 16 * 8.0 + 4) * U, "statistics %s, replica %d" % (group, r))
        v = gr.f64(val[c.rows(r, "nnz")])
        gr.assert_within(total.t[seg], er.seg_sum(c.index, v, group), er.seg_sum(c.index, v.abs(), group), (c.L[group] + 2) * U,
                         "incidence_sum %s, replica %d" % (group, r))
    del sv, se, val
    torch.cuda.empty_cache()


@pytest.mark.parametrize("group", ar.GROUPS)
def test_dropout_at_B(big, group):
    """incidence_attention_dropout and its backward with [nnz, 32] arrays beyond 2^31 bytes.  The mask is compared on the
    four replicas with _dropout_ref's Philox at those replicas' positions (the whole 547 M-element host mask is not
    formed): a dropped coefficient is +0.0 and a kept one alpha * scale, bit for bit; the kept share of the whole array
    is within 4 sigma of 1 - p; the backward equals incidence_attention_backward on the masked gradient, bit for bit,
    over the whole arrays.  Peak device memory: 20 GB."""
    c, H, pd = big, 32, 0.3
    assert c.nnz * H * 4 >= E31
    key, sid = 0x123456789ABCDEF, 0x0FEDCBA987654321
    rng = torch.tensor([key, sid], dtype=torch.int64, device=DEV)
    sv, se = lr.scores(c.N, H, seed=37), lr.scores(c.M, H, seed=38)
    plain = c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, SLOPE, heads=H)
    alpha, drop = c.plan.incidence_attention_dropout(c.ptr, c.ind, sv, se, group, SLOPE, pd, rng, heads=H)
    torch.cuda.synchronize()
    assert torch.equal(_bits(alpha), _bits(plain))
    scale = float(dr.scale(pd))
    n0 = c.one.nnz
    for r in lr.picked(c.K, n0 * H * 4):
        pos, h = np.meshgrid(np.arange(r * n0, (r + 1) * n0, dtype=np.uint64), np.arange(H, dtype=np.uint64), indexing="ij")
        word = dr.philox4x32_10((pos, h, np.full_like(pos, sid & dr.MASK32), np.full_like(pos, sid >> 32)),
                                (key & dr.MASK32, key >> 32))[0]
        keep = torch.from_numpy(word.astype(np.uint64) >= np.uint64(dr.threshold(pd))).to(DEV)
        a = alpha[c.rows(r, "nnz")]
        want = torch.where(keep, a * scale, torch.zeros_like(a))
        assert torch.equal(_bits(drop[c.rows(r, "nnz")]), _bits(want)), "dropout %s, replica %d" % (group, r)
    kept = drop != 0
    n = kept.numel()
    assert abs(int(kept.sum()) - (1 - pd) * n) <= 4 * (n * pd * (1 - pd)) ** 0.5
    dout = lr.randn(c.nnz, H, seed=39)
    got = c.plan.incidence_attention_dropout_backward(c.ptr, c.ind, alpha, dout, sv, se, group, SLOPE, pd, rng, heads=H)
    masked = torch.where(kept, dout * scale, torch.zeros_like(dout))
    want = c.plan.incidence_attention_backward(c.ptr, c.ind, alpha, masked, sv, se, group, SLOPE, heads=H)
    for a, b, name in zip(got, want, ("ds", "dsv", "dse")):
        assert torch.equal(_bits(a), _bits(b)), "dropout backward %s %s" % (group, name)
    del sv, se, plain, alpha, drop, kept, dout, masked, got, want
    torch.cuda.empty_cache()


# ---- 5. the fused attention gather -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", ar.GROUPS)
def test_fused_attention_equals_the_composition_at_E(big, group):
    """aggregate_incidence_attention and gather_rows_attention with X, Y and xe_out [*, 512] beyond 2^31 elements, 8 heads:
    over the whole arrays the bits of aggregate_incidence on incidence_attention's alpha, which
    test_aggregate_incidence_rows_at_E holds against float64; here the four replicas are compared with float64 as well
    (FP32_C + 2 c_alpha + (C + 1) U of the mass, test_fused_attention_gpu).  Scores [*, H] beyond 2^31 bytes need more
    than 120 heads, which the entry refuses under the default panel_rows (LDS for the rows' scores): not run.  Peak device
    memory: 39 GB."""
    c, H, F = big, 8, F_E
    assert c.N * F >= E31 and c.M * F >= E31
    X = lr.randn(c.N, F, seed=40)
    sv, se = lr.scores(c.N, H, seed=41), lr.scores(c.M, H, seed=42)
    alpha = c.plan.incidence_attention(c.ptr, c.ind, sv, se, group, SLOPE, heads=H)
    want = c.plan.aggregate_incidence(c.ptr, c.ind, X, alpha, alpha, c.degE, c.degV, c.W, heads=H)
    mx, inv = c.plan.incidence_attention_stats(c.ptr, c.ind, sv, se, group, SLOPE, heads=H)
    Y, Xe, ws = Guarded((c.N, F)), Guarded((c.M, F)), _workspace(c, F)
    c.plan.aggregate_incidence_attention(c.ptr, c.ind, X, sv, se, group, SLOPE, mx, inv, c.degE, c.degV, c.W, xe_out=Xe.t,
                                         out=Y.t, workspace=ws.t, heads=H)
    torch.cuda.synchronize()
    what = "fused attention %s" % group
    Y.check(what)
    Xe.check(what)
    ws.check(what, written=False)
    assert torch.equal(_bits(Y.t), _bits(want)), what
    c_lin = gr.FP32_C + 2 * (c.L[group] + 16 + 16 * 8.0) * U + (F // H + 1) * U
    for r in sorted(set(lr.picked(c.K, c.one.N * F) + lr.picked(c.K, c.one.M * F))):
        a = er.softmax_raw(c.index, _raw64(c, sv[c.rows(r, 1)], se[c.rows(r, 0)]), group, SLOPE)
        out, _, mass, _ = gr.evaluate(hr.fn, c.graph(r), {"x": X[c.rows(r, 1)], "v2e": a, "e2v": a, "heads": H},
                                      torch.zeros(c.one.N, F), ())
        gr.assert_within(Y.t[c.rows(r, 1)], out, mass, c_lin, "%s, replica %d" % (what, r))
    del want
    Y.refill()
    c.plan.gather_rows_attention(1, c.ptr, c.ind, Xe.t, mx, inv, sv, se, group, SLOPE, c.degV, None, heads=H, out=Y.t,
                                 workspace=ws.t)
    Y.check(what + ", hop 1 alone")
    hop0 = c.plan.gather_rows_attention(0, c.ptr, c.ind, X, mx, inv, sv, se, group, SLOPE, c.degE, c.W, heads=H, workspace=ws.t)
    assert torch.equal(_bits(hop0), _bits(Xe.t)), what + ", hop 0 alone"
    del hop0
    again = c.plan.aggregate_incidence(c.ptr, c.ind, X, alpha, alpha, c.degE, c.degV, c.W, heads=H)
    assert torch.equal(_bits(Y.t), _bits(again)), what + ", hop 1 alone"
    ws.check(what, written=False)
    del X, sv, se, alpha, again, mx, inv
    torch.cuda.empty_cache()


# ---- 6. max / min and the select gather ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", rr.OPS)
@pytest.mark.parametrize("hop", [0, 1])
def test_reduce_and_select_at_E(big, hop, op):
    """gather_rows_reduce and gather_rows_select with src, dst, arg_out, gs and dsrc [*, 512] beyond 2^31 elements: value
    and winner equal _reduce_ref's bit for bit on the four replicas (so arg_out holds positions of the replica's own
    entries), the select gather equals select_grad in float64 within FP32_C of the mass; the last replica again under
    every pull hop-kernel pair.  Peak device memory: 39 GB."""
    c, F = big, F_E
    nsrc, ndst, n0src, n0dst = (c.N, c.M, c.one.N, c.one.M) if hop == 0 else (c.M, c.N, c.one.M, c.one.N)
    assert nsrc * F >= E31 and ndst * F >= E31
    replicas = sorted(set(lr.picked(c.K, n0src * F) + lr.picked(c.K, n0dst * F)))
    src = lr.randn(nsrc, F, seed=50 + hop)
    dst, arg = Guarded((ndst, F)), Guarded((ndst, F), torch.int32, lr.ARG_SENTINEL)
    ws = Guarded((max(c.plan.reduce_workspace_bytes(F), 256),), torch.uint8, 0xA5)
    E, V = rr.entries(c.one)
    nnz0 = c.one.nnz
    try:
        for mask in (None,) + _masks(c):
            if mask is not None:
                c.plan.pin(F, "pull", mask)
                dst.refill()
                arg.refill()
            c.plan.gather_rows_reduce(hop, c.ptr, c.ind, src, op, out=dst.t, arg_out=arg.t, workspace=ws.t)
            torch.cuda.synchronize()
            what = "gather_rows_reduce hop %d %s, hop kernels %s" % (hop, op, mask)
            dst.check(what)
            arg.check(what)
            ws.check(what, written=False)
            for r in (replicas if mask is None else [c.K - 1]):
                val, win = rr.reduce_hop(c.one, hop, src[c.rows(r, 1 - hop)].cpu(), op, E, V)
                d = c.rows(r, hop)
                assert torch.equal(_bits(dst.t[d].cpu()), _bits(val)), "%s, values of replica %d" % (what, r)
                shifted = torch.where(win >= 0, win + r * nnz0, win)
                assert torch.equal(arg.t[d].cpu().long(), shifted), "%s, positions of replica %d" % (what, r)
    finally:
        c.plan.unpin(F)
    del dst
    torch.cuda.empty_cache()
    gs = lr.randn(ndst, F, seed=52 + hop)
    dsrc = Guarded((nsrc, F))
    c.plan.gather_rows_select(hop, c.ptr, c.ind, gs, arg.t, out=dsrc.t, workspace=ws.t)
    torch.cuda.synchronize()
    what = "gather_rows_select hop %d %s" % (hop, op)
    dsrc.check(what)
    ws.check(what, written=False)
    for r in replicas:
        d = c.rows(r, hop)
        win = arg.t[d].cpu().long()
        win = torch.where(win >= 0, win - r * nnz0, win)
        g = gr.f64(gs[d])
        gr.assert_within(dsrc.t[c.rows(r, 1 - hop)], rr.select_grad(c.one, hop, g, win, E, V),
                         rr.select_grad(c.one, hop, g.abs(), win, E, V), gr.FP32_C, "%s, replica %d" % (what, r))
    del src, gs
    torch.cuda.empty_cache()


# ---- 7. hyperedge_dot and rows_dot -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads", [1, 8])
def test_hyperedge_dot_and_rows_dot_at_E(big, heads):
    """hyperedge_dot with A, B [N, 512] beyond 2^31 elements and weights [nnz, heads], within 2 FP32_C + (F + 2) U of the
    mass (test_scale_grads_gpu); rows_dot of the same operands within (F + 1) U.  Both allocate their result: no
    guard bands.  Peak device memory: 19 GB."""
    c, F = big, F_E
    assert c.N * F >= E31
    A, B = lr.randn(c.N, F, seed=60), lr.randn(c.N, F, seed=61)
    wa, wb = lr.rand_weights(c.nnz, heads, seed=62), lr.rand_weights(c.nnz, heads, seed=63)
    got = c.plan.hyperedge_dot(c.ptr, c.ind, A, B, wa, wb, heads=heads)
    rows = c.plan.rows_dot(A, B)
    torch.cuda.synchronize()
    assert got.shape == (c.M,) and rows.shape == (c.N,)
    idx = sr.Index(c.one)
    for r in lr.picked(c.K, c.one.N * F):
        a, b = gr.f64(A[c.rows(r, 1)]), gr.f64(B[c.rows(r, 1)])
        p, q = (gr.f64(w[c.rows(r, "nnz")]) for w in (wa, wb))
        gr.assert_within(got[c.rows(r, 0)], sr.edge_dot(idx, a, p, b, q, heads), sr.edge_dot(idx, a.abs(), p, b.abs(), q, heads),
                         2 * gr.FP32_C + (F + 2) * U, "hyperedge_dot heads %d, replica %d" % (heads, r))
        gr.assert_within(rows[c.rows(r, 1)], (a * b).sum(1), (a * b).abs().sum(1), (F + 1) * U,
                         "rows_dot, replica %d" % r)
    del A, B, wa, wb
    torch.cuda.empty_cache()


def test_fused_attention_scores_at_B(big):
    """aggregate_incidence_attention and gather_rows_attention with 128 heads: scores sv, se and statistics [*, 128] beyond
    2^31 bytes.  A workgroup keeps three scalars per panel row and head in LDS, which the default panel_rows = 128 does
    not leave room for at 128 heads (the entry refuses); a plan of panel_rows = 32 over the same batch runs it.  The bits
    are those of aggregate_incidence on that plan with incidence_attention's alpha, over the whole arrays, and the four
    replicas are held against float64.  Peak device memory: 27 GB."""
    from hypergef_amd.plan import Plan, make_opts
    c, H, F = big, H_E, H_E
    assert min(c.N, c.M) * H * 4 >= E31
    plan = Plan.from_tensors(c.N, c.ptr, c.ind, make_opts(panel_rows=32))
    X = lr.randn(c.N, F, seed=43)
    sv, se = lr.scores(c.N, H, seed=44), lr.scores(c.M, H, seed=45)
    c_lin = gr.FP32_C + 2 * (max(c.L.values()) + 16 + 16 * 8.0) * U + (F // H + 1) * U
    for group in ar.GROUPS:
        nseg = c.M if group == "hyperedge" else c.N
        mx, inv = Guarded((nseg, H)), Guarded((nseg, H))
        plan.incidence_attention_stats(c.ptr, c.ind, sv, se, group, SLOPE, heads=H, out=(mx.t, inv.t))
        Y, Xe, ws = Guarded((c.N, F)), Guarded((c.M, F)), Guarded((max(plan.incidence_workspace_bytes(F), 256),), torch.uint8, 0xA5)
        plan.aggregate_incidence_attention(c.ptr, c.ind, X, sv, se, group, SLOPE, mx.t, inv.t, c.degE, c.degV, c.W, xe_out=Xe.t,
                                           out=Y.t, workspace=ws.t, heads=H)
        torch.cuda.synchronize()
        what = "fused attention, 128 heads, %s" % group
        for buf in (mx, inv, Y, Xe):
            buf.check(what)
        ws.check(what, written=False)
        alpha = plan.incidence_attention(c.ptr, c.ind, sv, se, group, SLOPE, heads=H)
        want_xe = torch.empty(c.M, F, device=DEV)
        want = plan.aggregate_incidence(c.ptr, c.ind, X, alpha, alpha, c.degE, c.degV, c.W, xe_out=want_xe, heads=H)
        assert torch.equal(_bits(Y.t), _bits(want)) and torch.equal(_bits(Xe.t), _bits(want_xe)), what
        del alpha, want
        hop0 = plan.gather_rows_attention(0, c.ptr, c.ind, X, mx.t, inv.t, sv, se, group, SLOPE, c.degE, c.W, heads=H)
        hop1 = plan.gather_rows_attention(1, c.ptr, c.ind, hop0, mx.t, inv.t, sv, se, group, SLOPE, c.degV, None, heads=H)
        assert torch.equal(_bits(hop0), _bits(want_xe)) and torch.equal(_bits(hop1), _bits(Y.t)), what + ", one hop at a time"
        del hop0, hop1, want_xe
        for r in sorted(set(lr.picked(c.K, c.one.N * H * 4) + lr.picked(c.K, c.one.M * H * 4))):
            a = er.softmax_raw(c.index, _raw64(c, sv[c.rows(r, 1)], se[c.rows(r, 0)]), group, SLOPE)
            out, _, mass, _ = gr.evaluate(hr.fn, c.graph(r), {"x": X[c.rows(r, 1)], "v2e": a, "e2v": a, "heads": H},
                                          torch.zeros(c.one.N, F), ())
            gr.assert_within(Y.t[c.rows(r, 1)], out, mass, c_lin, "%s, replica %d" % (what, r))
        del mx, inv, Y, Xe, ws
    del X, sv, se, plan
    torch.cuda.empty_cache()


# ---- 8. the linear kernels ------------------------------------------------------------------------------------------------------

# [ROWS_E, 128] passes 2^31 elements at row 2^24, so 4099 rows lie beyond it: the last row block (2048 rows) is wholly
# beyond, and dropping those rows from linear_wgrad's sums would change an entry by about sqrt(4099) = 64, against a bound
# of 2e-5 * 4 sqrt(ROWS_E) = 0.33
ROWS_E = 2 ** 24 + 4099


def _row_blocks(rows, F, block=2048):
    """Blocks of rows standing in for the replicas: the first, the middle, the one holding element 2^31, the last."""
    hit = E31 // F
    assert block < hit < rows - block
    return [slice(0, block), slice(rows // 2, rows // 2 + block), slice(hit - block // 2, hit + block // 2), slice(rows - block, rows)]


def test_linear_rows_and_wgrad_at_E(hg):
    """linear_rows with X and Y [2^24 + 4099, 128] beyond 2^31 elements, blocks of rows against the float64 product within
    test_gpu_parity's 2e-5 of the largest term; linear_wgrad of X and an independent B of the same shape against the float64 product
    accumulated over all rows on the device, within its 2e-5 * 4 sqrt(rows).  Peak device memory: 19 GB."""
    from hypergef_amd.plan import linear_rows, linear_wgrad
    rows, F = ROWS_E, 128
    assert rows * F >= E31
    X = lr.randn(rows, F, seed=70)
    Wl = lr.randn(F, F, seed=71).mul_(0.1)
    Y = Guarded((rows, F))
    linear_rows(X, Wl, out=Y.t)
    torch.cuda.synchronize()
    Y.check("linear_rows")
    w64 = Wl.double().cpu().numpy()
    for blk in _row_blocks(rows, F):
        ref = X[blk].double().cpu().numpy() @ w64.T
        y = Y.t[blk].cpu().numpy()
        scale = max(1.0, float(np.abs(ref).max()))
        assert np.abs(y - ref).max() <= 2e-5 * scale and np.allclose(y, ref, rtol=1e-4, atol=2e-5 * scale), blk
    del Y
    B = lr.randn(rows, F, seed=72)  # independent of X, as in linear_wgrad's test: every entry a sum of zero-mean products
    C = linear_wgrad(X, B)
    ref = torch.zeros(F, F, dtype=torch.float64, device=DEV)
    for lo in range(0, rows, 1 << 20):
        ref += X[lo:lo + (1 << 20)].double().t() @ B[lo:lo + (1 << 20)].double()
    err = float((C.double() - ref).abs().max())
    assert err <= 2e-5 * max(1.0, rows ** 0.5 * 4), err
    del X, B, C, ref
    torch.cuda.empty_cache()


def _linear_inputs(c, F_in, F_out, seed):
    X, R = lr.randn(c.N, F_in, seed=seed), lr.randn(c.N, F_in, seed=seed + 1)
    Wl = lr.randn(F_out, F_in, seed=seed + 2).div_(F_in ** 0.5)
    return X, R, Wl


def _bracket64(c, r, X, R, ca, cb):
    """(ca Aggr(X) + cb R, its mass) of replica r in float64."""
    g, rows = c.graph(r), c.rows(r, 1)
    x, res = gr.f64(X[rows]), gr.f64(R[rows])
    return g.A(x) * ca + res * cb, g.abs().A(x.abs()) * ca + res.abs() * cb


@pytest.mark.parametrize("variant", ["auto", "pull"])
def test_aggregate_linear_at_B_and_E(big, variant):
    """aggregate_linear 128 -> 512 with a residual: X, the residual and T_out [N, 128] beyond 2^31 bytes, Y [N, 512] beyond
    2^31 elements.  F_in is at most 128, so [N, F_in] passes 2^31 elements only from 2^24 vertices, four times this batch:
    not run.  T_out within FP32_C of the mass of the float64 bracket, Y within test_gpu_parity's 2e-5 of the largest term
    of the float64 product.  Peak device memory: 21 GB."""
    c, F_in, F_out, ca, cb = big, 128, F_E, 0.9, 0.1
    assert c.N * F_in * 4 >= E31 and c.N * F_out >= E31
    X, R, Wl = _linear_inputs(c, F_in, F_out, 80)
    Y, T = Guarded((c.N, F_out)), Guarded((c.N, F_in))
    ws = Guarded((max(c.plan.linear_workspace_bytes(F_in), 256) + 256,), torch.uint8, 0xA5)
    c.plan.aggregate_linear(c.ptr, c.ind, X, Wl, c.degE, c.degV, c.W, variant=variant, out=Y.t, workspace=ws.t, residual=R, ca=ca,
                            cb=cb, t_out=T.t)
    torch.cuda.synchronize()
    what = "aggregate_linear %s" % variant
    Y.check(what)
    T.check(what)
    ws.check(what, written=False)
    w64 = gr.f64(Wl)
    for r in sorted(set(lr.picked(c.K, c.one.N * F_in * 4) + lr.picked(c.K, c.one.N * F_out))):
        t64, mass = _bracket64(c, r, X, R, ca, cb)
        gr.assert_within(T.t[c.rows(r, 1)], t64, mass, gr.FP32_C, "%s, T_out of replica %d" % (what, r))
        ref = (t64 @ w64.t()).numpy()
        y = Y.t[c.rows(r, 1)].cpu().numpy()
        scale = max(1.0, float(np.abs(ref).max()))
        assert np.abs(y - ref).max() <= 2e-5 * scale and np.allclose(y, ref, rtol=1e-4, atol=2e-5 * scale), (what, r)
    c.plan.unbind()
    del X, R, Y, T, ws
    torch.cuda.empty_cache()


@pytest.mark.parametrize("variant", ["auto", "pull"])
def test_aggregate_linear_bf16_at_E(big, variant):
    """aggregate_linear_bf16 128 -> 512 with a residual and relu: Y [N, 512] bf16 beyond 2^31 elements (4.5 GB); X, the
    residual and T_out [N, 128] bf16 are 1.1 GB each and cannot pass 2^31 bytes on this batch (F_in is at most 128).
    T_out lies within bf16_c(1) of the float64 bracket on the four replicas and equals the fp32 call's bracket rounded
    once, bit for bit over the whole array (under "pull" with both calls on the same hop kernels, see below); Y within test_bf16_linear_gpu's bound of the float64 product of the call's own
    T_out.  Peak device memory: 26 GB."""
    from test_bf16_linear_gpu import _y_bound
    c, F_in, F_out, ca, cb = big, 128, F_E, 0.9, 0.1
    assert c.N * F_out >= E31
    X32, R32, W32 = _linear_inputs(c, F_in, F_out, 84)
    X, R, Wl = X32.bfloat16(), R32.bfloat16(), W32.bfloat16()
    X32, R32 = X.float(), R.float()
    Y, T = Guarded((c.N, F_out), torch.bfloat16), Guarded((c.N, F_in), torch.bfloat16)
    ws = Guarded((max(c.plan.linear_workspace_bytes(F_in), 256) + 256,), torch.uint8, 0xA5)
    kw = dict(degE=c.degE, degV=c.degV, W=c.W, variant=variant, ca=ca, cb=cb, relu=True)
    c.plan.aggregate_linear_bf16(c.ptr, c.ind, X, Wl, out=Y.t, workspace=ws.t, residual=R, t_out=T.t, **kw)
    torch.cuda.synchronize()
    what = "aggregate_linear_bf16 %s" % variant
    Y.check(what)
    T.check(what)
    ws.check(what, written=False)
    for r in lr.picked(c.K, c.one.N * F_out):  # the call as it runs by default, against float64
        rows = c.rows(r, 1)
        t64, mass = _bracket64(c, r, X, R, ca, cb)
        gr.assert_within(T.t[rows], t64, mass, gr.bf16_c(1), "%s, T_out of replica %d" % (what, r))
        _y_bound(Y.t[rows], T.t[rows], Wl, True, F_in, "%s, replica %d" % (what, r))
    # The fp32 call it is compared with reads X [N, 128] in fp32, 2.2 GB: beyond 2^31 bytes its pull hop 1 leaves the
    # streaming row gather (buffer descriptor) for the panel kernel, while the bf16 call's 1.1 GB X stays on it.  The two
    # then add the 699 members of the long hyperedge in different orders, and 22 of 555 M elements of T_out (members of
    # that hyperedge, spread over all replicas) round to the neighbouring bf16 value: measured, one bf16 unit each.  So
    # under "pull" both calls are pinned to the panel kernel (hop kernels 1, 1), where the documented equality holds.
    if variant == "pull":
        c.plan.pin(F_in, "pull", 4)
        T.refill()
        Y.refill()
        c.plan.aggregate_linear_bf16(c.ptr, c.ind, X, Wl, out=Y.t, workspace=ws.t, residual=R, t_out=T.t, **kw)
    T32 = torch.empty(c.N, F_in, device=DEV)
    try:
        c.plan.aggregate_linear(c.ptr, c.ind, X32, Wl.float(), residual=R32, t_out=T32, **kw)
    finally:
        c.plan.unpin(F_in)
    torch.cuda.synchronize()
    Y.check(what)
    T.check(what)
    assert torch.equal(_bits(T.t), _bits(T32.bfloat16())), what + ": T_out is not the fp32 bracket rounded once"
    c.plan.unbind()
    del X, R, X32, R32, T32, Y, T, ws
    torch.cuda.empty_cache()


# ---- 9. the neighbour-table gathers -------------------------------------------------------------------------------------------

def _close_b(y, ref, what):
    """test_table_gpu._assert_close: a deterministic kernel whose order may differ from the reference's."""
    y, ref = y.detach().cpu().numpy(), np.asarray(ref)
    assert (np.abs(y - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))).all() and np.allclose(y, ref, rtol=1e-4, atol=1e-6), what


def test_table_gathers_and_knn_aggr_at_E(hg, big):
    """table_gather, table_gather_t, knn_transpose and knn_aggr forward and backward over a block-diagonal table [K n0, 8]
    (rows * k far below 2^31; a synthetic table of random neighbours with a planted hub, not a searched one) with src, dst, X, Y and dX [K n0, 512] beyond 2^31 elements.  The base table has a hub in
    200 rows (beyond TABLE_SEQ_MAX: the long-row path of table_gather_t).  The transpose is exact; table_gather equals
    _table_ref.gather bit for bit; table_gather_t and knn_aggr lie within test_table_gpu's bound of the float64 result.
    The calls allocate their results: no guard bands.  Peak device memory: 37 GB."""
    import _table_ref as tr
    ops = hg.ops
    K, n0, k, F = big.K, 2050, 8, F_E
    n = K * n0
    assert n * F >= E31 and n * k < E31
    rng = np.random.default_rng(9)
    idx0 = rng.integers(0, n0, (n0, k)).astype(np.int32)
    idx0[rng.choice(n0, 200, replace=False), 3] = 17  # the hub
    assert np.bincount(idx0.reshape(-1), minlength=n0)[17] > hg.knn_graph.table_seq_max()
    idx = (torch.from_numpy(idx0).to(DEV)[None] + (torch.arange(K, device=DEV, dtype=torch.int32) * n0)[:, None, None]).reshape(n, k)
    ptr_v, pos_v = ops.knn_transpose(idx, n)
    ptr0, pos0 = tr.transpose(idx0, n0)
    # the scales of _table_ref.hub_operator_case, which test_table_gpu's bound is stated for: w in [0.5, 1.5), degE = 1 / k,
    # degV = in-degree^-1/2 (the kNN hypergraph's: they depend on the table alone); X and w are independent per replica
    g = torch.Generator(device=DEV).manual_seed(90)
    w = torch.rand(n * k, device=DEV, generator=g).add_(0.5)
    deg0 = np.bincount(idx0.reshape(-1), minlength=n0).astype(np.float64)
    degE = torch.full((n,), 1.0 / k, device=DEV)
    degV = torch.from_numpy(np.tile(np.where(deg0 > 0, np.maximum(deg0, 1) ** -0.5, 1.0).astype(np.float32), K)).to(DEV)
    X = lr.randn(n, F, seed=93)
    replicas = lr.picked(K, n0 * F)
    dst = hg.knn_graph.table_gather(idx, X, w, degV, degE)
    dst_t = hg.knn_graph.table_gather_t(ptr_v, pos_v, k, X, w, degE, degV)
    torch.cuda.synchronize()
    np_ = lambda t: t.cpu().numpy()  # noqa: E731
    for r in replicas:
        rows, ent = slice(r * n0, (r + 1) * n0), slice(r * n0 * k, (r + 1) * n0 * k)
        got_ptr = np_(ptr_v[r * n0:(r + 1) * n0 + 1])
        assert np.array_equal(got_ptr - r * n0 * k, ptr0) and np.array_equal(np_(pos_v[ent]) - r * n0 * k, pos0), r
        x, wr, e, v = np_(X[rows]), np_(w[ent]), np_(degE[rows]), np_(degV[rows])
        assert np.array_equal(np_(dst[rows]).view(np.int32), tr.gather(idx0, x, wr, v, e).view(np.int32)), "table_gather, replica %d" % r
        terms = (x.astype(np.float64) * e[:, None])[np.arange(n0 * k) // k] * wr[:, None].astype(np.float64)
        ref = np.zeros((n0, F))
        np.add.at(ref, idx0.reshape(-1), terms)
        _close_b(dst_t[rows], ref * v[:, None], "table_gather_t, replica %d" % r)
    del dst, dst_t
    X.requires_grad_(True)
    Y = ops.knn_aggr(idx, X, w, degE, degV, transpose=(ptr_v, pos_v))
    (dX,) = torch.autograd.grad(Y, X, X.detach())  # X's own values as the output gradient: no fifth array of 9 GB
    torch.cuda.synchronize()
    for r in replicas:
        rows, ent = slice(r * n0, (r + 1) * n0), slice(r * n0 * k, (r + 1) * n0 * k)
        x, wr, e, v = np_(X.detach()[rows]), np_(w[ent]), np_(degE[rows]), np_(degV[rows])
        _close_b(Y[rows], tr.aggr(idx0, x, wr, e, v), "knn_aggr, replica %d" % r)
        _close_b(dX[rows], tr.aggr_grad(idx0, x, wr, e, v), "knn_aggr backward, replica %d" % r)
    del X, Y, dX, w, idx, ptr_v, pos_v
    torch.cuda.empty_cache()


# ---- 10. the kNN searches -----------------------------------------------------------------------------------------------------

def test_knn_at_E(hg):
    """knn over X [32800, 65536] (beyond 2^31 elements; 65536 columns is the dot form's limit) for 24 queries, copies of the
    first and the last twelve rows: the difference form with cand_slices 0, 4 and 32 and form="dot".  The rows hold
    integers in -2 .. 2, so every distance is an integer below 2^24, exact in float32: idx and dist equal _knn_ref's (from
    float64 distances formed on the device) exactly, ties by index included, and the dot form equals the difference form
    bit for bit.  Peak device memory: 11 GB."""
    import _knn_ref as kr
    n, F, k = 32800, 65536, 16
    assert n * F >= E31 and 16 * F < 2 ** 24
    g = torch.Generator(device=DEV).manual_seed(100)
    X = torch.randint(-2, 3, (n, F), device=DEV, generator=g, dtype=torch.int8).float()
    Q = torch.cat([X[:12], X[-12:]]).clone()
    # integers: |q|^2 + |x|^2 - 2 q.x is exact in float64 (every partial sum an integer below 2^53) and equals the
    # difference form's sum
    D = torch.empty(Q.shape[0], n, dtype=torch.float64, device=DEV)
    Q64 = Q.double()
    for lo in range(0, n, 4096):
        blk = X[lo:lo + 4096].double()
        D[:, lo:lo + 4096] = (Q64 ** 2).sum(1)[:, None] + (blk ** 2).sum(1)[None, :] - 2.0 * (Q64 @ blk.t())
    ref_idx, ref_dist, _ = kr.knn(np.empty((n, 0)), k, np.empty((Q.shape[0], 0)), D=D.cpu().numpy())
    assert (ref_dist[:, 0] == 0).all() and set(ref_idx[:, 0]) == set(range(12)) | set(range(n - 12, n))
    base = None
    for form, slices in (("difference", 0), ("difference", 4), ("difference", 32), ("dot", 32)):
        idx, dist = hg.ops.knn(X, k, queries=Q, cand_slices=slices, form=form)
        torch.cuda.synchronize()
        what = "knn %s, cand_slices %d" % (form, slices)
        assert np.array_equal(idx.cpu().numpy(), ref_idx), what
        assert np.array_equal(dist.cpu().numpy().astype(np.float64), ref_dist), what
        if base is None:
            base = (idx, dist)
        assert torch.equal(idx, base[0]) and torch.equal(_bits(dist), _bits(base[1])), what
    del X, Q, Q64, D
    torch.cuda.empty_cache()
