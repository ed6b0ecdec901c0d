/*
 * hg_aggr.h -- C ABI of libhgaggr.so, the MI355X (gfx950) backend for the fused
 * vertex -> hyperedge -> vertex aggregation of HGNNConv / UniGNNConv.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.  It
 * is what the reference's operator layer binds instead of its CUDA launchers.
 * Each entry point cites the reference interface it replaces (paths relative
 * to the reference tree).  INTEGRATION.md shows the binding stubs.
 *
 * Conventions (reference: HyperGsys/include/util/check.cuh:11-12):
 *   Index = int32, DType = float32, feature matrices row-major [rows, F].
 *   H is the N x M vertex-by-hyperedge incidence matrix; the caller supplies
 *   H_T in CSR: csrptr_t[M+1], colind_t[nnz] (row = hyperedge, entries = member
 *   vertices), exactly the `H_T_csrptr` / `H_T_colind` tensors of
 *   HyperGsys/hypergraph.py:63-70.
 *
 * All device pointers must belong to the current HIP device.  Every function
 * returns HG_OK or a negative hg_status; nothing aborts, nothing throws.
 * hg_last_error() gives a thread-local message for the last failure.
 * Calls that take a stream only enqueue work on it; they do not synchronise.
 */
#ifndef HG_AGGR_H
#define HG_AGGR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HG_AGGR_VERSION 410 /* round 4: + hg_aggr_linear_res_dev_f32, HG_LIN_BF16X6 + hg_linear_pack_ex_f32 */

#if defined(__GNUC__)
#define HG_API __attribute__((visibility("default")))
#else
#define HG_API
#endif

typedef enum hg_status {
  HG_OK = 0,
  HG_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, bad CSR) */
  HG_ERR_NOMEM = -2,       /* host or device allocation failed */
  HG_ERR_HIP = -3,         /* a HIP runtime call or kernel launch failed */
  HG_ERR_WORKSPACE = -4,   /* caller workspace smaller than hg_plan_workspace_bytes */
  HG_ERR_UNSUPPORTED = -5  /* combination not implemented */
} hg_status;

typedef void *hg_stream_t; /* a hipStream_t; NULL = the legacy default stream */
typedef struct hg_plan hg_plan;

/* Kernel family used by hg_aggr_fused_f32. */
typedef enum hg_variant {
  HG_VARIANT_AUTO = 0,
  /* Atomic-free two-phase pull: Xe = S_e . (H^T X) over H_T CSR, then
   * Y = S_v . (H Xe) over H CSR.  Deterministic; bit-exact with the CPU
   * reference order for every row of at most `short_max` entries. */
  HG_VARIANT_PULL = 1,
  /* The reference's scheme (HGNNAggr_forward_kernel, hgnnaggr_cuda.cu:14-47):
   * hyperedge partial sum kept in registers, scattered with fp32 atomics. */
  HG_VARIANT_PUSH_ATOMIC = 2,
  /* Fused pull: vertex panels whose incident hyperedge sums are recomputed in
   * the workgroup and staged in LDS, so the M x F hyperedge feature matrix
   * never round-trips through HBM.  Hyperedges longer than t_big are materialised
   * by a pre-pass instead.  Vertices with more hyperedges than a panel holds are
   * cut into pieces (partial rows, summed by a fixup pass in a fixed order) or, the
   * heaviest ones of a large graph, served by the hub pass: persistent workgroups
   * that keep the hubs' running sums in registers while they stream the hyperedges,
   * each hyperedge sum computed once per pass however many hubs it feeds.
   * Rows of at most vdeg_max hyperedges keep HG_VARIANT_PULL's arithmetic order. */
  HG_VARIANT_FUSED = 3
} hg_variant;

typedef struct hg_plan_opts {
  int32_t short_max;  /* rows longer than this are cut out as wave tasks (default 32) */
  int32_t split_len;  /* a wave task covers at most this many entries (default 512)   */
  int32_t panel_rows; /* rows per row-panel workgroup (default 128)                   */
  int32_t panel_nnz;  /* index entries staged in LDS per panel (default 1024)         */
  int32_t flags;      /* HG_PLAN_* bits                                              */
  int32_t t_big;      /* fused: recompute hyperedges of at most this many members (8)  */
  int32_t fused_tile_bytes; /* fused: LDS tile budget per workgroup -> slots per panel (16384) */
  int32_t fused_steps; /* fused: a panel's hop-1 stream holds at most this many entries per lane group
                          (0 = 4 entries per slot on average); 8 = one batch of row loads in flight */
} hg_plan_opts;

#define HG_PLAN_HOST_ONLY 1 /* build the schedule on the host, upload nothing (tests) */
#define HG_PLAN_NO_XCD_REMAP 2 /* keep blockIdx -> panel identity mapping */
#define HG_PLAN_DFS_ORDER 4 /* fused: panel rows in plain depth-first order (no greedy growth) */
#define HG_PLAN_NO_ROW_STREAM 16 /* pull: always the general row-gather kernel (panels + wave tasks), never the streaming one */
#define HG_PLAN_NO_HUB_PASS 8 /* fused: no register-hub pass; every vertex too big for a panel is cut into pieces */

typedef struct hg_plan_info {
  int32_t N, M;
  int64_t nnz;
  int32_t short_max, split_len, panel_rows, panel_nnz, flags;
  /* hop 1 walks H_T (rows = hyperedges), hop 2 walks H (rows = vertices) */
  int32_t panels[2];   /* row panels                                   */
  int32_t tasks[2];    /* wave tasks for rows longer than short_max    */
  int32_t partials[2]; /* partial-sum slots of rows split over tasks   */
  int32_t fixups[2];   /* rows whose partials are summed in a 2nd pass */
  int32_t max_len[2];  /* longest row of each CSR                      */
  int64_t device_bytes; /* device memory held by the plan              */
} hg_plan_info;

/* Shape of the F-dependent fused schedule (hg_plan_prepare). */
typedef struct hg_fused_info {
  int32_t cap;      /* hyperedge slots (LDS tile rows) per vertex panel */
  int32_t t_big, vdeg_max;
  int32_t panels;
  int32_t n_mat;    /* materialised hyperedges */
  int32_t n_hub;    /* register hubs: running sums kept on chip by the hub pass */
  int64_t slots;    /* sum over panels of distinct hyperedges touched */
  int64_t member_entries; /* row gathers of one fused aggregation (panels only) */
  int32_t n_split;  /* vertices cut into pieces (panel rows that leave partial sums) */
  int32_t fixups;   /* rows summed from partial rows after the panels (hubs + split vertices) */
  int32_t hub_rounds, hub_workgroups; /* hub pass: rounds of hyperedge slots, persistent workgroups */
  int64_t hub_entries; /* row gathers of the hub pass */
  int64_t hub_pairs;   /* (hub, hyperedge) incidences served from the LDS tile */
  int64_t partial_rows; /* partial rows in the workspace (hub parts x workgroups + pieces) */
  int32_t record_words_max; /* largest panel record, 32-bit words (staged in LDS beside the tile) */
  int32_t stream_steps_max; /* longest entry stream of a panel: row gathers per lane group */
  int32_t lds_bytes;        /* LDS per panel workgroup without scale staging: tile + largest record */
  int32_t reserved;
} hg_fused_info;

HG_API int hg_version(void);
HG_API const char *hg_last_error(void);
HG_API const char *hg_status_string(int status);

/* ---- scheduler, reference-compatible ------------------------------------
 * Replaces balance_schedule (HyperGsys/balancer.py:4-33) and its C++ twin
 * hgnn_ef_full_balance_cpu (include/taskbalancer/balancer_kernel.cuh:229-259):
 * hyperedge r with n_r members is cut into w = ceil(n_r/ngs) partitions and
 * w*w (read j, write i) tasks, i outer / j inner; `key` holds the partition
 * starts plus a trailing nnz sentinel.  Host arrays in, host arrays out.
 * Two-call protocol: pass key == NULL to get *n_key / *n_group, then call
 * again with arrays of those lengths.  HG_ERR_INVALID when nnz == 0 (the
 * reference raises IndexError there). */
HG_API int hg_balance_schedule(int32_t nrow, int32_t ngs, const int32_t *csrptr_host,
                        int64_t *n_key, int64_t *n_group, int32_t *key,
                        int32_t *row, int32_t *group_st, int32_t *group_ed);

/* ---- input format ----------------------------------------------------------
 * MatrixMarket reader with the semantics of the reference's DataLoader
 * (include/dataloader/dataloader.hpp:22-180): 1-based `row col [value]` lines,
 * values dropped, entries sorted by (row, col); `symmetric` files are mirrored
 * and de-duplicated, `general` files keep duplicates.  Returns H (rows =
 * vertices) in CSR and its stable transpose H_T (rows = hyperedges, members
 * ascending).  The four arrays are malloc'ed; release each with hg_free. */
HG_API int hg_mtx_read(const char *path, int32_t *nrow, int32_t *ncol, int64_t *nnz,
                       int32_t **H_ptr, int32_t **H_ind, int32_t **HT_ptr, int32_t **HT_ind);
HG_API void hg_free(void *p);

/* ---- plan ------------------------------------------------------------------
 * The plan is this backend's own schedule (what hgnn_balancer,
 * include/taskbalancer/balancer.cuh:189-275, is to the reference kernels): it
 * derives H in CSR (vertex -> incident hyperedges, ascending) from H_T and
 * cuts both CSRs into row panels and wave tasks for 64-lane wavefronts.  It
 * depends only on the sparsity structure; build once per hypergraph, reuse for
 * every feature width and every call.  opts may be NULL (defaults). */
HG_API int hg_plan_create_host(hg_plan **out, int32_t N, int32_t M,
                        const int32_t *csrptr_t_host,
                        const int32_t *colind_t_host,
                        const hg_plan_opts *opts);
/* Same, from device arrays (copies them to the host on `stream`, synchronises
 * that stream once).  Not capturable into a hipGraph. */
HG_API int hg_plan_create_device(hg_plan **out, int32_t N, int32_t M, int64_t nnz,
                          const int32_t *csrptr_t_dev,
                          const int32_t *colind_t_dev,
                          const hg_plan_opts *opts, hg_stream_t stream);
HG_API void hg_plan_destroy(hg_plan *plan);
HG_API int hg_plan_get_info(const hg_plan *plan, hg_plan_info *info);
/* Host copy of the derived H CSR (tests / CLI): ptr_v[N+1], ind_v[nnz]. */
HG_API int hg_plan_get_vertex_csr(const hg_plan *plan, int32_t *ptr_v_host,
                           int32_t *ind_v_host);
/* Device pointers of the derived H CSR (valid for the plan's lifetime). */
HG_API int hg_plan_get_vertex_csr_device(const hg_plan *plan, const int32_t **ptr_v_dev,
                                  const int32_t **ind_v_dev);
/* Build (and upload) the part of the plan that depends on the feature width --
 * the fused variant's vertex panels -- ahead of time.  hg_aggr_fused_f32 does
 * this itself on first use of a width, but that first call allocates device
 * memory and so cannot be captured into a hipGraph.  info may be NULL. */
HG_API int hg_plan_prepare(const hg_plan *plan, int32_t F, hg_fused_info *info);
/* Optional: pre-gather the degree / weight vectors into the fused schedule's panel
 * order for feature width F.  Later hg_aggr_fused_f32 calls (fused variant) that pass
 * exactly these three pointers read the scales with coalesced loads instead of one
 * scattered 4-byte gather per hyperedge slot.  Re-bind after changing the vectors'
 * contents; passing other pointers simply bypasses the binding, and binding three NULL
 * pointers removes it (later calls gather their scales themselves: the safe choice for
 * vectors another library rewrites in place).  The binding is keyed on addresses only.
 * When W is given the call also checks once whether every W[e] is exactly 1.0f (what the
 * reference's models pass, model/ugsys/hgnn.py:12) and, if so, later calls skip that
 * multiplication -- the identity, bit for bit; this check synchronises `stream`.
 * Allocates on the first call per width (not capturable); enqueues one small kernel on
 * `stream` -- a caller that aggregates on a different stream orders the two itself. */
HG_API int hg_plan_bind_scales(const hg_plan *plan, int32_t F, const float *degE,
                               const float *degV, const float *W, hg_stream_t stream);
/* The variant HG_VARIANT_AUTO resolves to for feature width F (builds the
 * F-dependent schedule if the choice needs it); negative hg_status on error. */
HG_API int hg_plan_auto_variant(const hg_plan *plan, int32_t F);
/* Timed choice for feature width F, the counterpart of the reference's tuner (HyperGAggr_tune,
 * include/hgnnAgg.cuh:1115-1157: it times 20 partition sizes and keeps the fastest).  Runs the candidates on
 * the caller's buffers -- the fused schedule, and the pull variant with either kernel for each hop (streaming
 * row gather / panels + wave tasks) -- `iters` times each between two events on `stream`, waits for them, and
 * pins what HG_VARIANT_AUTO does for this width from then on.  Matters on launch-bound graphs (one dataset-sized
 * hypergraph), where the static rule cannot see which kernel's dependent round trips are shorter.  Same
 * arguments as hg_aggr_fused_f32 (Y ends up holding the result); workspace as after hg_plan_prepare.  The
 * candidates differ in summation order, so the low bits of later AUTO results depend on which one won; do not
 * call it while other threads use the plan.  info may be NULL. */
typedef struct hg_tune_info {
  int32_t variant;           /* HG_VARIANT_FUSED or HG_VARIANT_PULL */
  /* kernel of each pull hop (hop 0: vertices -> hyperedges), k0 + 3 * k1 with k = 0: streaming row gather,
   * 1: row panels + wave tasks, 2 (graphs of at most 2^18 incidences): the same kernel on the latency schedule --
   * every row of more than 8 entries is a wave task, its entries spread over the wave's lane groups and in
   * flight at once, instead of a chain of dependent load batches in one lane group */
  int32_t pull_hop_kernels;
  float us[10];              /* microseconds per call: fused, pull with hop kernels 0 .. 8 (negative: not run) */
  int32_t reserved;
} hg_tune_info;
HG_API int hg_plan_tune_f32(const hg_plan *plan, int32_t F, const int32_t *csrptr_t, const int32_t *colind_t,
                            const float *X, const float *degE, const float *degV, const float *W, float *Y,
                            void *workspace, size_t workspace_bytes, int32_t iters, hg_stream_t stream,
                            hg_tune_info *info);
/* The tuner's result without the timing: pins what HG_VARIANT_AUTO runs for feature width F, and the kernel of each
 * pull hop, to a choice the caller names -- yesterday's hg_tune_info, say, for the same bits today, or one candidate at a
 * time for a test that must know which kernel it checks.  variant is HG_VARIANT_FUSED or HG_VARIANT_PULL and
 * pull_hop_kernels is k0 + 3 * k1, both with the meaning of hg_tune_info; the pin holds for both alignment classes of the
 * width (rows that move as 16-byte lanes and rows that do not).  As after hg_plan_tune_f32, a forced HG_VARIANT_PULL,
 * hg_gather_rows_f32 and the bf16 call use the pinned hop kernels even where the pinned variant is fused, and the
 * incidence-weighted entries take the latency schedule where kernel 2 is pinned.  Kernel 0 falls through to kernel 1 where
 * the streaming row gather does not apply (F <= 8 with F % 4 != 0, HG_PLAN_NO_ROW_STREAM).  variant = HG_VARIANT_AUTO
 * removes the pin and the hop kernels of the width (pull_hop_kernels is ignored): the static rule decides again.
 * Only the plan's host state changes, under the lock that guards the AUTO choice: nothing is launched or allocated, and
 * host-only plans take the call.  A pinned HG_VARIANT_FUSED is not checked against the width here: where the fused
 * schedule cannot be built, the AUTO call that needs it returns that error.  Size the workspace after pinning
 * (hg_plan_workspace_bytes); do not call it while other threads run this width on the plan.
 * HG_ERR_INVALID, message through hg_last_error, plan unchanged: a null plan, F < 1, pull_hop_kernels outside 0 .. 8 or
 * naming kernel 2 on a plan without a latency schedule, any other variant (HG_VARIANT_PUSH_ATOMIC included).
 * hg_plan_has_latency_schedule: 1 where the plan carries the latency schedule kernel 2 runs on -- built for graphs of at
 * most 2^18 incidences whose short_max is above 8 -- else 0; negative hg_status for a null plan.
 * Detect these entries by their exported symbols (HG_AGGR_VERSION does not change). */
HG_API int hg_plan_set_choice(const hg_plan *plan, int32_t F, int32_t variant, int32_t pull_hop_kernels);
HG_API int hg_plan_has_latency_schedule(const hg_plan *plan);
/* Host copy of one hop's schedule as int32 quadruples (tests, tools): panels
 * {row0, nrows, nnz0, nnz_cnt}, tasks {row, beg, end, slot}, fixups {row,
 * first_slot, count, 0}; sizes from hg_plan_get_info.  Pointers may be NULL. */
HG_API int hg_plan_get_schedule(const hg_plan *plan, int32_t hop, int32_t *panels,
                                int32_t *tasks, int32_t *fixups);
/* Bytes of scratch hg_aggr_fused_f32 needs for feature width F, a multiple of 256: the larger
 * of the pull layout (the M x F hyperedge feature matrix plus partial-sum slots) and, once the
 * width's fused schedule exists, its layout (materialised rows, partial rows of hub vertices and
 * pieces).  The call resolves HG_VARIANT_AUTO for this width first -- building the fused schedule
 * on the host if that is the choice (once per width; milliseconds for dataset-sized graphs,
 * seconds for 10^7 incidences) -- so the size covers what an AUTO call will run.  A caller that
 * forces HG_VARIANT_FUSED on a plan whose AUTO choice is pull calls hg_plan_prepare first; a
 * fused call with a workspace sized before that returns HG_ERR_WORKSPACE, never writes past it. */
HG_API size_t hg_plan_workspace_bytes(const hg_plan *plan, int32_t F);

/* ---- the hot path ------------------------------------------------------------
 * Y[v,:] = degV[v] * sum_{e contains v} ( degE[e] * W[e] * sum_{u in e} X[u,:] )
 *
 * Replaces hgnnaggr_fp_cuda (source/hgnnaggr/hgnnaggr_cuda.cu:350-406),
 * unignnaggrdeg / unignnaggr launchers (source/unignnaggr/unignnaggr_cuda.cu:
 * 392-488) and HyperGAggr_device (include/hgnnAgg.cuh:985-1038).
 *   degE, W : [M] or NULL (factor 1);  degV : [N] or NULL.
 *     hgnnaggr      -> degE, degV, W      unignnaggrdeg -> degE, degV, W = NULL
 *     unignnaggr / aggr_proto kernels -> all three NULL
 *   Arithmetic order is the reference test's (test/hgnn_test.py:56-63):
 *     Xe = ((sum X) * degE) * W ;  Y = (sum Xe) * degV.
 *   Y is fully overwritten (no pre-zeroing needed); inputs are not modified.
 *   X, Y: row-major [N, F], any F >= 1, 4-byte aligned (16-byte alignment and F % 4 == 0 are not required:
 *   rows of more than 8 floats move as 16-byte lanes either way).
 *   workspace: device scratch of at least hg_plan_workspace_bytes(plan, F),
 *   256-byte aligned, private to this call until it completes on `stream`.
 *   csrptr_t / colind_t must be the arrays the plan was built from. */
HG_API int hg_aggr_fused_f32(const hg_plan *plan, int32_t F,
                      const int32_t *csrptr_t, const int32_t *colind_t,
                      const float *X, const float *degE, const float *degV,
                      const float *W, float *Y, void *workspace,
                      size_t workspace_bytes, int32_t variant,
                      hg_stream_t stream);

/* The same aggregation with X and Y in bf16 (bit patterns, row-major [N, F]); the arguments are those of
 * hg_aggr_fused_f32 and the call takes the same plan, scale vectors, workspace and stream.
 * Numerical contract:
 *   degE, degV, W stay fp32.  Everything between X and Y is fp32: the LDS hyperedge tile, the materialised
 *   hyperedge table, the partial rows of split vertices and of the hub pass, the workspace.  Each element is
 *   accumulated in fp32 in exactly the order the fp32 call uses and rounded to bf16 once, to nearest even
 *   (NaN stays NaN: the rounding of torch's .to(torch.bfloat16)).  The call runs the schedule and the AUTO
 *   choice of an fp32 call of the same width and builds none of its own.  bf16 -> fp32 is exact, so for
 *   X below 2 GiB as fp32:
 *     hg_aggr_fused_bf16(X)  ==  round_bf16(hg_aggr_fused_f32(fp32(X)))   bit for bit,
 *   any shape, weighted or not, HG_VARIANT_AUTO / FUSED / PULL.
 *   The workspace is the fp32 call's: hg_plan_workspace_bytes answers for both forms.
 * Returns HG_ERR_UNSUPPORTED (message through hg_last_error) for HG_VARIANT_PUSH_ATOMIC, F % 4 != 0, or X / Y
 * not 8-byte aligned; a caller pads narrower rows with zero columns.  Detect it by the exported symbol
 * (HG_AGGR_VERSION does not change). */
HG_API int hg_aggr_fused_bf16(const hg_plan *plan, int32_t F,
                      const int32_t *csrptr_t, const int32_t *colind_t,
                      const uint16_t *X, const float *degE, const float *degV,
                      const float *W, uint16_t *Y, void *workspace,
                      size_t workspace_bytes, int32_t variant,
                      hg_stream_t stream);

/* Aggregation with the layer's dense projection folded in: the
 * reference's HyperGsysHGNN / HyperGsysUinGINConv.forward run `X = self.W(X)` (nn.Linear
 * without bias, model/ugsys/hgnn.py:22-23, unigin.py:20-21) and then the aggregation on
 * the projected rows.  The aggregation is linear, so
 *     Y[N, F_out] = Aggr(X * Wlin^T) = Aggr(X) * Wlin^T
 * and this entry point aggregates the F_in-wide rows once and multiplies each finished
 * row by Wlin^T on the matrix cores (v_mfma_f32_16x16x4_f32, exact fp32) before it is
 * stored: X is read once and Y written once, the projected matrix never exists in HBM.
 * Results equal the two-step form up to fp32 rounding order (both are fp32 fma chains).
 *   Wlin   : [F_out, F_in] row-major device array (nn.Linear.weight)
 *   wfrag  : F_out * F_in floats, 16-byte aligned: Wlin in MFMA fragment order.  Fill it with
 *            hg_linear_pack_f32 after every weight update.  A wave keeps the fragments of
 *            its output-column tile in registers; in this order they are K/16 coalesced
 *            16-byte reads per lane (read from the row-major matrix they would touch more
 *            cache lines per panel than the whole gather of X)
 *   F_in in {32, 64, 128}; F_out a positive multiple of 16 (else HG_ERR_UNSUPPORTED and
 *   the caller runs its own linear followed by hg_aggr_fused_f32)
 * Where the fused panels cannot take the epilogue (pull variant, hub vertices) the
 * aggregated rows go to the workspace and a standalone MFMA kernel projects them; the
 * workspace is therefore hg_aggr_linear_workspace_bytes, not hg_plan_workspace_bytes. */
HG_API int hg_linear_pack_f32(int32_t F_out, int32_t F_in, const float *Wlin, float *wfrag,
                              hg_stream_t stream);
/* Flags of the `relu` argument of hg_aggr_linear_res(_dev)_f32 (bit 0 is the activation, as before).
 * HG_LIN_BF16X6: the fused panels' matrix phase at F_in = 128 may compute every fp32 product as six bf16
 * products (x = h + m + l in bf16 up to 2^-24 |x|, bf16 x bf16 is exact in fp32, the pipe accumulates in fp32;
 * the three smallest cross terms, < 2^-23 |a b|, are dropped -- below one rounding of the fp32 product) on
 * v_mfma_f32_16x16x32_bf16: 3/8 of the matrix-pipe cycles of the fp32 form, the same error bound
 * (tests: both forms within 1e-5 x row mass of the float64 answer; measured maxima side by side in DESIGN.md).
 * The caller then passes a wfrag of hg_linear_pack_floats(F_out, F_in, HG_LIN_BF16X6) floats filled by
 * hg_linear_pack_ex_f32 with the same flag: the fp32 fragments (hub vertices, the other variants and every
 * other width still use them) followed by Wlin's three bf16 planes.  Without the flag nothing changes.
 * Range: bf16 keeps fp32's exponent, so finite operands below 2^127 in magnitude behave as in the fp32 form;
 * an infinite operand (or one that rounds to infinity in bf16) yields NaN where the fp32 form yields +-inf. */
#define HG_LIN_RELU 1
#define HG_LIN_BF16X6 2
HG_API size_t hg_linear_pack_floats(int32_t F_out, int32_t F_in, int32_t flags);
HG_API int hg_linear_pack_ex_f32(int32_t F_out, int32_t F_in, const float *Wlin, float *wfrag, int32_t flags,
                                 hg_stream_t stream);
HG_API size_t hg_aggr_linear_workspace_bytes(const hg_plan *plan, int32_t F_in);
/* The same pass with a whole UniGNN layer folded in.  For every vertex v
 *     t     = ca * Aggr(X)[v] + cb * R[v]          (R NULL: t = ca * Aggr(X)[v])
 *     T_out[v] = t                                  (if T_out != NULL; the backward pass needs it)
 *     Y[v]  = act(t * Wlin^T),  act = relu if (relu & HG_LIN_RELU) else identity; relu & HG_LIN_BF16X6: see above
 * R and T_out are [N, F_in] row-major, 16-byte aligned.  This is one HyperGsysUniGCNII layer
 * (model/ugsys/unigcnii.py:19-21 with the relu of model/gnn.py:199): Xi = (1-alpha) Xv + alpha X0,
 * out = (1-beta) Xi + beta W(Xi) = Xi * ((1-beta) I + beta W)^T -- pack that matrix as wfrag --
 * and one HyperGsysUinGINConv layer (unigin.py:20-22): (1+eps) W(X) + Aggr(W(X)) =
 * ((1+eps) X + Aggr(X)) * W^T.  Arithmetic: the two products and the sum of t are separate fp32
 * operations in that order, then the MFMA fma chain; the value equals the reference's layer up
 * to fp32 rounding order. */
HG_API int hg_aggr_linear_res_f32(const hg_plan *plan, int32_t F_in, int32_t F_out,
                                  const int32_t *csrptr_t, const int32_t *colind_t, const float *X,
                                  const float *degE, const float *degV, const float *W,
                                  const float *wfrag, const float *R, float ca, float cb, int32_t relu,
                                  float *T_out, float *Y, void *workspace, size_t workspace_bytes,
                                  int32_t variant, hg_stream_t stream);
/* hg_aggr_linear_res_f32 with cb read from device memory when the kernel runs (cb_dev: one float, not NULL): for a
 * LEARNED scalar -- UniGIN's 1 + eps (unigin.py:14,22) -- the caller neither reads the value back to the host
 * (a device-to-host sync per layer and step) nor bakes it into a captured hipGraph. */
HG_API int hg_aggr_linear_res_dev_f32(const hg_plan *plan, int32_t F_in, int32_t F_out,
                                      const int32_t *csrptr_t, const int32_t *colind_t, const float *X,
                                      const float *degE, const float *degV, const float *W,
                                      const float *wfrag, const float *R, float ca, const float *cb_dev,
                                      int32_t relu, float *T_out, float *Y, void *workspace,
                                      size_t workspace_bytes, int32_t variant, hg_stream_t stream);
/* The linear's weight gradient, C[F_a, F_b] = A^T B with A [nrows, F_a], B [nrows, F_b] row-major:
 * dWlin = dY^T T in the backward pass of the layers above (the contraction runs over the vertices).
 * Every element of A and B is read once, straight into fp32 MFMA operands; workgroups are reduced
 * in a fixed order (deterministic).  F_a, F_b multiples of 16 with F_a * F_b <= 4096 -- one workgroup's
 * accumulators hold the whole output -- or both multiples of 64 up to 512: 64 x 64 blocks of the output as
 * independent contractions over the same rows (128 x 128: 3 x rocBLAS).  Else
 * HG_ERR_UNSUPPORTED: use a BLAS.  workspace = hg_linear_wgrad_workspace_bytes (0 = unsupported shape). */
HG_API size_t hg_linear_wgrad_workspace_bytes(int64_t nrows, int32_t F_a, int32_t F_b);
HG_API int hg_linear_wgrad_f32(int64_t nrows, int32_t F_a, int32_t F_b, const float *A, const float *B,
                               float *C, void *workspace, size_t workspace_bytes, hg_stream_t stream);
/* The projection alone, Y[nrows, F_out] = T[nrows, F_in] * Wlin^T, on the same MFMA kernel the
 * fallback path of hg_aggr_linear_f32 uses (same width limits, same packed wfrag). */
HG_API int hg_linear_rows_f32(int64_t nrows, int32_t F_in, int32_t F_out, const float *T,
                              const float *wfrag, float *Y, hg_stream_t stream);
HG_API int hg_aggr_linear_f32(const hg_plan *plan, int32_t F_in, int32_t F_out,
                              const int32_t *csrptr_t, const int32_t *colind_t, const float *X,
                              const float *degE, const float *degV, const float *W,
                              const float *wfrag, float *Y, void *workspace, size_t workspace_bytes,
                              int32_t variant, hg_stream_t stream);

/* The same layer on bf16 rows, its linear on the bf16 MFMA (v_mfma_f32_16x16x32_bf16) with fp32 accumulation.
 * X, R, T_out [N, F_in] and Y [N, F_out] are bf16 (bit patterns); Wlin [F_out, F_in] is bf16 and reaches the kernels
 * packed: hg_linear_pack_bf16 writes hg_linear_pack_bf16_bytes(F_out, F_in) = 2 F_out F_in bytes (0 for widths the
 * entries do not take) into wfrag.  degE, degV and W stay fp32.  F_in in {32, 64, 128}, F_out a positive multiple of 16.
 * The call runs the variant (the AUTO choice included) and the schedule hg_aggr_linear_res_f32 runs for the same
 * widths, with its hg_plan_bind_scales binding, and takes the same workspace, hg_aggr_linear_workspace_bytes(plan, F_in).
 * cb_dev != NULL overrides cb (a device scalar, as in hg_aggr_linear_res_dev_f32).  flags: HG_LIN_RELU or 0.
 *
 * Numerical contract.  With t32 the combined fp32 row ca * Aggr(X) + cb * R of hg_aggr_linear_res_f32 on the widened X
 * and R (same plan, variant, ca, cb):
 *   T_out[v] == round_bf16(t32[v]) bit for bit (round to nearest even, once);
 *   Y[v, n]  =  round_bf16(act(sum_k T_out[v, k] * Wb[n, k])): the products are exact in fp32, the sum is accumulated in
 *               fp32 in an order that depends on the plan and the widths only -- two calls give the same bits -- and the
 *               result is rounded to bf16 once, after the optional relu;
 *   a vertex in no hyperedge, with R == NULL, gives Y[v, :] = +0.
 * Non-finite operands are not special-cased: a NaN or infinity in X or R reaches T_out as round_bf16 leaves it (NaN stays
 * NaN, a finite fp32 value above bf16's range becomes infinity) and spreads to every Y[v, :] of its row through the
 * products (inf * 0 = NaN); relu maps NaN to 0, as the fp32 entry's does.  Rows of other vertices are not affected.
 *
 * Refusals launch nothing, set hg_last_error, and are decided in this order: HG_ERR_INVALID for a null plan, csrptr_t,
 * colind_t (nnz > 0), X, wfrag or Y, or for a flag other than HG_LIN_RELU; HG_ERR_UNSUPPORTED for
 * HG_VARIANT_PUSH_ATOMIC (or an unknown variant), for F_in outside {32, 64, 128} and for F_out % 16 != 0;
 * HG_ERR_UNSUPPORTED when X, Y, R or T_out is not 8-byte aligned or wfrag not 16-byte aligned; HG_ERR_UNSUPPORTED for a
 * plan built with HG_PLAN_HOST_ONLY; HG_ERR_WORKSPACE for a null, too small or not 16-byte aligned workspace.
 *
 * hg_aggr_linear_bf16_path tells which kernels such a call runs, as a bit mask: 1 = the fused panels run the epilogue
 * themselves (F_in = 128, F_out <= 128, fused variant, panels of at most 32 rows); 2 = some or all rows -- every row at
 * F_in = 32 / 64 and on the pull variant, hub and split vertices otherwise -- are aggregated in fp32 and go through the
 * rows kernel of hg_linear_rows_bf16.  A negative value is an hg_status.  It may build the schedule (host work), launches
 * nothing, and works on a host-only plan.
 * hg_linear_rows_bf16: Y[nrows, F_out] = round_bf16(T[nrows, F_in] . Wb^T) on that kernel; T and Y 8-byte aligned. */
HG_API size_t hg_linear_pack_bf16_bytes(int32_t F_out, int32_t F_in);
HG_API int hg_linear_pack_bf16(int32_t F_out, int32_t F_in, const uint16_t *Wlin, void *wfrag, hg_stream_t stream);
HG_API int hg_aggr_linear_res_bf16(const hg_plan *plan, int32_t F_in, int32_t F_out, const int32_t *csrptr_t,
                                   const int32_t *colind_t, const uint16_t *X, const float *degE, const float *degV,
                                   const float *W, const void *wfrag, const uint16_t *R, float ca, float cb,
                                   const float *cb_dev, int32_t flags, uint16_t *T_out, uint16_t *Y, void *workspace,
                                   size_t workspace_bytes, int32_t variant, hg_stream_t stream);
HG_API int hg_linear_rows_bf16(int64_t nrows, int32_t F_in, int32_t F_out, const uint16_t *T, const void *wfrag,
                               uint16_t *Y, hg_stream_t stream);
HG_API int hg_aggr_linear_bf16_path(const hg_plan *plan, int32_t F_in, int32_t F_out, int32_t variant);

/* One hop only (CSR times dense with unit values, optional row scales):
 *   dst[r,:] = scaleB[r] * scaleA[r] * sum_{p in row r} src[ind[p],:]
 * hop = 0 walks H_T (nrows = M, src has N rows), hop = 1 walks the derived H
 * (nrows = N, src has M rows).  The two-step comparator and tests use it; it
 * is the own-kernel counterpart of csrspmm_cusparse (include/spmm/spmm.cuh:
 * 22-77). */
HG_API int hg_gather_rows_f32(const hg_plan *plan, int32_t hop, int32_t F,
                       const int32_t *csrptr_t, const int32_t *colind_t,
                       const float *src, const float *scaleA,
                       const float *scaleB, float *dst, void *workspace,
                       size_t workspace_bytes, hg_stream_t stream);

/* ---- incidence-weighted aggregation ---------------------------------------------------------------------
 * A weight per (vertex, hyperedge) pair: a probabilistic incidence matrix h(v, e) (HGNN), or hypergraph attention's
 * coefficients a(v, e), learned, in both hops.  For the H_T entries p = (e, u) (the layout of csrptr_t / colind_t):
 *     Xe[e] = ((sum_{p=(e,u)} v2e[p] * X[u]) * degE[e]) * W[e]          (hop 1, walks H_T)
 *     Y[v]  =  (sum_{p=(e,v)} e2v[p] * Xe[e]) * degV[v]                 (hop 2, walks H)
 *   v2e_val, e2v_val: fp32 [nnz] aligned with colind_t, or NULL (unit weights); the same array twice for a symmetric
 *   weighting.  degE / degV / W as in hg_aggr_fused_f32 (degE = inf on an empty hyperedge is never applied).
 *   Arithmetic: the unweighted pull variant's order on its panels + wave-task kernel, each gathered row added as
 *   fma(row, weight, sum).  With both weight pointers NULL the call is that unweighted pull, bit for bit.
 *   Xe_out: [M, F] or NULL; receives hop 1's table (a backward pass needs it).  X, Xe_out, Y: any F >= 1, 4-byte aligned.
 *   workspace: hg_aggr_incidence_workspace_bytes(plan, F) (the pull layout), 256-byte aligned.
 *   Hop 2 reads e2v through the plan's permutation of H entries to H_T positions (hg_plan_get_incidence_perm), built
 *   and uploaded by the first call that passes e2v_val: that call allocates, so it cannot be captured into a hipGraph.
 *   Make one such call before capturing (hg_plan_get_incidence_perm alone does not do: it uploads nothing), as
 *   hg_plan_prepare is called before capturing hg_aggr_fused_f32.  Later calls only enqueue.
 *   HG_ERR_UNSUPPORTED where panel_rows / panel_nnz leave no LDS for the staged weights.
 * hg_incidence_dot_f32: out[p] = <A[u, :], B[e, :]> for every H_T entry p = (e, u): the weight gradient (A [N, F],
 *   B [M, F], out [nnz]).  Work is cut by entries; every output is reduced by one lane group in a fixed order
 *   (deterministic).
 * hg_plan_get_incidence_perm: host copy of perm[q] = H_T position of H entry q (the stable transpose behind
 *   hg_plan_get_vertex_csr, so ind_v[q] is the hyperedge holding position perm[q]); host-only plans too.
 * Detect these entries by their exported symbols (HG_AGGR_VERSION does not change). */
HG_API size_t hg_aggr_incidence_workspace_bytes(const hg_plan *plan, int32_t F);
HG_API int hg_aggr_incidence_f32(const hg_plan *plan, int32_t F, const int32_t *csrptr_t, const int32_t *colind_t,
                                 const float *X, const float *v2e_val, const float *e2v_val,
                                 const float *degE, const float *degV, const float *W,
                                 float *Xe_out, float *Y, void *workspace, size_t workspace_bytes, hg_stream_t stream);
HG_API int hg_incidence_dot_f32(const hg_plan *plan, int32_t F, const int32_t *csrptr_t, const int32_t *colind_t,
                                const float *A, const float *B, float *out, hg_stream_t stream);
HG_API int hg_plan_get_incidence_perm(const hg_plan *plan, int32_t *perm_host);

/* ---- hypergraph attention coefficients ------------------------------------------------------------------------------
 * The weights hg_aggr_incidence_f32 takes, computed where they are used: a score per incidence, normalised by a softmax
 * over each hyperedge's members or over each vertex's hyperedges.  Single head, fp32.  For every H_T entry p = (e, u):
 *     raw[p]   = sv[u] + se[e]                              sv: [N] or NULL (0), se: [M] or NULL (0)
 *     s[p]     = raw[p] > 0 ? raw[p] : slope * raw[p]       (leaky relu; slope = 1: the identity)
 *     alpha[p] = exp(s[p] - m_g) / sum_{q in g} exp(s[q] - m_g),   m_g = max_{q in g} s[q]
 *   group = 0: g is the hyperedge of p (a row of H_T); group = 1: g is the vertex of p (a row of H, reached through the
 *   plan's permutation).  alpha_out: [nnz] in H_T order, ready to be passed as v2e_val / e2v_val.  Positions exist only
 *   inside non-empty groups, so an empty group writes nothing; a group of one entry gives exactly 1.0f; the maximum is
 *   subtracted before the exponential, so finite scores of any magnitude give finite coefficients.
 * hg_incidence_attention_bwd_f32: given alpha (the forward's output) and dalpha, both [nnz] in H_T order,
 *     t_g = sum_{q in g} alpha[q] * dalpha[q],   ds[p] = alpha[p] * (dalpha[p] - t_g) * (raw[p] > 0 ? 1 : slope)
 *   ds_out: [nnz], H_T order, required (the sums below are formed from it).  dsv_out: [N] or NULL, dsv[v] = sum of ds
 *   over v's incidences; dse_out: [M] or NULL, dse[e] = sum of ds over e's members.  Both are fully overwritten (0 for a
 *   vertex in no hyperedge / an empty hyperedge).  sv / se are read only when slope != 1.
 * hg_incidence_sum_f32: the segment sum alone, out[e] = sum_{p in H_T row e} val[p] (side = 0, out [M]) or
 *   out[v] = sum over the H_T positions p of vertex v of val[p] (side = 1, out [N]); val [nnz] in H_T order.  The
 *   weighted degrees d(v) = sum_e w(e) h(v, e), delta(e) = sum_v h(v, e) of a probabilistic H are such sums.
 * All three: no atomics; every group is reduced by one lane group (or, above 128 entries, one workgroup) in an order that
 *   depends on the plan alone, so two calls give the same bits.  csrptr_t / colind_t must be the arrays the plan was built
 *   from.  The first call that needs the permutation (group / side = 1, or a gradient for the other end of the group) or
 *   a side's list of long rows builds and uploads it: that call allocates, so it cannot be captured into a hipGraph --
 *   make one call of the same form before capturing, as for hg_aggr_incidence_f32.  Later calls only enqueue.
 *   HG_ERR_UNSUPPORTED on a plan built with HG_PLAN_HOST_ONLY; HG_ERR_INVALID (message through hg_last_error, nothing
 *   launched) for a null plan or array, a group / side other than 0 / 1, a non-finite slope.
 * hg_plan_get_segment_info: how the segment kernels cut one side (tests, tools; host-only plans too): info[4] = {lanes per
 *   group, entries a lane keeps in registers, longest row a lane group takes, rows longer than that}; long_seg_host
 *   (NULL, or room for info[3] ids from a first call) receives those rows, ascending.
 * Detect these entries by their exported symbols (HG_AGGR_VERSION does not change). */
HG_API int hg_incidence_attention_f32(const hg_plan *plan, int32_t group, const int32_t *csrptr_t, const int32_t *colind_t,
                                      const float *sv, const float *se, float slope, float *alpha_out, hg_stream_t stream);
HG_API int hg_incidence_attention_bwd_f32(const hg_plan *plan, int32_t group, const int32_t *csrptr_t,
                                          const int32_t *colind_t, const float *sv, const float *se, float slope,
                                          const float *alpha, const float *dalpha, float *ds_out, float *dsv_out,
                                          float *dse_out, hg_stream_t stream);
HG_API int hg_incidence_sum_f32(const hg_plan *plan, int32_t side, const int32_t *csrptr_t, const int32_t *colind_t,
                                const float *val, float *out, hg_stream_t stream);
HG_API int hg_plan_get_segment_info(const hg_plan *plan, int32_t side, int32_t *info, int32_t *long_seg_host);

/* ---- several heads ---------------------------------------------------------------------------------------------------
 * The incidence path with `heads` = H attention heads in one call each, fp32.  Layout everywhere: the head is the fastest
 * index.  Scores are [N, H] / [M, H]; everything per incidence (alpha, dalpha, ds, val, v2e_val, e2v_val, the dot's out) is
 * [nnz, H], row p aligned with colind_t[p]; feature rows are F = H * C wide and head h owns columns h * C .. (h + 1) * C - 1.
 * heads = 1 is the single-head layout and runs the single-head entry's code: the same bits.
 * hg_incidence_attention_heads_f32 / _bwd_f32 / hg_incidence_sum_heads_f32: for every head h the contract of the single-head
 *   entry on column h of the score and entry arrays (dsv_out [N, H], dse_out [M, H], out [M, H] or [N, H]).  A lane group
 *   (above 128 entries: a workgroup) reduces one (group, head) pair in the single-head order, which depends on the group's
 *   length and the side's lane-group width, not on H: column h of a result has the bits of the single-head call on the
 *   contiguous column h of the inputs.  No atomics; one launch per body.
 * hg_aggr_incidence_heads_f32: hg_aggr_incidence_f32 with a weight per incidence and head,
 *     Xe[e, c] = ((sum_{p=(e,u)} v2e[p, c / C] * X[u, c]) * degE[e]) * W[e],   Y[v, c] = (sum_{p=(e,v)} e2v[p, c / C] * Xe[e, c]) * degV[v]
 *   on the same schedule, walk and fma order: the columns of head h equal, bit for bit, those of the single-head call of
 *   the same F with v2e_val = v2e[:, h], e2v_val = e2v[:, h].  Lanes are 16 bytes wide where the single-head call's are and
 *   C % 4 == 0 (a lane must lie inside one head), else 4 bytes.  Workspace: hg_aggr_incidence_workspace_bytes(plan, F).
 *   The weights are read from global memory where they lie (4 H contiguous bytes per incidence), not staged, so the LDS
 *   need does not depend on H: HG_ERR_UNSUPPORTED exactly where hg_aggr_incidence_f32 returns it.
 * hg_incidence_dot_heads_f32: out[p, h] = <A[u, hC .. (h+1)C), B[e, hC .. (h+1)C)> for every H_T entry p = (e, u), out
 *   [nnz, H]; each output is reduced by the lanes of its own head in a fixed order.
 * Limits: any 1 <= heads with F % heads == 0 (there is no upper limit short of nnz * heads < 2^40).  Refusals, nothing
 *   launched, message through hg_last_error: HG_ERR_INVALID for heads < 1 or F % heads != 0; HG_ERR_UNSUPPORTED for a plan
 *   built with HG_PLAN_HOST_ONLY; otherwise the single-head entries' rules.  The first-call-allocates rule is theirs too;
 *   the permutation and the long-row lists are shared with the single-head calls.
 * Detect these entries by their exported symbols (HG_AGGR_VERSION does not change). */
HG_API int hg_incidence_attention_heads_f32(const hg_plan *plan, int32_t group, int32_t heads, const int32_t *csrptr_t,
                                            const int32_t *colind_t, const float *sv, const float *se, float slope,
                                            float *alpha_out, hg_stream_t stream);
HG_API int hg_incidence_attention_heads_bwd_f32(const hg_plan *plan, int32_t group, int32_t heads, const int32_t *csrptr_t,
                                                const int32_t *colind_t, const float *sv, const float *se, float slope,
                                                const float *alpha, const float *dalpha, float *ds_out, float *dsv_out,
                                                float *dse_out, hg_stream_t stream);
HG_API int hg_incidence_sum_heads_f32(const hg_plan *plan, int32_t side, int32_t heads, const int32_t *csrptr_t,
                                      const int32_t *colind_t, const float *val, float *out, hg_stream_t stream);
HG_API int hg_aggr_incidence_heads_f32(const hg_plan *plan, int32_t F, int32_t heads, const int32_t *csrptr_t,
                                       const int32_t *colind_t, const float *X, const float *v2e_val, const float *e2v_val,
                                       const float *degE, const float *degV, const float *W, float *Xe_out, float *Y,
                                       void *workspace, size_t workspace_bytes, hg_stream_t stream);
HG_API int hg_incidence_dot_heads_f32(const hg_plan *plan, int32_t F, int32_t heads, const int32_t *csrptr_t,
                                      const int32_t *colind_t, const float *A, const float *B, float *out,
                                      hg_stream_t stream);

/* ---- attention dropout ------------------------------------------------------------------------------------------------
 * Dropout on the attention coefficients, fused into the softmax and its backward: no stored mask, no further pass over
 * the [nnz, heads] array.  With a[p, h] the coefficient hg_incidence_attention_heads_f32 computes for H_T position p and
 * head h, p_drop in [0, 1) and the 128-bit state rng = {key, sid} (two uint64 in device memory):
 *     w         = philox4x32_10(counter = (p, h, sid_lo, sid_hi), key = (key_lo, key_hi))[0]      (Random123's Philox)
 *     keep      = w >= T,   T = (uint32) floor((double) p_drop * 2^32)
 *     scale     = 1.0f / (1.0f - p_drop)                                                   (fp32, rounded on the host)
 *     alpha_drop_out[p, h] = keep ? fl(a[p, h] * scale) : +0.0f,     alpha_out[p, h] = a[p, h]
 *   alpha_out has the bits hg_incidence_attention_heads_f32 writes for the same scores: the backward needs the undropped
 *   coefficient at the dropped positions too.  The mask depends on (rng, p, h) alone -- not on group, on the lane-group
 *   width or on the lane that owns the entry -- so both groups drop the same positions for the same state.
 * hg_incidence_attention_dropout_heads_bwd_f32: given alpha (alpha_out above) and dout, the gradient of alpha_drop_out,
 *     dalpha[p, h] = keep ? fl(dout[p, h] * scale) : +0.0f
 *   with the mask regenerated from rng_dev, then exactly hg_incidence_attention_heads_bwd_f32 on (alpha, dalpha): the same
 *   t_g, ds, dsv, dse in the same order, so the results have the bits of that entry on the pre-masked gradient.
 * rng_dev: two uint64 {key, sid}, 8-byte aligned, read by the kernel when it runs -- not by the call.  A launch captured
 *   into a hipGraph therefore draws a new mask on every replay whose state was updated in between (by a captured device
 *   operation, say), as cb_dev of hg_aggr_linear_res_dev_f32 lets a captured step change its coefficient.  The backward
 *   must find the words its forward found.
 * heads = 1 is the single-head layout.  Refusals (nothing launched, message through hg_last_error): HG_ERR_INVALID for
 *   p_drop outside [0, 1) or NaN, for a null (or misaligned) rng_dev, a null alpha_out, alpha_drop_out or ds_out;
 *   otherwise the rules of the *_heads_f32 entries above (HG_ERR_UNSUPPORTED for a plan built with HG_PLAN_HOST_ONLY,
 *   heads < 1, ...).  The first-call-allocates rule is theirs, and what is allocated is shared with them.
 * hg_dropout_keep_host: the mask itself, on the host, from the same source as the kernels: keep_out[p * heads + h] = 1
 *   where (p, h) is kept, else 0, for p < nnz (< 2^31).  Needs neither a plan nor a device (tools, tests).
 * Detect these entries by their exported symbols (HG_AGGR_VERSION does not change). */
HG_API int hg_incidence_attention_dropout_heads_f32(const hg_plan *plan, int32_t group, int32_t heads,
                                                    const int32_t *csrptr_t, const int32_t *colind_t, const float *sv,
                                                    const float *se, float slope, float p_drop, const uint64_t *rng_dev,
                                                    float *alpha_out, float *alpha_drop_out, hg_stream_t stream);
HG_API int hg_incidence_attention_dropout_heads_bwd_f32(const hg_plan *plan, int32_t group, int32_t heads,
                                                        const int32_t *csrptr_t, const int32_t *colind_t, const float *sv,
                                                        const float *se, float slope, float p_drop, const uint64_t *rng_dev,
                                                        const float *alpha, const float *dout, float *ds_out,
                                                        float *dsv_out, float *dse_out, hg_stream_t stream);
HG_API int hg_dropout_keep_host(uint64_t key, uint64_t sid, float p_drop, int64_t nnz, int32_t heads, uint8_t *keep_out);

/* ---- a logit per incidence ------------------------------------------------------------------------------------------------
 * The softmax entries above form raw = sv[u] + se[e] themselves, so a score must split into a vertex term plus a hyperedge
 * term.  These take one more input, entry_score [nnz, heads] in H_T order (row p aligned with colind_t[p], head fastest):
 *     raw[p, h] = (sv[u, h] + se[e, h]) + entry_score[p, h]          the bracket is formed first; a NULL sv / se adds +0
 *   and are the *_heads_f32 / *_dropout_heads_f32 entries from there on: leaky relu, maximum, exponentials, order of
 *   reduction, rows above 128 entries on a workgroup, the Philox mask.  entry_score = 0 gives their bits, and so does
 *   entry_score = fl(sv[u] + se[e]) with sv = se = NULL (for scores without a -0.0).  A dot-product logit
 *   (hg_incidence_dot_heads_f32), GATv2's, or any score of the pair (u, e) goes here.
 * *_bwd_f32: the leaky factor takes the sign of the same three-term raw; ds_out [nnz, heads] is the gradient of entry_score
 *   itself, no further pass; dsv_out / dse_out (NULL: not wanted) are its sums as above.
 * Side 0 streams entry_score, side 1 reaches it through the plan's permutation as it reaches alpha.  No atomics; two
 *   calls give the same bits.  heads = 1 is the single-head layout.
 * Refusals, nothing launched: HG_ERR_INVALID for a null plan, heads < 1, a group other than 0 / 1 or a NULL entry_score
 *   (decided in this order, before the plan is looked at); HG_ERR_UNSUPPORTED for a plan built with HG_PLAN_HOST_ONLY;
 *   then HG_ERR_INVALID for a null array, a non-finite slope, p_drop outside [0, 1) or a bad rng_dev, as above.  The
 *   first-call-allocates rule is the other entries', and what is allocated is shared with them: a call captured into a
 *   hipGraph replays correctly after one warm call of the same group.
 * hg_gather_rows_incidence_heads_f32: one hop of hg_aggr_incidence_heads_f32 as an entry of its own,
 *     hop 0: dst[e, c] = ((sum_{p=(e,u)} w[p, c / C] * src[u, c]) * scaleA[e]) * scaleB[e]     src [N, F], dst [M, F]
 *     hop 1: dst[v, c] = ((sum_{p=(e,v)} w[p, c / C] * src[e, c]) * scaleA[v]) * scaleB[v]     src [M, F], dst [N, F]
 *   w: [nnz, heads] in H_T order (hop 1 reads it through the permutation), or NULL (unit weights); scaleA / scaleB: one
 *   factor per row of dst, or NULL.  It is the function hg_aggr_incidence*_f32 runs twice: the same schedule choice, LDS
 *   check, streaming-store choice and kernel instances, so hop 0 into hop 1 with (degE, W) and (degV, NULL) gives that
 *   entry's Xe_out and Y bit for bit.  It is the backward of hg_incidence_dot_heads_f32: dB = hop 0 of (A, g), dA = hop 1
 *   of (B, g).  workspace: hg_aggr_incidence_workspace_bytes(plan, F).  HG_ERR_INVALID for hop outside 0 / 1 (decided
 *   first), heads < 1 or F % heads != 0; HG_ERR_UNSUPPORTED for a host-only plan and where hg_aggr_incidence_f32 returns it.
 * Detect these entries by their exported symbols (HG_AGGR_VERSION does not change). */
HG_API int hg_incidence_attention_entry_heads_f32(const hg_plan *plan, int32_t group, int32_t heads, const int32_t *csrptr_t,
                                                  const int32_t *colind_t, const float *sv, const float *se,
                                                  const float *entry_score, float slope, float *alpha_out,
                                                  hg_stream_t stream);
HG_API int hg_incidence_attention_entry_heads_bwd_f32(const hg_plan *plan, int32_t group, int32_t heads,
                                                      const int32_t *csrptr_t, const int32_t *colind_t, const float *sv,
                                                      const float *se, const float *entry_score, float slope,
                                                      const float *alpha, const float *dalpha, float *ds_out,
                                                      float *dsv_out, float *dse_out, hg_stream_t stream);
HG_API int hg_incidence_attention_entry_dropout_heads_f32(const hg_plan *plan, int32_t group, int32_t heads,
                                                          const int32_t *csrptr_t, const int32_t *colind_t, const float *sv,
                                                          const float *se, const float *entry_score, float slope,
                                                          float p_drop, const uint64_t *rng_dev, float *alpha_out,
                                                          float *alpha_drop_out, hg_stream_t stream);
HG_API int hg_incidence_attention_entry_dropout_heads_bwd_f32(const hg_plan *plan, int32_t group, int32_t heads,
                                                              const int32_t *csrptr_t, const int32_t *colind_t,
                                                              const float *sv, const float *se, const float *entry_score,
                                                              float slope, float p_drop, const uint64_t *rng_dev,
                                                              const float *alpha, const float *dout, float *ds_out,
                                                              float *dsv_out, float *dse_out, hg_stream_t stream);
HG_API int hg_gather_rows_incidence_heads_f32(const hg_plan *plan, int32_t hop, int32_t F, int32_t heads,
                                              const int32_t *csrptr_t, const int32_t *colind_t, const float *src,
                                              const float *w, const float *scaleA, const float *scaleB, float *dst,
                                              void *workspace, size_t workspace_bytes, hg_stream_t stream);

/* ---- fused attention aggregation: the coefficients formed inside the gather -------------------------------------------------
 * hg_incidence_attention_heads_f32 into hg_aggr_incidence_heads_f32(v2e = e2v = alpha) writes alpha [nnz, heads] once and
 * reads it twice, the second time through the plan's permutation.  Every value of it is a function of four small numbers:
 *     alpha[p = (e, u), h] = exp(leaky(sv[u, h] + se[e, h]) - seg_max[g, h]) * seg_inv[g, h]      g = e (group 0) or u (group 1)
 * These entries keep the two per-segment numbers instead and form alpha in the lane that gathers the row it weighs.
 * hg_incidence_attention_stats_heads_f32: the maximum and sum passes of hg_incidence_attention_heads_f32 -- the same lane
 *   groups, workgroup path for rows above 128 entries and order of reduction -- writing seg_max = m and seg_inv = 1 / sum
 *   per segment and head: [M, heads] for group 0, [N, heads] for group 1, head fastest, fully overwritten, (0, 0) for an
 *   empty segment.  sv / se may be NULL (0).  It reads no permutation, with either group.
 * hg_aggr_incidence_attention_heads_f32: Y = hg_aggr_incidence_heads_f32(X, alpha, alpha, degE, degV, W) for the alpha of
 *   (group, sv, se, slope), bit for bit, Xe_out included, from seg_max / seg_inv of the stats entry.  Both hops run
 *   hg_aggr_incidence_heads_f32's schedules (a pinned latency schedule included), lanes and streaming-store choice on
 *   instances of the row gather that form w with the softmax kernel's own arithmetic.  What belongs to the destination row
 *   (its score; the statistics where the row is the segment) is read once per row; what belongs to the entry is gathered
 *   beside its row:
 *       hop 0, group 0: row se[e], seg_*[e]; entry sv[u]            hop 1, group 0: row sv[v]; entry se[e], seg_*[e]
 *       hop 0, group 1: row se[e]; entry sv[u], seg_*[u]            hop 1, group 1: row sv[v], seg_*[v]; entry se[e]
 *   No weights are staged and no permutation is read or uploaded; a panel's LDS is the unweighted one plus up to three
 *   floats per row and head.  workspace: hg_aggr_incidence_workspace_bytes(plan, F).
 * hg_gather_rows_attention_heads_f32: one hop of it as an entry of its own, as hg_gather_rows_incidence_heads_f32 is of
 *   hg_aggr_incidence_heads_f32: hop 0 with (degE, W) into hop 1 with (degV, NULL) gives the two-hop entry's bits.
 * Refusals, nothing launched, in this order: HG_ERR_INVALID for a null plan, hop outside 0 / 1, group outside 0 / 1,
 *   heads < 1, F < 1 or F % heads != 0, a null array (sv and se may both be NULL, seg_max / seg_inv may not), a non-finite
 *   slope; HG_ERR_WORKSPACE; HG_ERR_UNSUPPORTED for a plan built with HG_PLAN_HOST_ONLY, and where panel_rows * heads
 *   leaves no room in the 160 KiB of LDS.  The first stats call on a side uploads the long-row list the segment entries
 *   share (not capturable; one warm call makes every later one capturable); the two gather entries allocate nothing.
 * Not covered: dropout, a logit per incidence (entry_score is itself an [nnz, heads] stream) and bf16 rows.
 * Detect these entries by their exported symbols (HG_AGGR_VERSION does not change). */
HG_API int hg_incidence_attention_stats_heads_f32(const hg_plan *plan, int32_t group, int32_t heads, const int32_t *csrptr_t,
                                                  const int32_t *colind_t, const float *sv, const float *se, float slope,
                                                  float *seg_max_out, float *seg_inv_out, hg_stream_t stream);
HG_API int hg_aggr_incidence_attention_heads_f32(const hg_plan *plan, int32_t F, int32_t heads, int32_t group,
                                                 const int32_t *csrptr_t, const int32_t *colind_t, const float *X,
                                                 const float *sv, const float *se, float slope, const float *seg_max,
                                                 const float *seg_inv, const float *degE, const float *degV, const float *W,
                                                 float *Xe_out, float *Y, void *workspace, size_t workspace_bytes,
                                                 hg_stream_t stream);
HG_API int hg_gather_rows_attention_heads_f32(const hg_plan *plan, int32_t hop, int32_t group, int32_t F, int32_t heads,
                                              const int32_t *csrptr_t, const int32_t *colind_t, const float *src,
                                              const float *sv, const float *se, float slope, const float *seg_max,
                                              const float *seg_inv, const float *scaleA, const float *scaleB, float *dst,
                                              void *workspace, size_t workspace_bytes, hg_stream_t stream);

/* ---- gradients of the scales degE, W (one factor per hyperedge) and degV (one per vertex) ---------------------------------
 * For Y = degV . H_e2v (degE . W . (H_v2e^T X)) and its gradient dY, with P[v] = degV[v] * dY[v]:
 *     q[e] = < sum_{p=(e,u)} v2e[p] X[u],  sum_{p=(e,v)} e2v[p] P[v] >        dW[e] = q[e] * degE[e],  ddegE[e] = q[e] * W[e]
 *     ddegV[v] = < dY[v], Z[v] >,   Z = the aggregation without degV
 * hg_hyperedge_dot_heads_f32: out[e] = sum_c (sum_{p=(e,u)} wa[p, c / C] * A[u, c]) * (sum_{p=(e,u)} wb[p, c / C] * B[u, c]),
 *   q with (A, wa) = (X, v2e) and (B, wb) = (P, e2v).  A, B: [N, F] fp32, any F >= 1, 4-byte aligned; wa, wb: [nnz, heads]
 *   in H_T order, head fastest, or NULL (unit weights); C = F / heads; out [M], fully overwritten, an empty hyperedge
 *   gives exactly +0.0f.  Both sums run over the same H_T row: one lane group per hyperedge gathers the two member rows of
 *   an entry together and keeps both sums in registers, so neither [M, F] table is written.  Lanes are 16 bytes where
 *   F % 4 == 0, C % 4 == 0 and A, B are 16-byte aligned, else 4 bytes; rows wider than a lane group's tile (256 columns
 *   at 16-byte lanes) are walked once per column chunk.  Hyperedges of more than 128 members take one workgroup each (the
 *   list behind hg_plan_get_segment_info, side 0), the lane groups' sums combined through LDS in a fixed order.  No
 *   atomics; one launch plus at most one for the long rows; the order depends on the plan, F and heads only, so two
 *   calls give the same bits, and exchanging (A, wa) with (B, wb) gives them too.
 *   Refusals, nothing launched, in this order: HG_ERR_INVALID for a null plan, F < 1, heads < 1 or F % heads != 0;
 *   HG_ERR_UNSUPPORTED for a plan built with HG_PLAN_HOST_ONLY; HG_ERR_INVALID for a null A, B or out, then for a null
 *   csrptr_t / colind_t.  The first call on a plan builds and uploads the long-row list the segment entries share (not
 *   capturable; one warm call of either makes every later one capturable).
 * hg_rows_dot_f32: out[r] = <A[r, :], B[r, :]> for r < nrows, A and B [nrows, F]; one lane group per row, fixed order, no
 *   plan: the last step of ddegV.  HG_ERR_INVALID for nrows < 0, F < 1 or a null array.
 * Detect these entries by their exported symbols (HG_AGGR_VERSION does not change). */
HG_API int hg_hyperedge_dot_heads_f32(const hg_plan *plan, int32_t F, int32_t heads, const int32_t *csrptr_t,
                                      const int32_t *colind_t, const float *A, const float *wa, const float *B,
                                      const float *wb, float *out, hg_stream_t stream);
HG_API int hg_rows_dot_f32(int64_t nrows, int32_t F, const float *A, const float *B, float *out, hg_stream_t stream);

/* ---- bf16 feature rows on the incidence path -----------------------------------------------------------------------------------
 * The weighted row gather, the two-hop aggregation and the per-incidence dot with feature rows in bf16, on hg_aggr_fused_bf16's
 * contract -- fp32 in between, the fp32 call's order, one rounding:
 *   - per-incidence weights, scaleA / scaleB, degE / degV / W and the dot's out stay fp32;
 *   - a bf16 row is widened in the load (exact); lane accumulators, wave-task partial rows, the workspace and hop 1's table are
 *     fp32, summed on the fp32 entry's schedule, lanes and order; a bf16 destination is rounded once, to nearest even (NaN
 *     stays NaN).
 * So each entry equals its _f32 twin called on 16-byte aligned widened copies of the bf16 arrays: fp32 outputs bit for bit,
 * bf16 outputs the fp32 output rounded to bf16, bit for bit.  Only 16-byte lanes (four columns: 8 bytes of bf16) exist for
 * bf16 rows: F % 4 == 0, C = F / heads with C % 4 == 0, bf16 row arrays 8-byte aligned and fp32 row arrays 16-byte aligned
 * (where the fp32 twin takes those lanes too); anything else is HG_ERR_UNSUPPORTED, decided after the twin's own refusals,
 * in the twin's order, nothing launched -- widen, call the fp32 entry and round instead.
 * hg_gather_rows_incidence_heads_bf16: hg_gather_rows_incidence_heads_f32 with io saying which of src / dst holds bf16 rows:
 *   HG_ROWS_SRC_BF16, HG_ROWS_DST_BF16 or both; io = 0 (or another bit) is HG_ERR_INVALID, decided with hop: use the fp32
 *   entry.  w NULL: the unweighted instances.  The pinned latency schedule, the LDS check and the workspace
 *   (hg_aggr_incidence_workspace_bytes(plan, F)) are the fp32 entry's; streaming stores are chosen on the bytes of a row of
 *   dst, which moves no bits.
 * hg_aggr_incidence_heads_bf16: hg_aggr_incidence_heads_f32 with X and Y bf16 (heads = 1: hg_aggr_incidence_f32): hop 1 reads
 *   bf16 rows into the fp32 table -- Xe_out if given, else the workspace; Xe_out has the fp32 call's bits -- and hop 2
 *   rounds its fp32 sums into Y.  v2e_val = e2v_val = NULL gives the bits of hg_aggr_fused_bf16 on the pull kernels of the
 *   same schedule.
 * hg_incidence_dot_heads_bf16: hg_incidence_dot_heads_f32 (heads = 1: hg_incidence_dot_f32) with io saying which of A / B
 *   holds bf16 rows: HG_DOT_A_BF16, HG_DOT_B_BF16 or both; io = 0 is HG_ERR_INVALID, decided first.  out is fp32
 *   [nnz, heads]; lane count, run length, fma chain and butterfly are the fp32 kernel's.
 * Not covered: bf16 weights, the attention instances (hg_aggr_incidence_attention_heads_f32), the segment kernels,
 *   hg_hyperedge_dot_heads_f32 and hg_rows_dot_f32.
 * Detect these entries by their exported symbols (HG_AGGR_VERSION does not change). */
#define HG_ROWS_SRC_BF16 1
#define HG_ROWS_DST_BF16 2
#define HG_DOT_A_BF16 1
#define HG_DOT_B_BF16 2
HG_API int hg_gather_rows_incidence_heads_bf16(const hg_plan *plan, int32_t hop, int32_t F, int32_t heads,
                                               const int32_t *csrptr_t, const int32_t *colind_t, const void *src,
                                               const float *w, const float *scaleA, const float *scaleB, void *dst,
                                               void *workspace, size_t workspace_bytes, int32_t io, hg_stream_t stream);
HG_API int hg_aggr_incidence_heads_bf16(const hg_plan *plan, int32_t F, int32_t heads, const int32_t *csrptr_t,
                                        const int32_t *colind_t, const uint16_t *X, const float *v2e_val,
                                        const float *e2v_val, const float *degE, const float *degV, const float *W,
                                        float *Xe_out, uint16_t *Y, void *workspace, size_t workspace_bytes,
                                        hg_stream_t stream);
HG_API int hg_incidence_dot_heads_bf16(const hg_plan *plan, int32_t F, int32_t heads, const int32_t *csrptr_t,
                                       const int32_t *colind_t, const void *A, const void *B, float *out, int32_t io,
                                       hg_stream_t stream);

/* ---- max and min in the row gather, with the winner recorded --------------------------------------------------------------
 * hg_gather_rows_reduce_f32: one hop with a comparison in place of the sum, op = HG_REDUCE_MAX or HG_REDUCE_MIN, fp32:
 *     hop 0: dst[e, c] = ((op_{p=(e,u)} src[u, c]) * scaleA[e]) * scaleB[e]     arg_out[e, c] = p*      src [N, F], dst [M, F]
 *     hop 1: dst[v, c] = ((op_{p=(e,v)} src[e, c]) * scaleA[v]) * scaleB[v]     arg_out[v, c] = p*      src [M, F], dst [N, F]
 *   arg_out: int32 [rows of dst, F], the winning incidence's position in colind_t (the convention of the [nnz] weight
 *   arrays; hop 1 finds it through the plan's permutation).  The winner is the entry with the greatest (smallest) value
 *   under > (<), so -0.0 ties +0.0; among ties the smallest position wins.  The value before scaling is src[ind[p*], c] bit
 *   for bit.  A non-empty row always has a winner (all -inf under max: its first position).  An empty row gets exactly +0.0
 *   and arg_out = -1, no scale applied (degE may be inf).  NaN in src: unspecified (which entry wins, and so dst and arg_out
 *   of that column).  scaleA / scaleB: one factor per row of dst, or NULL.
 *   It runs on the schedules of hg_gather_rows_incidence_heads_f32 -- panels, wave tasks, partial slots and fixups, a pinned
 *   latency schedule honoured, the same LDS check -- with (value, position) carried per column; the comparison is exact and
 *   the tie rule total, so every schedule and every call give the same bits.  No atomics.  16-byte lanes where F % 4 == 0 and
 *   src, dst and arg_out are 16-byte aligned, else 4-byte lanes on the sum gather's lane groups (column tiles above 64 lanes).
 *   workspace: hg_gather_rows_reduce_workspace_bytes(plan, F), 256-byte aligned: a float and an int32 table of partial slots.
 * hg_gather_rows_select_f32: the gradient of that hop's src, as a row gather over the OTHER hop's CSR -- no scatter, no
 *   atomics, the sum gather's order of addition.  hop names the hop being differentiated; arg is its arg_out and gs its
 *   incoming gradient times the scales (the caller multiplies), both [rows of dst, F]; dsrc is [rows of src, F]:
 *     dsrc[u, c] = sum over the entries q of row u of the opposite CSR, in row order, of (arg[r_q, c] == pos(q)) ? gs[r_q, c] : 0
 *   with r_q the entry's other end and pos(q) its colind_t position.  A duplicate incidence is two positions, of which the
 *   winner is one: its gradient arrives once.  dsrc is fully overwritten.  Lanes as above (gs, arg, dsrc); the same workspace.
 * Both: the first call that walks H (reduce hop 1, select of hop 0) uploads the plan's permutation and so cannot be
 *   captured into a hipGraph; make one such call before capturing.  Refusals, nothing launched, in this order:
 *   HG_ERR_INVALID for a null plan, a hop outside 0 / 1, an op other than the two; HG_ERR_UNSUPPORTED for a plan built with
 *   HG_PLAN_HOST_ONLY; HG_ERR_INVALID for F < 1 or a null array; HG_ERR_UNSUPPORTED where hg_aggr_incidence_f32 returns it
 *   (LDS); HG_ERR_WORKSPACE.
 * Not covered: bf16 rows, per-incidence weights, and hg_gather_max_f32 below, which keeps the reference's arithmetic.
 * Detect these entries by their exported symbols (HG_AGGR_VERSION does not change). */
#define HG_REDUCE_MAX 1
#define HG_REDUCE_MIN 2
HG_API size_t hg_gather_rows_reduce_workspace_bytes(const hg_plan *plan, int32_t F);
HG_API int hg_gather_rows_reduce_f32(const hg_plan *plan, int32_t hop, int32_t F, int32_t op, const int32_t *csrptr_t,
                                     const int32_t *colind_t, const float *src, const float *scaleA, const float *scaleB,
                                     float *dst, int32_t *arg_out, void *workspace, size_t workspace_bytes,
                                     hg_stream_t stream);
HG_API int hg_gather_rows_select_f32(const hg_plan *plan, int32_t hop, int32_t F, const int32_t *csrptr_t,
                                     const int32_t *colind_t, const float *gs, const int32_t *arg, float *dsrc,
                                     void *workspace, size_t workspace_bytes, hg_stream_t stream);

/* first_aggr = "max" pieces (hgnnaggr_max, source/hgnnaggr/hgnnaggr_cuda.cu:144-208).
 * hg_gather_max_f32: Xe[e,k] = (max_{u in e} X[u,k], start -1e5, strict >) * (degE[e]*W[e]),
 * record[e,k] = winning vertex (0 if none).  The second hop is hg_gather_rows_f32(hop = 1).
 * hg_scatter_record_f32 (backward): Y = 0; Y[record[e,k], k] += T[e,k] * degV[record[e,k]]. */
HG_API int hg_gather_max_f32(int32_t M, int32_t F, const int32_t *csrptr_t, const int32_t *colind_t,
                             const float *X, const float *degE, const float *W, float *Xe,
                             int32_t *record, hg_stream_t stream);
HG_API int hg_scatter_record_f32(int32_t N, int32_t M, int32_t F, const float *T,
                                 const int32_t *record, const float *degV, float *Y,
                                 hg_stream_t stream);

/* The reference's kernel driven by the reference's schedule tensors
 * (HGNNAggr_forward_kernel(+_sf), hgnnaggr_cuda.cu:14-84; unweighted twins
 * hgnnAgg.cuh:33-53, 98-167): task g reads partition group_st[g] and scatters
 * to partition group_ed[g] of hyperedge group_row[g] with fp32 atomics.  Pass
 * group_key == NULL for one task per hyperedge (needs csrptr_t).  Y is zeroed
 * on `stream` first (the reference's torch::zeros, hgnnaggr_cuda.cu:374). */
HG_API int hg_aggr_push_groups_f32(int32_t N, int32_t M, int32_t F, int64_t n_group,
                            const int32_t *group_key, const int32_t *group_row,
                            const int32_t *group_st, const int32_t *group_ed,
                            const int32_t *csrptr_t, const int32_t *colind_t,
                            const float *X, const float *degE,
                            const float *degV, const float *W, float *Y,
                            hg_stream_t stream);

/* k nearest neighbours in feature space, without the nq x n distance matrix (csrc/hg_knn.hip): the hyperedges of HGNN's
 * ModelNet40 / NTU2012 hypergraphs and of DHGNN's layers ("each vertex and its k nearest neighbours").  float32 only.
 *
 * Q [nq, F] are the query rows and X [n, F] the candidates, row-major, 4-byte aligned (device memory).
 *   d2(i, j) = sum_c (Q[i, c] - X[j, c])^2 in float32, in the difference form -- never |q|^2 + |x|^2 - 2 q.x -- summed
 * over c = 0 .. F - 1 in that order into one accumulator with an explicit fma.  Identical rows give exactly +0.0; inputs
 * of integer value with d2 < 2^24 give exact results; -0.0 cannot occur; the bits of d2(i, j) are the same on every call,
 * in every tile and under every cand_slices.
 * Selection: row i of idx / dist [nq, k] holds the k smallest candidates under the TOTAL ORDER (d2, j) -- the smaller
 * distance first, among equal distances the smaller index -- written in that order, ascending.  Because the order is
 * total the result is one bit pattern for every tiling, every cand_slices and every call.  No atomics are used.
 * self_first != 0 (needs Q == X: the same pointer and nq == n): candidate j == i is ranked before everything else, so
 * slot 0 of row i is (i, 0.0) even where an exact duplicate of row i has a smaller index.
 * seg != NULL (HOST memory, [B + 1], ascending, seg[0] = 0, seg[B] = n; needs Q == X): row i competes with the rows of
 * its own segment only -- many small point sets in one tensor.  A segment of fewer than k rows is HG_ERR_INVALID.  The
 * offsets are copied to the workspace and the stream is waited for once, before the launch.
 * mean_dist != NULL: mean_dist[i] = the mean of sqrt(d2(i, j)) (the hardware's square root: 1 ulp, a d2 below the smallest
 * normal number counts as 0) over every candidate j of row i (its segment, or all n; itself included), summed in an order that is fixed for given (nq, n, seg, cand_slices): bit-identical across calls; it
 * may differ in the last bits across cand_slices.
 * cand_slices > 1 gives every workgroup one slice of its candidate tiles; the slices' lists go to the workspace and a
 * second kernel merges them under the same order.  0 picks 1 or 2 from nq and n (never more: see the workspace bound).
 * workspace: hg_knn_workspace_bytes(nq, n, F, k, cand_slices) bytes of device memory, at most
 * 16 * nq * k * max(cand_slices, 1) + 4096; it may be NULL when that is what seg == NULL and one slice need (nothing).
 * hg_knn_workspace_bytes returns 0 for arguments hg_knn_f32 refuses.
 * Refusals launch nothing and touch no device, set hg_last_error, and are decided in this order: HG_ERR_INVALID for a
 * null Q, X, idx or dist; nq, n or F < 1; k outside 1 .. 64; k > n; cand_slices < 0; self_first with Q != X; seg with
 * Q != X, with B < 1, seg[0] != 0 or seg[B] != n, not ascending, or with a segment shorter than k.  Then
 * HG_ERR_UNSUPPORTED for cand_slices > 32 or a pointer that is not 4-byte aligned, and HG_ERR_WORKSPACE for a workspace
 * that is null or too small when one is needed.  NaN inputs: unspecified. */
HG_API int hg_knn_f32(const float *Q, int32_t nq, const float *X, int32_t n, int32_t F, int32_t k, const int32_t *seg,
                      int32_t B, int32_t self_first, int32_t cand_slices, int32_t *idx, float *dist, float *mean_dist,
                      void *workspace, size_t workspace_bytes, hg_stream_t stream);
HG_API size_t hg_knn_workspace_bytes(int32_t nq, int32_t n, int32_t F, int32_t k, int32_t cand_slices);

/* hg_knn_f32's search with a dot-form prefilter on the f32 matrix unit (csrc/hg_knn_dot.hip), for wide rows.  idx and dist
 * are hg_knn_f32's for the same arguments, BIT FOR BIT, on every input: dist holds the difference-form float32 values and
 * the order is the same total order (d2, j).  The dot form never decides the result:
 *   n2[j] = sum_c X[j, c]^2 (float32, one fma per column, c ascending), s~(i, j) = sum_c Q[i, c] X[j, c] on
 *   v_mfma_f32_32x32x2_f32 (an fma chain in ascending c: the same bits in every tiling), d~ = (n2q[i] + n2[j]) - 2 s~;
 *   every row shortlists its kp = min(n, 32 ceil((k + 16) / 32)) smallest candidates under (d~, j) -- with self_first row i
 *   itself always -- and the shortlist's d2 is computed and ranked exactly as hg_knn_f32 does;
 *   with T the largest shortlisted d~, u = 2^-24, C = (2 F + 4)(1 + 1/64) rounded up to an integer, and
 *     E1 = C u (n2q[i] + max_j n2[j]) + (F + 2) 2^-146,   Ei = E1 + (F + 4) u max(T, 0),
 *   every candidate outside the shortlist has d2 >= T - Ei (|d~ - d2_exact| <= E1, and d2 >= d2_exact (1 - (F + 2) u)).  The row
 *   is certified iff its k-th d2 is strictly below T - Ei, or nothing was left out (n <= kp); a row that is not certified
 *   is searched over all n candidates in the difference form by the same launch, and fallback[i] (nullable, int32 [nq])
 *   is 1 for such a row and 0 for a certified one.
 * There is no seg: rows of point-set batches are narrow.  F is at most 65536 (the bound's derivation: HG_ERR_INVALID).
 * mean_dist != NULL: mean_dist[i] = the float32 mean over all n candidates of sqrt(max(d~(i, j), 0)) (the hardware's square
 * root), the pair (i, i) counting as exactly 0 when Q == X: within mean_j sqrt(E1) and the float32 summation error of the
 * exact mean; one bit pattern per cand_slices.  It is NOT hg_knn_f32's mean_dist bit for bit.
 * cand_slices: as hg_knn_f32's, clipped to the number of 128-row candidate tiles; 0 picks about 512 workgroups.  idx and dist
 * do not depend on it, and neither does fallback: the slices' shortlists are merged before T is taken.
 * workspace: hg_knn_dot_workspace_bytes(nq, n, F, k, cand_slices) bytes of device memory, always needed:
 * 4 (n + nq + n / 64) + slices nq (8 kp + 4) + 2048 at the most, kp <= 96 -- O(nq (k + shortlist) + nq + n), nothing of
 * nq x n.  It returns 0 for arguments hg_knn_dot_f32 refuses.
 * Nothing is allocated, copied to or from the host or waited for: five launches on `stream` (four when Q == X), recordable
 * into a hipGraph.  Refusals as hg_knn_f32's, in its order, with F > 65536 after F < 1: HG_ERR_INVALID for the arguments,
 * then HG_ERR_UNSUPPORTED for cand_slices > 32 or a misaligned pointer, then HG_ERR_WORKSPACE.  NaN inputs: unspecified;
 * norms that overflow are handled (such rows take the exhaustive path). */
HG_API int hg_knn_dot_f32(const float *Q, int32_t nq, const float *X, int32_t n, int32_t F, int32_t k, int32_t self_first,
                          int32_t cand_slices, int32_t *idx, float *dist, float *mean_dist, int32_t *fallback,
                          void *workspace, size_t workspace_bytes, hg_stream_t stream);
HG_API size_t hg_knn_dot_workspace_bytes(int32_t nq, int32_t n, int32_t F, int32_t k, int32_t cand_slices);

/* hg_knn_dot_f32 for bfloat16 rows (Q, X: bfloat16 bits, row-major, 2-byte aligned), the prefilter on
 * v_mfma_f32_32x32x16_bf16.  idx and dist are what hg_knn_f32 -- and so hg_knn_dot_f32 -- returns for the rows widened to
 * float32, BIT FOR BIT, on every input: the rerank and the exhaustive path read the bfloat16 rows, widen each element at
 * the load (exact) and then run hg_knn_f32's arithmetic.  dist is float32 and never holds an estimate.  Everything said of
 * hg_knn_dot_f32 holds -- kp, the shortlists, self_first, cand_slices, fallback, mean_dist (the mean of the bf16 estimates:
 * within mean_j sqrt(E1b) and the float32 summation error of the exact mean), the workspace (the same size:
 * hg_knn_dot_bf16_workspace_bytes), five launches, nothing allocated, copied or waited for, the refusals and their order
 * (the alignment: 2 bytes for Q and X, 4 for the rest) -- with this estimate and this bound in place of E1:
 *   n2[j] as above on the widened values (the bits of hg_knn_dot_f32's norm of the widened row); s~(i, j) accumulated by
 *   G = ceil(F / 16) instructions, instruction g taking columns 16 g .. 16 g + 15 (zeros past F) in every tiling;
 *   d~ = (n2q[i] + n2[j]) - 2 s~.
 *   Products of bfloat16 values are exact in float32.  The order and rounding of the instruction's sum are not documented;
 *   the bound rests on one HYPOTHESIS H: for exact products p_0 .. p_15 the result acc' of one instruction satisfies
 *     |acc' - (acc + sum p_i)| <= 17 v (|acc| + sum |p_i|),  v = 2^-23,
 *   up to quantities flushed to zero (below), and bfloat16 subnormal inputs are read at their value.  H holds for
 *   round-to-nearest additions in any order (at most 8 v) and for alignment to the largest exponent with truncation and no
 *   guard bit (16 v for the other sixteen terms, v for the result).  Over G instructions
 *     |s~ - S| <= ((1 + 17 v)^G - 1) sum_c |q_c x_c| <= 34 G u 1.0042 (Nq + Nx) / 2,  u = 2^-24, G <= 4096,
 *   and with the norms' F-term fma chains, as for E1,
 *     E1b = C_b u (n2q[i] + max_j n2[j]) + (65 G + 1) 2^-126,   C_b = (F + 34 G + 4)(1 + 1/64) rounded up to an integer,
 *     Ei  = E1b + (F + 4) u max(T, 0).
 *   The absolute term is sized for a matrix unit that flushes subnormal products and partial sums to zero: at most 2^-126 is
 *   lost per flushed quantity, an instruction has 16 products and 16 partial sums, so s~ loses at most 32 G 2^-126 (1 + 17 v)^G
 *   and d~ twice that, below (65 G) 2^-126; the last 2^-126 covers the gradual underflow of the fewer than 4 F + 8 vector
 *   operations.  The certificate is hg_knn_dot_f32's with E1b: the k-th d2 strictly below T - Ei, or n <= kp; and
 *   n2q + n2max < 1e37 and every shortlist slot filled. */
HG_API int hg_knn_dot_bf16(const uint16_t *Q, int32_t nq, const uint16_t *X, int32_t n, int32_t F, int32_t k, int32_t self_first,
                           int32_t cand_slices, int32_t *idx, float *dist, float *mean_dist, int32_t *fallback,
                           void *workspace, size_t workspace_bytes, hg_stream_t stream);
HG_API size_t hg_knn_dot_bf16_workspace_bytes(int32_t nq, int32_t n, int32_t F, int32_t k, int32_t cand_slices);
/* A DIAGNOSTIC, not part of any computation: est [nq, n] receives the raw estimate d~(i, j) of every pair (no self_first, no
 * clamp) and e1 [nq] the rows' E1b, from the same device code that forms the prefilter's tiles, so that H can be checked
 * against the hardware: |est - d2_exact| <= e1 must hold for every pair.  Unlike every other entry it allocates (the norms),
 * and it waits for `stream` before it returns.  HG_ERR_INVALID for a null pointer, nq, n or F < 1, F > 65536;
 * HG_ERR_UNSUPPORTED for nq * n above 2^22 or a misaligned pointer. */
HG_API int hg_knn_dot_estimates_bf16(const uint16_t *Q, int32_t nq, const uint16_t *X, int32_t n, int32_t F, float *est,
                                     float *e1, hg_stream_t stream);

/* Aggregation over a dense neighbour table, with no plan (csrc/hg_table.hip).  idx [rows, k] int32 is what hg_knn_f32
 * writes: hyperedge i has the k members idx[i, 0 .. k - 1], so H_T is the table itself (csrptr_t an arange) and position
 * p = i k + s of the table is entry s of hyperedge i.  1 <= k <= 64 and rows * k < 2^31.  None of the three entries
 * allocates, synchronises or copies to or from the host: each launches on `stream` and returns, so each can be recorded
 * into a hipGraph.  float32 only.
 *
 * hg_table_transpose: ptr_v [n + 1] receives the CSR offsets of the n vertices and pos_v[ptr_v[v] .. ptr_v[v + 1]) the
 *   positions p with idx[p] == v in ASCENDING p: the stable sort of the positions by vertex, a function of idx alone.
 *   Hyperedge p / k and slot p % k come from the position, so pos_v is column index and weight index in one.  An entry of
 *   idx outside 0 .. n - 1 is counted nowhere: ptr_v[n] is the number of valid entries and pos_v [rows * k] is
 *   unspecified from there on.  A vertex named twice by one row has both positions.  workspace:
 *   hg_table_transpose_workspace_bytes(rows, k, n) bytes of device memory (a pure host function; 0 for arguments the
 *   entry refuses), 4-byte aligned.
 * hg_table_gather_f32 (a hyperedge's members):  dst[i] = dst_scale[i] * sum_{s = 0 .. k-1} term(i k + s, idx[i, s]),
 *   i < rows, src [n, F], dst [rows, F].
 * hg_table_gather_t_f32 (a vertex's hyperedges): dst[v] = dst_scale[v] * sum_{q = ptr_v[v] .. ptr_v[v+1]-1}
 *   term(pos_v[q], pos_v[q] / k),  v < n, src [rows, F], dst [n, F].
 *   term(p, j) = (src[j] * src_scale[j]) * w[p]; w [rows * k], src_scale [source rows] and dst_scale [destination rows]
 *   may each be NULL, and an absent factor is no multiplication.  The accumulator starts at +0.0, every term is rounded
 *   and added with one rounded add (no fma), dst_scale is applied once at the end.  A vertex with no entry is exactly
 *   +0.0 whatever its scale.  An entry of idx outside 0 .. n - 1 (of pos_v outside 0 .. rows k - 1) contributes nothing
 *   and is not read through.
 *   ORDER: a row of at most HG_TABLE_SEQ_MAX entries -- every row of hg_table_gather_f32 -- is summed in ascending s / q
 *   into one accumulator per column: a float32 loop reproduces it bit for bit.  A longer vertex row is cut into P
 *   consecutive pieces of ceil(len / P) entries, each summed in ascending q from +0.0, and the P partial rows are added in
 *   the tree part[g] += part[g + s], s = P' / 2, P' / 4 .. 1 (P' the power of two at or above P); P = 4 * (64 / L) with
 *   L = min(ceil(F / c), 64) and c = 4 columns a lane where F % 4 == 0 and src and dst are 16-byte aligned, else 1.  So
 *   the bits of a row depend on its entries, its length, F and the alignment alone -- not on the launch, the other rows or
 *   where the row stands.  No floating-point atomics: two calls give the same bits.
 * Refusals launch nothing, set hg_last_error, in this order: HG_ERR_INVALID for a null idx (ptr_v, pos_v), src or dst,
 *   for rows, n or F < 1, for k outside 1 .. 64, for rows * k >= 2^31; HG_ERR_UNSUPPORTED for a pointer that is not
 *   4-byte aligned; HG_ERR_WORKSPACE (the transpose) for a null, small or misaligned workspace. */
#define HG_TABLE_SEQ_MAX 128
HG_API int hg_table_seq_max(void); /* HG_TABLE_SEQ_MAX of the library as built */
HG_API size_t hg_table_transpose_workspace_bytes(int32_t rows, int32_t k, int32_t n);
HG_API int hg_table_transpose(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t *ptr_v, int32_t *pos_v,
                              void *workspace, size_t workspace_bytes, hg_stream_t stream);
HG_API int hg_table_gather_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, const float *src,
                               const float *w, const float *src_scale, const float *dst_scale, float *dst,
                               hg_stream_t stream);
HG_API int hg_table_gather_t_f32(const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k, int32_t n, int32_t F,
                                 const float *src, const float *w, const float *src_scale, const float *dst_scale,
                                 float *dst, hg_stream_t stream);

/* Training through the weights of a neighbour table (csrc/hg_table.hip): the distances of a given table, the two
 * "difference gathers" that are their gradient, and the dot products that are the gradient of the table's weights.  Like
 * the entries above, each launches once on `stream`, allocates and waits for nothing and can be recorded into a hipGraph;
 * float32 only; no floating-point atomics, so two calls give the same bits.
 *
 * hg_table_dist_f32: dist[i, s] = d2(i, idx[i, s]) = sum_c (Q[i, c] - X[idx[i, s], c])^2 for Q [rows, F], X [n, F],
 *   dist [rows, k], in hg_knn_f32's arithmetic (its d2(i, j) paragraph above): the difference form, c = 0 .. F - 1 in that
 *   order, one accumulator from +0.0, the difference rounded and then one explicit fma.  So for the idx that hg_knn_f32 or
 *   hg_knn_dot_f32 returned, dist is the dist they returned, BIT FOR BIT, under self_first too; identical rows give +0.0.
 *   The bits depend on the two rows alone -- not on F % 4, the alignment or the launch.  An entry of idx outside 0 .. n - 1
 *   gives +0.0 and is not read through.
 * hg_table_gather_diff_f32 / hg_table_gather_t_diff_f32: hg_table_gather_f32 / hg_table_gather_t_f32 with a centre row,
 *   dst[r] = dst_scale[r] * sum_entries term(p, j),   term(p, j) = ((ctr[r] - src[j]) * src_scale[j]) * w[p],
 *   ctr [destination rows, F] (never NULL): the subtraction and every multiplication are rounded on their own, and the term
 *   is added with one rounded add (no fma).  Everything else is the plain gathers': which entries a row has, the absent
 *   factors, the +0.0 of an empty row, the ignored entries, and the ORDER paragraph above word for word, with c = 4 only
 *   where ctr is 16-byte aligned as well.  A source row equal to the centre contributes exactly 0.
 *   With g = 2 dDist these are the gradients of hg_table_dist_f32: dQ = gather_diff(idx; ctr = Q, src = X, w = g) and
 *   dX = gather_t_diff(ptr_v, pos_v; ctr = X, src = Q, w = g).
 * hg_table_dot_f32: out[p] = a_scale[j] * <A[j], B[i]> + <C[j], D[i]> for every position p = i k + s, j = idx[p]; A, C
 *   [n, F], B, D [rows, F], a_scale [n], out [rows * k].  a_scale may be NULL (no multiplication); C and D are both NULL
 *   (no second product and no addition) or both given.  An entry outside 0 .. n - 1 writes +0.0 and is not read through.
 *   DOT ORDER: c = 4 columns a lane where F % 4 == 0 and A, B, C and D are 16-byte aligned, else 1; L = the power of two
 *   at or above min(ceil(F / c), 64) lanes share a position.  Lane l owns the columns m L c + l c .. m L c + l c + c - 1
 *   below F, m = 0, 1 ..; over them, ascending, it runs s1 = fma(A[j, x], B[i, x], s1) and s2 = fma(C[j, x], D[i, x], s2),
 *   each from +0.0, and forms t[l] = a_scale[j] * s1 + s2 (the product rounded, then one rounded add; no fma).  Then
 *   t[l] = t[l] + t[l xor o] for o = L / 2, L / 4 .. 1, every lane at once, and out[p] = t[0].  So the bits of out[p] depend
 *   on the two pairs of rows, a_scale[j], F and the alignment alone -- not on k, the launch or where the row stands.
 *   With Xe = gather(idx, X, w, NULL, degE) and G = gather(idx, dY, w, degV, degE), the gradient of the weights of
 *   Y = degV . H_w (degE . (H_w^T X)) is dw = hg_table_dot_f32(A = dY, a_scale = degV, B = Xe, C = X, D = G).
 * Refusals launch nothing, set hg_last_error, in gather_refusal's order: HG_ERR_INVALID for a null idx (ptr_v, pos_v), then
 *   a null ctr (the difference gathers), a null src or dst / Q, X or dist / A, B or out, C without D or D without C; for
 *   rows, n or F < 1, k outside 1 .. 64, rows * k >= 2^31; then HG_ERR_UNSUPPORTED for a pointer that is not 4-byte
 *   aligned. */
HG_API int hg_table_dist_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, const float *Q, const float *X,
                             float *dist, hg_stream_t stream);
HG_API int hg_table_gather_diff_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, const float *src,
                                    const float *w, const float *src_scale, const float *dst_scale, const float *ctr,
                                    float *dst, hg_stream_t stream);
HG_API int hg_table_gather_t_diff_f32(const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k, int32_t n,
                                      int32_t F, const float *src, const float *w, const float *src_scale,
                                      const float *dst_scale, const float *ctr, float *dst, hg_stream_t stream);
HG_API int hg_table_dot_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, const float *A,
                            const float *a_scale, const float *B, const float *C, const float *D, float *out,
                            hg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HG_AGGR_H */
