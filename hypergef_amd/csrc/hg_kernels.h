// Kernel argument blocks and launchers shared by hg_kernels.hip and hg_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hg_internal.h"

namespace hg {

// A bf16 element as the kernels see it: the bit pattern (hg_aggr_fused_bf16).  Rows of X and Y may be bf16; the tiles,
// the materialised table, the partial rows and the scale vectors stay fp32.
struct bf16 {
  uint16_t bits;
};

struct GatherArgs {
  const int32_t *ptr;   // CSR row pointers [nrows + 1]
  const int32_t *ind;   // CSR column indices
  const void *src;      // gathered table [*, F], fp32 or bf16 (launch_gather's src_bf16)
  void *dst;            // output [nrows, F], fp32 or bf16 (launch_gather's dst_bf16)
  const float *scaleA;  // per-row factor applied first, or null
  const float *scaleB;  // per-row factor applied second, or null
  float *partial;       // partial-sum slots [nslots, F]
  const int32_t *scale_map;  // row -> index into scaleA/scaleB, or null (identity)
  const int32_t *dst_map;    // row -> output row, or null (identity)
  const Panel *panels;
  const Task *tasks;
  int32_t npanels, ntasks, n_task_blocks;
  int32_t F;
  int32_t panel_rows, panel_nnz;  // LDS carve-up
  int32_t xcd_remap;
  int32_t nt_dst = 0;  // rows of dst are final output nothing reads again in this call chain: streaming (nt) stores
};

// GatherArgs plus per-entry weights (hg_aggr_incidence_f32): entry p of the walked CSR adds w[wperm ? wperm[p] : p] *
// src[ind[p]].  Only gather_rows_kernel's weighted instances take it (fp32 rows); every other kernel keeps GatherArgs
// and so reads its arguments where it always did.
struct WeightedGatherArgs : GatherArgs {
  const float *w = nullptr;        // null: unit weights, the unweighted kernels
  const int32_t *wperm = nullptr;  // null: w is in the walked CSR's own order
};

// A weight per entry and head (hg_aggr_incidence_heads_f32): w is [nnz, heads], head fastest, and head h owns columns
// h * C .. (h + 1) * C - 1 of the F = heads * C wide rows.  Only gather_rows_kernel's WH instances take it.
struct HeadsGatherArgs : WeightedGatherArgs {
  int32_t heads = 1, C = 0;
};

// The attention coefficients formed in the gather (hg_aggr_incidence_attention_heads_f32): the weight of entry p of row r
// for head h is attention_weight (hg_attention.h) of the row's score, the score of the entry's other end ind[p], and the
// statistics of p's segment -- the row (stat_row) or the entry's other end.  All four arrays are [*, heads], head fastest.
// Only gather_rows_kernel's WA instances take it; they stage no weights and read no permutation.
struct AttnGatherArgs : GatherArgs {
  const float *row_score = nullptr;  // [nrows, heads], or null (0)
  const float *ent_score = nullptr;  // [rows of src, heads], or null (0)
  const float *seg_max = nullptr;    // stat_row: [nrows, heads]; else [rows of src, heads]
  const float *seg_inv = nullptr;
  int32_t stat_row = 0;
  float slope = 0.f;
  int32_t heads = 1, C = 0;
};

// GatherArgs for gather_rows_reduce_kernel (hg_gather_rows_reduce_f32, hg_gather_rows_select_f32), fp32 rows, no
// scale_map / dst_map.  An entry's position is its H_T position: its own index q in the walked CSR, or pperm[q].
// max / min: arg_out [nrows, F] receives the winner's position (-1: empty row), ipartial [nslots, F] holds the positions
// beside partial's values.  select: src is gs, arg_in [rows of src, F] the forward's arg; scales are not applied.
struct ReduceGatherArgs : GatherArgs {
  const int32_t *pperm = nullptr;
  int32_t *arg_out = nullptr;
  int32_t *ipartial = nullptr;
  const int32_t *arg_in = nullptr;
};

// What happens to an aggregated row t = Aggr(X)[v] on its way through the linear epilogue:
//   t' = ca * t + cb * R[v]   (R null: t' = ca * t),   T_out[v] = t' if wanted,
//   Y[v] = act(t' * Wlin^T),  act = relu or identity.
// One UniGCNII layer ((1-a) Xv + a X0, then (1-b) Xi + b W(Xi), relu: model/ugsys/unigcnii.py:19-21,
// model/gnn.py:196-199) or UniGIN layer ((1+eps) W(X) + Aggr(W(X)): unigin.py:20-22) is one such pass.
struct LinEpilogue {
  const float *R = nullptr;
  float ca = 1.f, cb = 0.f;
  const float *cb_dev = nullptr;  // non-null: cb is this device scalar, read when the kernel runs (a learned 1 + eps)
  int32_t relu = 0;
  float *T_out = nullptr;
  const void *wsplit = nullptr;  // Wlin as three bf16 planes in fragment order (launch_linear_pack_split): the fused panels' K = 128
                                 // matrix phase may then run as six bf16 products per fp32 product (HG_LIN_BF16X6)
};

struct FusedArgs {
  int32_t npanels;
  const int32_t *rec;     // packed per-panel records (hg_fused.cpp, pack_records)
  const FRec *rec_tab;    // per panel: record offset / length / list positions
  const int32_t *eid_all; // hyperedge id of every slot, record order (-1: materialised)
  int32_t max_rec_words;  // LDS space for one record
  int32_t ng;             // lane groups the records were packed for
  int32_t cap, rows_cap;  // LDS tile rows (hyperedge slots) and rows per panel
  int32_t dv_regs = 0;    // set by the launcher: bound degV travels in registers, not through LDS (fused_packed_kernel)
  const void *X;  // fp32, or bf16 (launch_fused's xy_bf16)
  const float *Xe_mat, *degE, *W, *degV;
  const float *bsA, *bsB, *bsD;  // bound scales in panel order (or null: gather from degE/W/degV)
  void *Y;        // fp32, or bf16 (launch_fused's xy_bf16)
  float *partial = nullptr;  // partial rows (pieces of split vertices): a row id with bit 31 set lands here
  int32_t F;
  int32_t xcd_remap;
  int32_t x_bytes;        // byte size of X (its own element size) if it fits a buffer descriptor (< 2 GiB), else 0
  int32_t mat_bytes;      // same for the materialised table
  int32_t nrows_x;        // rows of X
  int32_t nrows_mat = 0;  // rows of the materialised table
  int32_t y_nt = 0;       // rows of Y leave with the streaming (nt) hint: set for rows of whole 64-byte units (F % 16 == 0)
  int32_t reverse_runs = 0;  // each XCD walks its run of panels backwards (set after a substantial materialisation pre-pass)
  // fused linear epilogue (hg_aggr_linear_f32): Y[N, F_out] = (aggregated rows) * Wlin^T
  const float *Wlin = nullptr;  // Wlin [F_out, F] in MFMA fragment order (launch_linear_pack), or null
  int32_t F_out = 0;
  LinEpilogue epi;
};

// Y[rowmap ? rowmap[r] : r, :] = T[r, :] * Wlin^T for r < nrows; T is [nrows, F_in] row-major.
struct LinearArgs {
  const float *T;
  const float *Wlin;  // [F_out, F_in] in MFMA fragment order (launch_linear_pack)
  const int32_t *rowmap;
  float *Y;
  int64_t nrows;
  int32_t F_in, F_out;
  LinEpilogue epi;
};

// linear_rows_bf16_kernel (hg_aggr_linear_res_bf16's fallback, hg_linear_rows_bf16): row i of the call is row
// rowmap[i] (null: i) of T, R, T_out and Y alike.  Y = round_bf16(act(t . Wb^T)), t = T's row if T is bf16, else
// round_bf16(ca * T + cb * R) of the fp32 row (written to T_out where wanted).
struct LinearB16Args {
  const void *T;          // [*, F_in] bf16, or fp32 (launch_linear_bf16's t_f32)
  const void *wfrag;      // Wb [F_out, F_in] in fragment order (launch_linear_pack_bf16)
  const int32_t *rowmap;
  bf16 *Y;                // [*, F_out]
  int64_t nrows;
  int32_t F_in, F_out;
  const bf16 *R = nullptr;  // t_f32 only, as LinEpilogue's
  float ca = 1.f, cb = 0.f;
  const float *cb_dev = nullptr;
  int32_t relu = 0;
  bf16 *T_out = nullptr;    // t_f32 only
  int32_t y_nt = 0;         // rows of Y are whole 64-byte units: streaming stores
};

// The hub pass (HubPass, hg_internal.h): persistent workgroups, register accumulators.
struct HubArgs {
  const int32_t *rec;       // round records (hg_fused.cpp, build_hub_pass)
  const HubRec *rec_tab;
  const int32_t *wg_first;  // [nwg + 1] rounds of each workgroup
  const int32_t *vslot0;    // [ng * R] first partial row of each virtual row, -1 = unused
  int32_t nwg, ng, cap, max_rec_words;
  const void *X;        // fp32, or bf16 (launch_hub_pass's x_bf16)
  const float *Xe_mat, *degE, *W;
  float *partial;
  int32_t F;
  int32_t x_bytes, mat_bytes, nrows_x, nrows_mat;
  int32_t n_heavy = 0;  // hubs fed by stream flags (bits 24..27 of a slot's last entry)
  int32_t hslot0[kHubHeavy] = {};  // their first partial rows
};

// stream_rows_kernel (RowStream, hg_internal.h)
struct StreamArgs {
  const int32_t *rec;
  const SRec *rec_tab;
  int32_t nrec, ng, cap, max_rec_words;
  const void *src;              // gathered table [nrows_src, F], fp32 or bf16 (launch_stream_rows' src_bf16)
  int32_t src_bytes, nrows_src;
  const float *scaleA, *scaleB; // indexed by the record's sidx lists, or null
  void *dst;                    // fp32 or bf16 (launch_stream_rows' dst_bf16)
  float *partial;
  int32_t F, xcd_remap;
  int32_t nt_dst = 0;  // as GatherArgs::nt_dst
};

struct PushArgs {
  int64_t n_group;
  const int32_t *group_key, *group_row, *group_st, *group_ed;
  const int32_t *csrptr_t, *colind_t;
  const float *X, *degE, *degV, *W;
  float *Y;
  int32_t F;
};

// The element type of the rows of X / Y is a launch argument, not a field of the argument blocks: src_bf16 / dst_bf16 /
// xy_bf16 / x_bf16 pick the kernels' bf16 instances (16-byte lanes, F % 4 == 0; tiles, partial rows and the
// materialised table stay fp32).  At most one of src_bf16 and dst_bf16.
hipError_t launch_gather(const GatherArgs &a, int nfix, int nfix_l1, const Fixup *fixups, bool vec4,
                         hipStream_t stream, bool src_bf16 = false, bool dst_bf16 = false);
// the same with a.w (not null) on the weighted instances.  src_bf16 / dst_bf16 (either or both): as launch_gather's, vec4 only
hipError_t launch_gather_weighted(const WeightedGatherArgs &a, int nfix, int nfix_l1, const Fixup *fixups, bool vec4,
                                  hipStream_t stream, bool src_bf16 = false, bool dst_bf16 = false);
// a.w [nnz, heads] on the per-head instances.  vec4: as above; lane4: 16-byte lanes may be used (vec4 and C % 4 == 0, so
// that a lane lies inside one head); otherwise 4-byte lanes on the single-head call's lane groups.
// src_bf16 / dst_bf16: bf16 rows, lane4 only.
hipError_t launch_gather_heads(const HeadsGatherArgs &a, int nfix, int nfix_l1, const Fixup *fixups, bool vec4, bool lane4,
                               hipStream_t stream, bool src_bf16 = false, bool dst_bf16 = false);
// the attention instances: launch_gather_heads' lanes and order of summation, the weights formed from a's scores and statistics
hipError_t launch_gather_attention(const AttnGatherArgs &a, int nfix, int nfix_l1, const Fixup *fixups, bool vec4, bool lane4,
                                   hipStream_t stream);
// rmode 1 / 2: the max / min instances and their fixups; 3: the select instances and the sum gather's fixups.  Lanes as
// launch_gather's (vec4: F % 4 == 0 and src, dst, arg and both partial tables 16-byte aligned); LDS as the weighted instances'.
hipError_t launch_gather_reduce(const ReduceGatherArgs &a, int rmode, int nfix, int nfix_l1, const Fixup *fixups, bool vec4,
                                hipStream_t stream);
// the LDS one of their workgroups asks for: the unweighted panel plus one (stat_row: three) float per row and head
size_t attn_gather_lds_bytes(int32_t panel_rows, int32_t panel_nnz, int32_t heads, bool stat_row);
// out[p, h] = <A[ind[p], hC .. (h+1)C), B[e, hC .. (h+1)C)>, out [nnz, H].  lane4: C % 4 == 0 and A, B 16-byte aligned.
hipError_t launch_incidence_dot_heads(int32_t M, int64_t nnz, int32_t H, int32_t C, const int32_t *ptr, const int32_t *ind,
                                      const void *A, const void *B, float *out, bool lane4, hipStream_t stream,
                                      bool a_bf16 = false, bool b_bf16 = false);
// out[p] = <A[ind[p], :], B[e, :]> for every entry p of the CSR (ptr, ind) over M rows, e the row holding p (the weight
// gradient of hg_aggr_incidence_f32).  vec4: F % 4 == 0 and A, B 16-byte aligned.  a_bf16 / b_bf16: rows of A / B are bf16
// (vec4 / lane4 only, 8-byte aligned), widened in the load: the fp32 call's lanes, fma chain and butterfly.
hipError_t launch_incidence_dot(int32_t M, int64_t nnz, int32_t F, const int32_t *ptr, const int32_t *ind, const void *A,
                                const void *B, float *out, bool vec4, hipStream_t stream, bool a_bf16 = false,
                                bool b_bf16 = false);
// hyperedge_dot_kernel (hg_hyperedge_dot_heads_f32): out[e] = sum_c (sum_{p=(e,u)} wa[p, c / C] A[u, c]) * (sum_p wb[p, c / C] B[u, c])
struct EdgeDotArgs {
  const int32_t *ptr, *ind;  // H_T
  const int32_t *long_seg;   // hyperedges of more than kSegLong members (hg_attention.h), ascending [nlong]
  int32_t nlong;
  int32_t M, F, heads, C;    // F = heads * C
  const float *A, *wa;       // [N, F]; [nnz, heads] in H_T order, head fastest, or null (unit weights)
  const float *B, *wb;
  float *out;                // [M]
};
// lane4: 16-byte lanes (F % 4 == 0, C % 4 == 0, A and B 16-byte aligned); one launch, and one more for the long rows
hipError_t launch_hyperedge_dot(const EdgeDotArgs &a, bool lane4, hipStream_t stream);
// out[r] = <A[r, :], B[r, :]> for r < nrows.  vec4: F % 4 == 0 and A, B 16-byte aligned.
hipError_t launch_rows_dot(int64_t nrows, int32_t F, const float *A, const float *B, float *out, bool vec4,
                           hipStream_t stream);
// y_f32 (with xy_bf16, F in {32, 64, 128}): rows of X are bf16, rows of Y fp32 -- the aggregated rows of the bf16 linear
// layer on their way to linear_rows_bf16_kernel.  xy_bf16 with a.Wlin: the native bf16 epilogue (fused_linear_b16_ok);
// a.Wlin is then the bf16 fragments of launch_linear_pack_bf16, a.epi.R / a.epi.T_out point at bf16 rows, a.Y is bf16.
hipError_t launch_fused(const FusedArgs &a, bool vec4, hipStream_t stream, bool xy_bf16 = false, bool y_f32 = false);
hipError_t launch_hub_pass(const HubArgs &a, bool vec4, hipStream_t stream, bool x_bf16 = false);
size_t hub_pass_lds_bytes(int32_t cap, int32_t row_floats, int32_t max_rec_words);
// Y[fx.row] = scale[fx.row] * (sum of the fixup's partial rows); first-level fixups first.  Y_bf16: rows of Y are bf16.
hipError_t launch_fixups(const Fixup *fixups, int nfix, int nfix_l1, int32_t F, float *partial, void *Y,
                         const float *scaleA, const float *scaleB, const int32_t *scale_map, bool vec4,
                         hipStream_t stream, bool nt_dst = false, bool Y_bf16 = false);
bool stream_rows_ok(const StreamArgs &a, bool vec4);  // buffer-addressable table, 16-byte lanes
hipError_t launch_stream_rows(const StreamArgs &a, hipStream_t stream, bool src_bf16 = false, bool dst_bf16 = false);
bool fused_linear_ok(const FusedArgs &a);  // can launch_fused run this call's linear epilogue?
hipError_t launch_linear(const LinearArgs &a, hipStream_t stream);
bool fused_linear_b16_ok(const FusedArgs &a);  // fused_linear_ok, and the panels take the native bf16 epilogue (F = 128, F_out <= 128)
hipError_t launch_linear_bf16(const LinearB16Args &a, bool t_f32, hipStream_t stream);
hipError_t launch_linear_pack_bf16(int32_t F_out, int32_t F_in, const uint16_t *Wlin, void *wfrag, hipStream_t stream);
int wgrad_parts(int64_t nrows, int32_t Fa, int32_t Fb);
bool wgrad_shape_ok(int32_t Fa, int32_t Fb);  // <= 16 tiles of 16 x 16, or both widths multiples of 64 up to 512 (64 x 64 blocks)
hipError_t launch_wgrad(int64_t nrows, int32_t Fa, int32_t Fb, const float *A, const float *B, float *C,
                        float *partial, hipStream_t stream);
hipError_t launch_linear_pack(int32_t F_out, int32_t F_in, const float *Wlin, float *wfrag, hipStream_t stream);
hipError_t launch_linear_pack_split(int32_t F_out, int32_t F_in, const float *Wlin, void *wsplit, hipStream_t stream);
int fused_tile_row_floats(int F, bool vec4);
hipError_t launch_push(const PushArgs &a, hipStream_t stream);
hipError_t launch_bind_scales(int64_t nslots, const int32_t *eid_all, const float *degE, const float *W,
                              float *bsA, float *bsB, int64_t nrows, const int32_t *prow, const float *degV,
                              float *bsD, hipStream_t stream);
// *flag (device int32, preset to 1) is cleared if any of W[0..n) differs from 1.0f
hipError_t launch_all_ones(int64_t n, const float *W, int32_t *flag, hipStream_t stream);
hipError_t launch_gather_max(int32_t M, int32_t F, const int32_t *ptr, const int32_t *ind, const float *X,
                             const float *degE, const float *W, float *Xe, int32_t *record,
                             hipStream_t stream);
hipError_t launch_scatter_record(int32_t M, int32_t F, const float *T, const int32_t *record,
                                 const float *degV, float *Y, hipStream_t stream);

}  // namespace hg
