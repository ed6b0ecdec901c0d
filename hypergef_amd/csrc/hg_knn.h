// k-nearest-neighbour search (hg_knn.hip): tile sizes, limits and the workspace layout, shared by the two C entries
// hg_knn_f32 / hg_knn_workspace_bytes and by anything that wants to reason about the split.
//
// A workgroup of kKnnBlock threads owns kKnnTQ query rows and walks its candidate rows kKnnTC at a time; both are staged
// through LDS kKnnFC columns at a time.  Each lane holds an 8 x 8 tile of (query, candidate) sums.  A query row's running
// best-k list lives in the registers of the 32 lanes that share the row: lane t holds slots t and t + 32.
#pragma once
#include <cstddef>
#include <cstdint>

namespace hg {

constexpr int kKnnBlock = 256;     // threads per workgroup
constexpr int kKnnTQ = 64;         // query rows per workgroup
constexpr int kKnnTC = 256;        // candidate rows per tile
constexpr int kKnnFC = 32;         // columns per LDS chunk (the last chunk is padded with zeros)
constexpr int kKnnMaxK = 64;       // two list slots per lane x 32 lanes
constexpr int kKnnMaxSlices = 32;  // cand_slices above this: HG_ERR_UNSUPPORTED
constexpr int kKnnMergeRows = 4;   // merge kernel: one wave per query row, four rows per workgroup

// Where the pieces of the caller's workspace start (bytes).  Slice 0 keeps its list in idx / dist and its partial mean in
// mean_dist themselves, so the workspace holds slices 1 .. slices - 1 only:
//   [seg copy, int32 n + 1, when nq == n][idx, slices - 1 x nq x k int32][dist, the same in float][mean, slices - 1 x nq]
struct KnnLayout {
  size_t seg, idx, dist, mean, total;
};
KnnLayout knn_layout(int64_t nq, int64_t n, int k, int slices);

// cand_slices = 0: 2 when the query tiles alone leave most of the device idle and there are candidate tiles to share,
// else 1.  Never more than 2: hg_knn_workspace_bytes(.., cand_slices = 0) promises 16 nq k + 4096 bytes at the most.
int knn_auto_slices(int64_t nq, int64_t n);

// The dot-form prefilter (hg_knn_dot.hip, hg_knn_dot_f32): a workgroup of kDotBlock threads owns kDotTQ query rows, one wave
// 32 of them, and walks its candidate rows kDotTC at a time on v_mfma_f32_32x32x2_f32; both are staged through LDS kDotFC
// columns at a time, row-major with a row pitch of kDotLd floats.  A query row's shortlist lives in the 32 lanes of the
// half wave that holds the row's accumulators: lane t holds slots t, t + 32 and t + 64.
constexpr int kDotBlock = 256;
constexpr int kDotTQ = 128;
constexpr int kDotTC = 128;
constexpr int kDotFC = 32;
constexpr int kDotLd = 33;          // odd: the 32 rows and the two columns of an operand read land in 64 different banks
constexpr int kDotNormRows = 64;    // rows per workgroup of the norm kernel (one block maximum each)
constexpr int kDotMaxF = 65536;     // the error bound's derivation assumes (F + 1) 2^-24 <= 2^-8 + 2^-24
constexpr int kDotRerankRows = 64;  // the rerank kernel's batch: one candidate row per lane
// bfloat16 rows (hg_knn_dot_bf16): the same workgroup and tiles on v_mfma_f32_32x32x16_bf16, 16 columns per instruction
constexpr int kDotBfFC = 64;        // columns per LDS chunk: 128 bytes a row, four instructions
constexpr int kDotBfLd = 72;        // row pitch in elements, 144 bytes: nine 16-byte slots, odd, for the 16-byte operand reads
constexpr int64_t kDotEstimatesMax = 1 << 22;  // hg_knn_dot_estimates_bf16 (a diagnostic): nq * n above this is refused

// Shortlist slots per lane for k: the shortlist holds 32 * knn_dot_slots(k) entries, at least k + 16 (slack 16 .. 47).
inline int knn_dot_slots(int k) { return (k + 16 + 31) / 32; }

// Where the pieces of hg_knn_dot_f32's workspace start (bytes); kp = min(n, 32 * knn_dot_slots(k)) shortlist entries:
//   [n2x, float n][n2q, float nq][block maxima of n2x, float ceil(n / 64)][n2max, one float]
//   [shortlist idx, slices x nq x kp int32][shortlist estimates, the same in float][partial means, slices x nq]
struct KnnDotLayout {
  size_t n2x, n2q, bmax, n2max, idx, est, mean, total;
  int kp;
};
KnnDotLayout knn_dot_layout(int64_t nq, int64_t n, int k, int slices);

// cand_slices = 0: as many slices as fill about two workgroups per compute unit, at most one per candidate tile.
// Every other value is clipped to the number of candidate tiles (a slice without a tile has nothing to list).
int knn_dot_slices(int64_t nq, int64_t n, int cand_slices);

// The arguments hg_knn_f32 and hg_knn_dot_f32 have in common, and what both refuse about them (hg_knn.hip).
struct KnnCall {
  const char *entry;
  const void *Q, *X, *idx, *dist;
  int32_t nq, n, F, k, self_first, cand_slices;
};
// The sizes a *_workspace_bytes entry answers for (max_F: the entry's widest row, 0: no limit); it returns 0 for the others.
bool knn_sizes_ok(int32_t nq, int32_t n, int32_t F, int32_t k, int32_t cand_slices, int32_t max_F);
// The refusals up to the entry's own alignment check, in the order include/hg_aggr.h gives: HG_OK, or the status with the
// error set.  max_F: as above, refused where the dot entry refuses it; seg / B: the difference entry's segments (null: none).
int knn_refusal(const KnnCall &c, int32_t max_F, const int32_t *seg, int32_t B);

}  // namespace hg
