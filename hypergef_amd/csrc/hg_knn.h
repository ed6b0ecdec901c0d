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

}  // namespace hg
