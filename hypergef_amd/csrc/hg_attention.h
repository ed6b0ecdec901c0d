// Segment kernels of the hypergraph attention coefficients (hg_attention.hip): argument block and launcher, shared with
// hg_api.hip.  A segment is one group of incidences: a hyperedge's members (side 0, a contiguous H_T row) or a vertex's
// hyperedges (side 1, an H row whose entries reach their H_T positions through perm).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hg {

constexpr int kSegBlock = 256;  // threads per workgroup: 256 / width lane groups, or one long segment
constexpr int kSegKeep = 4;     // entries per lane whose gathered values stay in registers across the passes
constexpr int kSegLong = 128;   // segments of more entries leave the lane groups for a whole workgroup

enum {
  kSegSoftmax = 0,
  kSegSoftmaxBwd = 1,
  kSegSum = 2,
  kSegSoftmaxDrop = 3,
  kSegSoftmaxDropBwd = 4,
  // the four softmax bodies with a logit per incidence added to the score (SegEntryArgs)
  kSegSoftmaxEntry = 5,
  kSegSoftmaxEntryBwd = 6,
  kSegSoftmaxEntryDrop = 7,
  kSegSoftmaxEntryDropBwd = 8,
  // kSegSoftmax's maximum and sum passes alone: out_entry [nseg] receives every segment's maximum, out_seg [nseg] the
  // reciprocal of its sum (0 and 0 for an empty segment); no alpha is written and perm is not read
  kSegStats = 9
};

// The score's non-linearity and the coefficient of one incidence from its segment's statistics (kSegStats): what
// softmax_segment forms entry by entry -- raw = own + other with the segment's own score first (absent: 0) and the
// other end's absent meaning no addition, leaky relu, __expf of the difference to the maximum, times the reciprocal of
// the sum -- in that order, so that a kernel that forms its weights here (gather_rows_kernel's attention instances) has
// the bits kSegSoftmax would have written.  The library is built without floating-point contraction: the product
// slope * raw and the subtraction stay two roundings here as there.
__device__ __forceinline__ float leaky(float raw, float slope) { return raw > 0.f ? raw : slope * raw; }
__device__ __forceinline__ float attention_weight(float own, float other, bool has_other, float slope, float seg_max,
                                                  float seg_inv) {
  const float raw = has_other ? own + other : own;
  return __expf(leaky(raw, slope) - seg_max) * seg_inv;
}

struct SegArgs {
  const int32_t *ptr;       // the side's CSR row pointers [nseg + 1]: csrptr_t, or the derived ptr_v
  const int32_t *ind;       // the other end of every entry: colind_t (member vertex), or ind_v (hyperedge)
  const int32_t *perm;      // side 1: H entry -> H_T position; side 0: null
  const int32_t *long_seg;  // ids of the segments of more than kSegLong entries, ascending [nlong]
  int32_t nseg, nlong;
  const float *own;    // score of the segment's own end ([nseg]: se on side 0, sv on side 1), or null (0)
  const float *other;  // score gathered through ind ([N] sv on side 0, [M] se on side 1), or null (0)
  float slope;
  const float *val;    // kSegSoftmaxBwd: alpha; kSegSum: the summed values; H_T order
  const float *dval;   // kSegSoftmaxBwd: dalpha, H_T order
  float *out_entry;    // kSegSoftmax: alpha; kSegSoftmaxBwd: ds; H_T order.  kSegStats: the segments' maxima [nseg]
  float *out_seg;      // kSegSoftmaxBwd: the segments' own sums of ds (or null); kSegSum: out [nseg]; kSegStats: 1 / sum [nseg]
};

// The same arrays with `heads` columns, head fastest: own / other / out_seg [*, heads], val / dval / out_entry [nnz, heads].
struct SegHeadsArgs : SegArgs {
  int32_t heads;
};

// What the two dropout bodies take beside the block of the body they extend.  The mask is a function of (rng, H_T
// position, head) alone (hg_philox.h): kSegSoftmaxDrop writes alpha to out_entry as kSegSoftmax does and
// keep ? alpha * scale : +0 to out_drop; kSegSoftmaxDropBwd runs kSegSoftmaxBwd on (val, keep ? dval * scale : +0).
struct DropFields {
  const uint64_t *rng;  // device memory, read when the kernel runs: {key, sid}
  uint32_t T;           // an entry is kept where its Philox word >= T = floor(p_drop * 2^32)
  float scale;          // 1 / (1 - p_drop), rounded once on the host
  float *out_drop;      // kSegSoftmaxDrop: the dropped coefficients, H_T order; kSegSoftmaxDropBwd: unused
};
struct SegDropArgs : SegArgs {
  DropFields drop;
};
struct SegDropHeadsArgs : SegHeadsArgs {
  DropFields drop;
};

// The entry-logit bodies (kSegSoftmaxEntry*): raw[p, h] = (own + other) + entry[p, h].  One block for all four, the most
// general one (heads and dropout; heads = 1 and an unused `drop` are the special cases), so that the family has 24
// instances, not 96.
struct SegEntryArgs : SegDropHeadsArgs {
  const float *entry;  // [nnz, heads], H_T order, head fastest: side 0 streams it, side 1 reaches it through perm
};

// Lane-group width of a side whose segments of at most kSegLong entries hold `mean` entries on average.
int seg_width(double mean);

// One launch of segment_kernel on any of the five blocks.  body: kSeg*, among those of the block -- kSegSoftmax,
// kSegSoftmaxBwd, kSegSum and kSegStats on SegArgs / SegHeadsArgs, the two kSegSoftmaxDrop* on the dropout blocks (drop.rng
// needed), the four kSegSoftmaxEntry* on SegEntryArgs (entry needed; drop.rng by its two dropout bodies only); side 0 / 1;
// width 4 / 8 / 16 (seg_width).  A block with heads (>= 1) gives one lane group or, for a long segment, one workgroup
// to every (segment, head): column h is reduced as a block without heads reduces its single column.
template <typename ARGS>
hipError_t launch_segments(int body, int side, int width, const ARGS &a, hipStream_t stream);
extern template hipError_t launch_segments(int, int, int, const SegArgs &, hipStream_t);
extern template hipError_t launch_segments(int, int, int, const SegHeadsArgs &, hipStream_t);
extern template hipError_t launch_segments(int, int, int, const SegDropArgs &, hipStream_t);
extern template hipError_t launch_segments(int, int, int, const SegDropHeadsArgs &, hipStream_t);
extern template hipError_t launch_segments(int, int, int, const SegEntryArgs &, hipStream_t);

}  // namespace hg
