// Hypergraph attention coefficients (include/hg_aggr.h, hg_incidence_attention_f32 and friends): one family of segment
// kernels with three bodies -- the fused score + softmax, its backward, and the plain segment sum.
//
// A segment is a group of incidences: the members of a hyperedge (side 0: a contiguous row of H_T, entry i sits at H_T
// position i) or the hyperedges of a vertex (side 1: a row of the derived H, entry i sits at H_T position perm[i]).
// Everything per entry -- alpha, dalpha, ds, val -- lives in H_T order, so side 0 streams it and side 1 reaches it through
// perm, as hop 2 of hg_aggr_incidence_f32 reaches e2v.
//
// Work split.  A lane group of W lanes (4, 8 or 16: the side's mean segment length, seg_width) owns one segment and
// strides over it; 256 / W segments per workgroup.  A lane gathers its first kSegKeep entries once and keeps them in
// registers across the passes of a body (softmax: maximum, sum, write); what a longer segment holds beyond W * kSegKeep
// entries is gathered again in each pass.  Segments of more than kSegLong entries would leave one lane group looping
// long after the grid has drained (the power-law shape has 4096-entry hyperedges and 25000-entry vertices beside a mean
// of 3-6): the lane groups skip them, and the first `nlong` workgroups of the same launch take one each from the plan's
// list, all 256 lanes striding, the same code with W = 256.
//
// No atomics.  A lane adds its entries in ascending order, the lanes of a group are combined by an xor butterfly
// (commutative at every step: all lanes end with the same bits), a workgroup combines its four waves' results in wave
// order through LDS.  The order depends on the segment's length and the side's width only: two calls give the same bits.
//
// One kernel, segment_kernel<BODY, SIDE, W, ARGS>, carries that split for every body and every argument block
// (hg_attention.h); what a block adds to SegArgs selects, at compile time, what the kernel does beside it.
//
// Heads (the blocks derived from SegHeadsArgs, the *_heads_f32 entries).  Scores are [nseg, H], entry arrays [nnz, H],
// head fastest.  A lane group owns one (segment, head) pair, consecutive lane groups the consecutive heads of one
// segment, so the groups of a wave read neighbouring words of the same rows; the long segments take one workgroup per
// (segment, head).  A pair runs the single-head code on column h (Col<true>: element i of a column sits at i * H + h), so
// its order of reduction is the single-head one -- it depends on the segment's length and W, not on H -- and column h of
// a result has the bits of the single-head call on column h of the inputs.  The other blocks count segments in 32 bits
// and index with Col<false>, the plain index.
//
// Dropout (kSegSoftmaxDrop / kSegSoftmaxDropBwd, the blocks with DropFields).  The same two segment functions with a
// Drop in place of NoDrop: the forward writes alpha as before and, beside it, keep ? alpha * scale : +0; the backward
// masks and scales dalpha as it loads it and is the plain backward from there on.  keep is word 0 of Philox4x32-10 on
// the counter (H_T position, head, sid) compared with a threshold (hg_philox.h): no mask is stored, both sides and every
// width see the same one, and an entry beyond the kSegKeep kept ones recomputes it in each pass as it gathers its score
// again.  The reductions are untouched, so alpha, t, ds and the sums have the bits of the plain bodies on pre-masked
// input.  The plain bodies do not see any of this: NoDrop compiles to nothing.
//
// Entry logits (kSegSoftmaxEntry*, SegEntryArgs).  The four softmax bodies with a logit per incidence, t [nnz, H] in H_T
// order: raw = (own + other) + t[p], the bracket formed first, as before.  An Entry in place of NoEntry adds t as the
// score is gathered: a kept entry folds it into the value it keeps in registers, an entry beyond the kept ones looks up
// its position (side 1: perm) and gathers t again in each pass, as it gathers the score again.  Everything after raw --
// leaky relu, maximum, exponentials, reduction order, the mask -- is the code above, so t = 0 gives the bits of the plain
// bodies.  The backward's ds is the gradient of t itself.  The four bodies run on the most general block alone (heads
// and dropout): a single-head call has H = 1 (Col<true>{1, 0} is the plain index in 64 bits), a call without dropout
// leaves `drop` unread -- 24 instances instead of 96.
//
// Segment statistics (kSegStats, on SegArgs / SegHeadsArgs).  The softmax body up to the reciprocal of the sum, which
// then leaves with the maximum, [nseg, H]: lane groups, the workgroup path and the order of reduction are the softmax's,
// so attention_weight (hg_attention.h) on the two gives alpha's bits and no [nnz, H] array need exist
// (hg_aggr_incidence_attention_heads_f32).  Positions are not looked up: side 1 runs without perm.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "hg_attention.h"
#include "hg_philox.h"

namespace hg {
namespace {

struct OpMax {
  static __device__ __forceinline__ float apply(float a, float b) { return fmaxf(a, b); }
};
struct OpSum {
  static __device__ __forceinline__ float apply(float a, float b) { return a + b; }
};

// Where element i of the column a lane group works on sits: the array itself (single head), or column h of an [*, H]
// array.  The single-head form is the plain index, so those instances are what they were before heads existed.
template <bool MH>
struct Col;
template <>
struct Col<false> {
  __device__ __forceinline__ int32_t operator()(int32_t i) const { return i; }
  __device__ __forceinline__ uint32_t head() const { return 0; }
};
template <>
struct Col<true> {
  int32_t H, h;
  __device__ __forceinline__ int64_t operator()(int32_t i) const { return (int64_t)i * H + h; }  // nnz * H may pass 2^31
  __device__ __forceinline__ uint32_t head() const { return (uint32_t)h; }
};

// Combine one value per lane over the W lanes that share a segment; every lane gets the result.
template <int W, typename Op>
__device__ __forceinline__ float combine(float v, float *lds) {
  if constexpr (W <= 64) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v = Op::apply(v, __shfl_xor(v, o, W));
    return v;
  } else {  // the whole workgroup: four waves
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = Op::apply(v, __shfl_xor(v, o, 64));
    __syncthreads();  // the previous result has been read by everyone
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return Op::apply(Op::apply(lds[0], lds[1]), Op::apply(lds[2], lds[3]));
  }
}

// H_T position of entry i of the walked CSR
template <int SIDE>
__device__ __forceinline__ int32_t position(const SegArgs &a, int32_t i) {
  return SIDE == 0 ? i : a.perm[i];
}

// raw score of entry i: the segment's own score plus the gathered one of the entry's other end
template <bool MH>
__device__ __forceinline__ float raw_score(const SegArgs &a, Col<MH> col, float own, int32_t i) {
  return a.other ? own + a.other[col(a.ind[i])] : own;
}

// The logit of the entry itself (kSegSoftmaxEntry*): raw = (own + other) + t[p], p the entry's H_T position.  With NoEntry
// the segment functions take the `else` of every `if constexpr (kEnt)`, which is the line that was there: the instances
// without an entry logit stay instruction for instruction what they were (a wrapper around raw_score does not: it
// changes the order of inlining, and with it the register allocation).
struct NoEntry {};
struct Entry {
  const float *t;
};
template <bool MH>
__device__ __forceinline__ float raw_entry(const SegArgs &a, const Entry &en, Col<MH> col, float own, int32_t i, int32_t p) {
  return raw_score(a, col, own, i) + en.t[col(p)];
}
// the same for an entry whose position has not been looked up: only the entry logit needs it
template <int SIDE, bool MH>
__device__ __forceinline__ float raw_entry(const SegArgs &a, const Entry &en, Col<MH> col, float own, int32_t i) {
  return raw_score(a, col, own, i) + en.t[col(position<SIDE>(a, i))];
}

// The dropout of a launch as a lane holds it: the state read from device memory when the kernel runs (a seed passed by
// value would be frozen into a captured launch), the threshold, the scale and the second output.
struct NoDrop {};
struct Drop {
  DropRng rng;
  uint32_t T;
  float scale;
  float *out;
};
__device__ __forceinline__ Drop load_drop(const DropFields &f) {
  return Drop{drop_rng(f.rng[0], f.rng[1]), f.T, f.scale, f.out_drop};
}
// v as dropout leaves it at H_T position p of the column: fl(v * scale) where kept, else +0
template <bool MH>
__device__ __forceinline__ float dropped(const NoDrop &, Col<MH>, int32_t, float v) { return v; }
template <bool MH>
__device__ __forceinline__ float dropped(const Drop &d, Col<MH> col, int32_t p, float v) {
  return drop_keep(d.rng, d.T, (uint32_t)p, col.head()) ? v * d.scale : 0.f;
}

// alpha = softmax over the segment of leaky(raw).  An empty segment runs no entry loop at all: nothing is written and no
// exponential of (-inf) - (-inf) is formed.  A one-entry segment gives exp(0) / 1 = 1.0f exactly.
// STATS (kSegStats): the maximum and sum passes as they stand, then the segment's m and 1 / sum go out in place of alpha
// (0 and 0 for an empty segment, whose m is -inf and whose sum is 0); positions are not looked up, so perm is not read.
template <int SIDE, int W, bool MH, typename DROP = NoDrop, typename ENT = NoEntry, bool STATS = false>
__device__ __forceinline__ void softmax_segment(const SegArgs &a, Col<MH> col, int32_t seg, int32_t beg, int32_t end, int lane,
                                                float *lds, const DROP &d = DROP{}, const ENT &en = ENT{}, bool valid = true) {
  constexpr bool kDrop = std::is_same_v<DROP, Drop>;
  constexpr bool kEnt = std::is_same_v<ENT, Entry>;
  const float own = (a.own && beg < end) ? a.own[col(seg)] : 0.f;
  float sc[kSegKeep];
  int32_t pos[kSegKeep];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < kSegKeep; k++) {
    const int32_t i = beg + lane + k * W;
    if (i < end) {
      if constexpr (!STATS) pos[k] = position<SIDE>(a, i);
      if constexpr (kEnt) sc[k] = leaky(raw_entry(a, en, col, own, i, pos[k]), a.slope);
      else sc[k] = leaky(raw_score(a, col, own, i), a.slope);
      m = fmaxf(m, sc[k]);
    }
  }
  const int32_t tail = beg + lane + kSegKeep * W;
#pragma unroll 4
  for (int32_t i = tail; i < end; i += W) {
    if constexpr (kEnt) m = fmaxf(m, leaky(raw_entry<SIDE>(a, en, col, own, i), a.slope));
    else m = fmaxf(m, leaky(raw_score(a, col, own, i), a.slope));
  }
  m = combine<W, OpMax>(m, lds);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < kSegKeep; k++) {
    if (beg + lane + k * W < end) {
      sc[k] = __expf(sc[k] - m);
      sum += sc[k];
    }
  }
#pragma unroll 4
  for (int32_t i = tail; i < end; i += W) {
    if constexpr (kEnt) sum += __expf(leaky(raw_entry<SIDE>(a, en, col, own, i), a.slope) - m);
    else sum += __expf(leaky(raw_score(a, col, own, i), a.slope) - m);
  }
  sum = combine<W, OpSum>(sum, lds);
  const float inv = 1.f / sum;  // the entry holding the maximum contributes exp(0) = 1: sum >= 1 wherever it is used
  if constexpr (STATS) {
    if (lane == 0 && valid) {
      a.out_entry[col(seg)] = beg < end ? m : 0.f;
      a.out_seg[col(seg)] = beg < end ? inv : 0.f;
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < kSegKeep; k++)
    if (beg + lane + k * W < end) {
      if constexpr (kDrop) {  // the product that forms alpha is rounded first, then scaled
        const float al = sc[k] * inv;
        a.out_entry[col(pos[k])] = al;
        d.out[col(pos[k])] = dropped(d, col, pos[k], al);
      } else {
        a.out_entry[col(pos[k])] = sc[k] * inv;
      }
    }
  if constexpr (kDrop) {
#pragma unroll 2
    for (int32_t i = tail; i < end; i += W) {
      const int32_t p = position<SIDE>(a, i);
      float al;
      if constexpr (kEnt) al = __expf(leaky(raw_entry(a, en, col, own, i, p), a.slope) - m) * inv;
      else al = __expf(leaky(raw_score(a, col, own, i), a.slope) - m) * inv;
      a.out_entry[col(p)] = al;
      d.out[col(p)] = dropped(d, col, p, al);
    }
  } else {
#pragma unroll 4
    for (int32_t i = tail; i < end; i += W) {
      if constexpr (kEnt) {
        const int32_t p = position<SIDE>(a, i);
        a.out_entry[col(p)] = __expf(leaky(raw_entry(a, en, col, own, i, p), a.slope) - m) * inv;
      } else {
        a.out_entry[col(position<SIDE>(a, i))] = __expf(leaky(raw_score(a, col, own, i), a.slope) - m) * inv;
      }
    }
  }
}

// ds = alpha * (dalpha - t) * leaky'(raw), t = sum over the segment of alpha * dalpha; the segment's own sum of ds goes to
// out_seg (0 for an empty segment).  slope == 1: the non-linearity is the identity and no score is gathered.
template <int SIDE, int W, bool MH, typename DROP = NoDrop, typename ENT = NoEntry>
__device__ __forceinline__ void softmax_bwd_segment(const SegArgs &a, Col<MH> col, int32_t seg, int32_t beg, int32_t end, int lane,
                                                    float *lds, bool valid, const DROP &d = DROP{}, const ENT &en = ENT{}) {
  constexpr bool kEnt = std::is_same_v<ENT, Entry>;
  const bool need_raw = a.slope != 1.f;
  const float own = (need_raw && a.own && beg < end) ? a.own[col(seg)] : 0.f;
  float al[kSegKeep], da[kSegKeep], fac[kSegKeep];
  int32_t pos[kSegKeep];
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < kSegKeep; k++) {
    const int32_t i = beg + lane + k * W;
    if (i < end) {
      pos[k] = position<SIDE>(a, i);
      al[k] = a.val[col(pos[k])];
      da[k] = dropped(d, col, pos[k], a.dval[col(pos[k])]);
      if constexpr (kEnt) fac[k] = (need_raw && !(raw_entry(a, en, col, own, i, pos[k]) > 0.f)) ? a.slope : 1.f;
      else fac[k] = (need_raw && !(raw_score(a, col, own, i) > 0.f)) ? a.slope : 1.f;
      t += al[k] * da[k];
    }
  }
  const int32_t tail = beg + lane + kSegKeep * W;
#pragma unroll 4
  for (int32_t i = tail; i < end; i += W) {
    const int32_t p = position<SIDE>(a, i);
    t += a.val[col(p)] * dropped(d, col, p, a.dval[col(p)]);
  }
  t = combine<W, OpSum>(t, lds);
  float dsum = 0.f;
#pragma unroll
  for (int k = 0; k < kSegKeep; k++) {
    if (beg + lane + k * W < end) {
      const float ds = al[k] * (da[k] - t) * fac[k];
      a.out_entry[col(pos[k])] = ds;
      dsum += ds;
    }
  }
#pragma unroll 4
  for (int32_t i = tail; i < end; i += W) {
    const int32_t p = position<SIDE>(a, i);
    float f;
    if constexpr (kEnt) f = (need_raw && !(raw_entry(a, en, col, own, i, p) > 0.f)) ? a.slope : 1.f;
    else f = (need_raw && !(raw_score(a, col, own, i) > 0.f)) ? a.slope : 1.f;
    const float ds = a.val[col(p)] * (dropped(d, col, p, a.dval[col(p)]) - t) * f;
    a.out_entry[col(p)] = ds;
    dsum += ds;
  }
  if (a.out_seg) {
    dsum = combine<W, OpSum>(dsum, lds);
    if (lane == 0 && valid) a.out_seg[col(seg)] = dsum;
  }
}

template <int SIDE, int W, bool MH>
__device__ __forceinline__ void sum_segment(const SegArgs &a, Col<MH> col, int32_t seg, int32_t beg, int32_t end, int lane, float *lds,
                                            bool valid) {
  float s = 0.f;
#pragma unroll 4
  for (int32_t i = beg + lane; i < end; i += W) s += a.val[col(position<SIDE>(a, i))];
  s = combine<W, OpSum>(s, lds);
  if (lane == 0 && valid) a.out_seg[col(seg)] = s;
}

template <int BODY, int SIDE, int W, bool MH, typename ARGS>
__device__ __forceinline__ void run_segment(const ARGS &a, Col<MH> col, int32_t seg, int32_t beg, int32_t end, int lane, float *lds,
                                            bool valid) {
  if constexpr (BODY == kSegSoftmax) softmax_segment<SIDE, W>(a, col, seg, beg, end, lane, lds);
  else if constexpr (BODY == kSegSoftmaxBwd) softmax_bwd_segment<SIDE, W>(a, col, seg, beg, end, lane, lds, valid);
  else if constexpr (BODY == kSegSoftmaxDrop) softmax_segment<SIDE, W>(a, col, seg, beg, end, lane, lds, load_drop(a.drop));
  else if constexpr (BODY == kSegSoftmaxDropBwd)
    softmax_bwd_segment<SIDE, W>(a, col, seg, beg, end, lane, lds, valid, load_drop(a.drop));
  else if constexpr (BODY == kSegSoftmaxEntry) softmax_segment<SIDE, W>(a, col, seg, beg, end, lane, lds, NoDrop{}, Entry{a.entry});
  else if constexpr (BODY == kSegSoftmaxEntryBwd)
    softmax_bwd_segment<SIDE, W>(a, col, seg, beg, end, lane, lds, valid, NoDrop{}, Entry{a.entry});
  else if constexpr (BODY == kSegSoftmaxEntryDrop)
    softmax_segment<SIDE, W>(a, col, seg, beg, end, lane, lds, load_drop(a.drop), Entry{a.entry});
  else if constexpr (BODY == kSegSoftmaxEntryDropBwd)
    softmax_bwd_segment<SIDE, W>(a, col, seg, beg, end, lane, lds, valid, load_drop(a.drop), Entry{a.entry});
  else if constexpr (BODY == kSegStats)
    softmax_segment<SIDE, W, MH, NoDrop, NoEntry, true>(a, col, seg, beg, end, lane, lds, NoDrop{}, NoEntry{}, valid);
  else sum_segment<SIDE, W>(a, col, seg, beg, end, lane, lds, valid);
}

// The heads of a block: those derived from SegHeadsArgs carry the count, the others have one.
template <typename ARGS>
constexpr bool kHasHeads = std::is_base_of_v<SegHeadsArgs, ARGS>;
template <typename ARGS>
__host__ __device__ __forceinline__ int32_t heads_of(const ARGS &a) {
  if constexpr (kHasHeads<ARGS>) return a.heads;
  else return 1;
}
template <bool MH>
__device__ __forceinline__ Col<MH> column(int32_t H, int32_t h) {
  if constexpr (MH) return Col<true>{H, h};
  else return Col<false>{};
}

// Workgroups [0, nlong * H): one (long segment, head) each (they run longest, so they start first); the others: 256 / W
// lane groups, one (segment, head) each, head fastest.  Lanes without a pair of their own (past the last one, or a long
// segment's lane group) walk an empty range and take part in the butterflies: no lane leaves before the last cross-lane
// step.  A block without heads has H = 1 at compile time and counts in 32 bits; nseg * H may pass 2^31.
template <int BODY, int SIDE, int W, typename ARGS>
__global__ __launch_bounds__(kSegBlock) void segment_kernel(ARGS a) {
  constexpr bool kHeads = kHasHeads<ARGS>;
  using count_t = std::conditional_t<kHeads, int64_t, int32_t>;
  __shared__ float lds[kSegBlock / 64];
  const int32_t H = heads_of(a);
  const count_t nlong = (count_t)a.nlong * H;
  if ((count_t)blockIdx.x < nlong) {
    const int32_t seg = a.long_seg[blockIdx.x / H];
    run_segment<BODY, SIDE, kSegBlock>(a, column<kHeads>(H, (int32_t)(blockIdx.x % H)), seg, a.ptr[seg], a.ptr[seg + 1],
                                       (int)threadIdx.x, lds, true);
    return;
  }
  constexpr int kGroups = kSegBlock / W;
  const int64_t s = (int64_t)((count_t)blockIdx.x - nlong) * kGroups + (int)threadIdx.x / W;
  bool valid = s < (int64_t)a.nseg * H;
  const int32_t seg = valid ? (int32_t)(s / H) : 0;
  const int32_t h = valid ? (int32_t)(s % H) : 0;
  int32_t beg = 0, end = 0;
  if (valid) {
    beg = a.ptr[seg];
    end = a.ptr[seg + 1];
    if (end - beg > kSegLong) {  // a workgroup of its own has it
      beg = end = 0;
      valid = false;
    }
  }
  run_segment<BODY, SIDE, W>(a, column<kHeads>(H, h), seg, beg, end, (int)threadIdx.x % W, lds, valid);
}

template <int BODY, int SIDE, int W, typename ARGS>
void launch_one(unsigned nblocks, const ARGS &a, hipStream_t stream) {
  hipLaunchKernelGGL((segment_kernel<BODY, SIDE, W, ARGS>), dim3(nblocks), dim3(kSegBlock), 0, stream, a);
}

template <int BODY, int SIDE, typename ARGS>
hipError_t launch_width(int width, unsigned nblocks, const ARGS &a, hipStream_t stream) {
  switch (width) {
    case 4: launch_one<BODY, SIDE, 4>(nblocks, a, stream); break;
    case 8: launch_one<BODY, SIDE, 8>(nblocks, a, stream); break;
    case 16: launch_one<BODY, SIDE, 16>(nblocks, a, stream); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <int BODY, typename ARGS>
hipError_t launch_side(int side, int width, unsigned nblocks, const ARGS &a, hipStream_t stream) {
  return side == 0 ? launch_width<BODY, 0>(width, nblocks, a, stream) : launch_width<BODY, 1>(width, nblocks, a, stream);
}

}  // namespace

// The narrowest lane group that covers an average segment in one step: a wider one idles lanes on the typical segment
// (mean lengths are 3-6), a narrower one walks it in several dependent steps.
int seg_width(double mean) { return mean <= 4.0 ? 4 : mean <= 8.0 ? 8 : 16; }

template <typename ARGS>
hipError_t launch_segments(int body, int side, int width, const ARGS &a, hipStream_t stream) {
  const int64_t heads = heads_of(a);  // the work items are (segment, head) pairs
  if (heads < 1) return hipErrorInvalidValue;
  if (a.nseg <= 0) return hipSuccess;
  if (side < 0 || side > 1 || a.nlong < 0 || !a.ptr || (a.nlong > 0 && !a.long_seg)) return hipErrorInvalidValue;
  if (width != 4 && width != 8 && width != 16) return hipErrorInvalidValue;
  const int64_t groups = kSegBlock / width;
  const int64_t nblocks = a.nlong * heads + (a.nseg * heads + groups - 1) / groups;
  if (nblocks > 0x7fffffff) return hipErrorInvalidValue;
  if constexpr (std::is_same_v<ARGS, SegEntryArgs>) {
    if (!a.entry) return hipErrorInvalidValue;
    if ((body == kSegSoftmaxEntryDrop || body == kSegSoftmaxEntryDropBwd) && !a.drop.rng) return hipErrorInvalidValue;
    switch (body) {
      case kSegSoftmaxEntry: return launch_side<kSegSoftmaxEntry>(side, width, (unsigned)nblocks, a, stream);
      case kSegSoftmaxEntryBwd: return launch_side<kSegSoftmaxEntryBwd>(side, width, (unsigned)nblocks, a, stream);
      case kSegSoftmaxEntryDrop: return launch_side<kSegSoftmaxEntryDrop>(side, width, (unsigned)nblocks, a, stream);
      case kSegSoftmaxEntryDropBwd: return launch_side<kSegSoftmaxEntryDropBwd>(side, width, (unsigned)nblocks, a, stream);
    }
  } else if constexpr (std::is_base_of_v<SegDropArgs, ARGS> || std::is_base_of_v<SegDropHeadsArgs, ARGS>) {
    if (!a.drop.rng) return hipErrorInvalidValue;
    switch (body) {
      case kSegSoftmaxDrop: return launch_side<kSegSoftmaxDrop>(side, width, (unsigned)nblocks, a, stream);
      case kSegSoftmaxDropBwd: return launch_side<kSegSoftmaxDropBwd>(side, width, (unsigned)nblocks, a, stream);
    }
  } else {
    switch (body) {
      case kSegSoftmax: return launch_side<kSegSoftmax>(side, width, (unsigned)nblocks, a, stream);
      case kSegSoftmaxBwd: return launch_side<kSegSoftmaxBwd>(side, width, (unsigned)nblocks, a, stream);
      case kSegSum: return launch_side<kSegSum>(side, width, (unsigned)nblocks, a, stream);
      case kSegStats:
        if (!a.out_entry || !a.out_seg) return hipErrorInvalidValue;
        return launch_side<kSegStats>(side, width, (unsigned)nblocks, a, stream);
    }
  }
  return hipErrorInvalidValue;
}

template hipError_t launch_segments(int, int, int, const SegArgs &, hipStream_t);
template hipError_t launch_segments(int, int, int, const SegHeadsArgs &, hipStream_t);
template hipError_t launch_segments(int, int, int, const SegDropArgs &, hipStream_t);
template hipError_t launch_segments(int, int, int, const SegDropHeadsArgs &, hipStream_t);
template hipError_t launch_segments(int, int, int, const SegEntryArgs &, hipStream_t);

}  // namespace hg
