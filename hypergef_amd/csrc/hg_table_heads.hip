// Several attention heads over a dense neighbour table idx [rows, k] (include/hg_aggr.h, the hg_table_*_heads_f32 entries):
// the softmax, its backward and the segment sum, the two weighted sum gathers and the weight gradient's dot products, for
// H heads in one launch each.  Head is the fastest dimension of every score and coefficient array ([.., H]); head h owns
// the columns h Ch .. (h + 1) Ch - 1 of a feature row of F = H Ch columns.  Head h of every result is, bit for bit, what
// the single-head entry (hg_table_softmax.hip, hg_table.hip) gives on column h / on head h's columns: every kernel here
// keeps the single-head kernel's ownership, entry-to-lane assignment and order, and widens what a lane carries.
//
// Softmax family (SIDE, BODY as in hg_table_softmax.hip): a lane group of L lanes owns a segment, one entry per lane and
// pass, and a lane handles a slab of HV consecutive heads of its entry at once -- HV = 4 (one 16-byte load of the other
// end's score row and of entry_score, one 16-byte store of alpha) where H % 4 == 0 and the head-fastest arrays are 16-byte
// aligned, else 1.  The slab is the OUTER loop: a vertex segment keeps up to kSoftKeep logits x HV heads in registers
// across its three passes, and idx[p] / pos_v[q] are read once per slab.  The butterfly reduces the HV values together.
// A vertex segment of more than HG_TABLE_SEQ_MAX entries is taken by the whole workgroup, slab after slab, in the same
// launch.  No workspace, no atomics, no host list.
//
// Statistics (kBodyStats, hg_table_attention_stats_heads_f32): the softmax body stopped after its sum pass -- the same lanes,
// entries, butterflies and workgroup join, so the maximum m and inv = 1 / sum it stores per (segment, head) are the numbers
// the softmax multiplies with.  hg_table_attention.hip's gathers form alpha from them.
//
// Attention dropout (DROP, the hg_table_softmax_dropout_*_heads_f32 entries): a compile-time variant of the softmax and of its
// backward -- the same ownership, lanes, passes and reductions, so alpha, ds and dgroup keep their bits.  The mask of
// hg_philox.h is a function of (rng, p, h) alone.  A thread loads the two state words once, ahead of every segment.  The
// forward forms the mask only in its store pass, once per candidate (p, h), beside the alpha it scales: the maximum and sum
// passes know nothing of it.  The backward of a short segment masks dout where it loads it, into the registers that already
// hold the entry across the two passes -- one Philox per candidate (p, h); a long workgroup segment keeps no entries, so it
// forms the mask again in its second pass.  Non-candidates run no Philox: their lanes are off where it is computed.
//
// Gathers: table_gather_kernel's shape (16-byte lanes, kTableBatch row loads in flight, long rows through the LDS tree in
// the pieces the plain call has at the same F), the one weight per entry replaced by the weight of the lane's own head:
// w[p, c / Ch].  A 16-byte lane whose four columns share a head (Ch % 4 == 0) loads one weight an entry; one that straddles
// two heads keeps its 16-byte row load -- the long rows' pieces are a function of F and the alignment, not of Ch -- and loads
// a weight per column.  The lanes of a row group read w[p, .] from one run of 4 H bytes.
//
// Dot products: a lane group of L lanes (DOT ORDER at width Ch) owns one (table row, head); the H groups of a row are
// neighbours in the wave, so together they read A[j] / C[j] as one contiguous row of F columns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <string>
#include <type_traits>

#include "hg_aggr.h"
#include "hg_attention.h"
#include "hg_internal.h"
#include "hg_philox.h"
#include "hg_table.h"

namespace hg {
namespace {

constexpr int kSoftBlock = 64 * kTableWaves;
constexpr int kSoftMinL = 8;                         // side 1: the narrowest lane group (hg_table_softmax.hip's)
constexpr int kSoftKeep = kTableSeqMax / kSoftMinL;  // side 1: entries a lane keeps in registers, each HV heads wide
constexpr int kMaxHV = 4;

enum { kBodySoftmax = 0, kBodySoftmaxBwd = 1, kBodySum = 2, kBodyStats = 3 };

// V consecutive floats, one 16-byte access where V == 4
template <int V>
struct Vec {
  float v[V];
};

template <int V>
__device__ __forceinline__ Vec<V> vec_load(const float *p) {
  Vec<V> r;
  if constexpr (V == 4) {
    const float4 x = *reinterpret_cast<const float4 *>(p);
    r.v[0] = x.x;
    r.v[1] = x.y;
    r.v[2] = x.z;
    r.v[3] = x.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int V>
__device__ __forceinline__ void vec_store(float *p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = float4{v[0], v[1], v[2], v[3]};
  else *p = v[0];
}

// ---- softmax, its backward and the segment sum -----------------------------------------------------------------------------

struct HeadsSoftmaxArgs {
  const int32_t *idx, *ptr_v, *pos_v;
  const float *node, *edge, *entry;  // the scores [n, H], [rows, H], [rows k, H]; each may be null
  const float *val, *dval;           // backward: alpha and dalpha; sum: the summed values; [rows k, H]
  float *out_entry;                  // softmax: alpha; backward: ds; [rows k, H]
  float *out_seg;                    // backward: the segments' own sums of ds, or null; sum: out; [segments, H]
  const uint64_t *rng;               // dropout: {key, sid} in device memory, read when the kernel runs
  float *out_drop;                   // dropout, softmax: alpha after dropout; [rows k, H]
  uint32_t T;                        // dropout: an entry is kept where its Philox word >= T = floor(p_drop * 2^32)
  float scale;                       // dropout: 1 / (1 - p_drop), rounded once on the host
  float slope;
  int32_t rows, k, n, entries, nseg, H;
  int32_t L, R;                      // lanes per segment, segments per wave
  float *out_inv;                    // stats: 1 / the segment's sum, beside its maximum in out_seg; [segments, H]
};

template <int SIDE>
__device__ __forceinline__ void seg_range(const HeadsSoftmaxArgs &a, int seg, int &beg, int &end) {
  if (SIDE) {
    beg = max(a.ptr_v[seg], 0);
    end = min(a.ptr_v[seg + 1], a.entries);
  } else {
    beg = seg * a.k;
    end = beg + a.k;
  }
}

// Entry q of a segment: its table position p and the other end j, both 0 where the entry is no candidate
template <int SIDE>
__device__ __forceinline__ bool seg_entry(const HeadsSoftmaxArgs &a, int q, bool on, int &p, int &j) {
  if (SIDE) {
    p = a.pos_v[on ? q : 0];
    on = on && (unsigned)p < (unsigned)a.entries;
    p = on ? p : 0;
    j = p / a.k;
  } else {
    p = on ? q : 0;
    j = a.idx[p];
    on = on && (unsigned)j < (unsigned)a.n;
    j = on ? j : 0;
  }
  return on;
}

// raw = (own + other) + entry for the heads h0 .. h0 + HV - 1, the segment's own score first; an absent score is no addition
template <int SIDE, int HV>
__device__ __forceinline__ Vec<HV> seg_raw(const HeadsSoftmaxArgs &a, const Vec<HV> &own, int p, int j, int h0) {
  const float *other = SIDE ? a.edge : a.node;
  bool have = (SIDE ? a.node : a.edge) != nullptr;
  Vec<HV> raw;
#pragma unroll
  for (int i = 0; i < HV; ++i) raw.v[i] = have ? own.v[i] : 0.f;
  if (other) {
    const Vec<HV> o = vec_load<HV>(other + (size_t)j * a.H + h0);
#pragma unroll
    for (int i = 0; i < HV; ++i) raw.v[i] = have ? raw.v[i] + o.v[i] : o.v[i];
    have = true;
  }
  if (a.entry) {
    const Vec<HV> e = vec_load<HV>(a.entry + (size_t)p * a.H + h0);
#pragma unroll
    for (int i = 0; i < HV; ++i) raw.v[i] = have ? raw.v[i] + e.v[i] : e.v[i];
  }
  return raw;
}

template <bool MAX>
__device__ __forceinline__ float join(float x, float y) {
  return MAX ? fmaxf(x, y) : x + y;
}

// the butterfly of one lane group on HV values at once: every lane of the wave takes part
template <bool MAX, int HV>
__device__ __forceinline__ void group_join(float (&v)[HV], int L) {
  for (int o = L >> 1; o >= 1; o >>= 1)
#pragma unroll
    for (int i = 0; i < HV; ++i) v[i] = join<MAX>(v[i], __shfl_xor(v[i], o, 64));
}

// the whole workgroup: the wave's butterfly, one slot per wave and head, joined in ascending wave order by every thread
template <bool MAX, int HV>
__device__ __forceinline__ void block_join(float (&v)[HV], float (*slot)[kTableWaves][kMaxHV], int &buf, int w, int lane) {
  group_join<MAX, HV>(v, 64);
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < HV; ++i) slot[buf][w][i] = v[i];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < HV; ++i) {
    float r = slot[buf][0][i];
#pragma unroll
    for (int o = 1; o < kTableWaves; ++o) r = join<MAX>(r, slot[buf][o][i]);
    v[i] = r;
  }
  buf ^= 1;
}

// The dropout of a launch as a thread holds it: the state words, loaded once
struct NoDrop {};
struct Drop {
  DropRng rng;
  uint32_t T;
  float scale;
};

// v, the heads h0 .. h0 + HV - 1 of table position p, as dropout leaves it: fl(v * scale) where kept, else +0.  The caller
// runs it for candidates only.
template <int HV>
__device__ __forceinline__ void drop_slab(const Drop &d, int p, int h0, float (&v)[HV]) {
#pragma unroll
  for (int i = 0; i < HV; ++i) v[i] = drop_keep(d.rng, d.T, (uint32_t)p, (uint32_t)(h0 + i)) ? v[i] * d.scale : 0.f;
}

// The heads h0 .. h0 + HV - 1 of the segment a lane group owns whole: entries [beg, end) (none where the group is off),
// lane cl of L takes beg + cl + u L.  Every lane of the wave runs this, for the shuffles; NS: the entries a lane can hold.
template <int SIDE, int BODY, int NS, int HV, typename DROP>
__device__ __forceinline__ void group_segment(const HeadsSoftmaxArgs &a, const DROP &drop, int h0, int seg, bool act, int beg,
                                              int end, int L, int cl) {
  constexpr bool kDrop = std::is_same_v<DROP, Drop>;
  const int len = end - beg;
  const size_t H = (size_t)a.H;
  const float *own_score = SIDE ? a.node : a.edge;
  Vec<HV> own{};
  if (BODY != kBodySum && own_score && act) own = vec_load<HV>(own_score + (size_t)seg * H + h0);
  int pp[NS];  // the candidate's position, or -1
#pragma unroll
  for (int u = 0; u < NS; ++u) pp[u] = -1;

  if constexpr (BODY == kBodySoftmax || BODY == kBodyStats) {
    float x[NS][HV], m[HV], s[HV], o4[HV];
#pragma unroll
    for (int i = 0; i < HV; ++i) m[i] = -INFINITY;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool on = cl + u * L < len;
      if (NS > 1 && !__any(on)) break;
      int p, j;
      const bool ok = seg_entry<SIDE>(a, beg + cl + u * L, on, p, j);
      const Vec<HV> raw = seg_raw<SIDE, HV>(a, own, p, j, h0);
      pp[u] = ok ? p : -1;
#pragma unroll
      for (int i = 0; i < HV; ++i) {
        x[u][i] = leaky(raw.v[i], a.slope);
        m[i] = ok ? fmaxf(m[i], x[u][i]) : m[i];
      }
    }
    group_join<true, HV>(m, L);
#pragma unroll
    for (int i = 0; i < HV; ++i) s[i] = 0.f;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      if (NS > 1 && !__any(cl + u * L < len)) break;
#pragma unroll
      for (int i = 0; i < HV; ++i) {
        x[u][i] = __expf(x[u][i] - m[i]);
        s[i] = pp[u] >= 0 ? s[i] + x[u][i] : s[i];
      }
    }
    group_join<false, HV>(s, L);
    float inv[HV];  // the maximum's entry contributes exp(0) = 1: s >= 1 wherever inv is used
#pragma unroll
    for (int i = 0; i < HV; ++i) inv[i] = 1.f / s[i];
    if constexpr (BODY == kBodyStats) {  // s == 0: no candidate added anything, and nothing reads the pair
#pragma unroll
      for (int i = 0; i < HV; ++i) {
        o4[i] = s[i] == 0.f ? 0.f : m[i];
        inv[i] = s[i] == 0.f ? 0.f : inv[i];
      }
      if (act && cl == 0) {
        vec_store<HV>(a.out_seg + (size_t)seg * H + h0, o4);
        vec_store<HV>(a.out_inv + (size_t)seg * H + h0, inv);
      }
      return;
    }
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool on = cl + u * L < len;
      if (NS > 1 && !__any(on)) break;
#pragma unroll
      for (int i = 0; i < HV; ++i) o4[i] = pp[u] >= 0 ? x[u][i] * inv[i] : 0.f;
      if (SIDE) {
        if (pp[u] >= 0) vec_store<HV>(a.out_entry + (size_t)pp[u] * H + h0, o4);
      } else if (on) {
        vec_store<HV>(a.out_entry + (size_t)(beg + cl + u * L) * H + h0, o4);
      }
      if constexpr (kDrop) {  // the mask: here and nowhere else, once per candidate (p, h); o4 is +0 elsewhere
        if (pp[u] >= 0) drop_slab<HV>(drop, pp[u], h0, o4);
        if (SIDE) {
          if (pp[u] >= 0) vec_store<HV>(a.out_drop + (size_t)pp[u] * H + h0, o4);
        } else if (on) {
          vec_store<HV>(a.out_drop + (size_t)(beg + cl + u * L) * H + h0, o4);
        }
      }
    }
  } else if constexpr (BODY == kBodySoftmaxBwd) {
    float av[NS][HV], dv[NS][HV], gv[NS][HV], dot[HV], dsum[HV], o4[HV];
#pragma unroll
    for (int i = 0; i < HV; ++i) dot[i] = 0.f;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool on = cl + u * L < len;
      if (NS > 1 && !__any(on)) break;
      int p, j;
      const bool ok = seg_entry<SIDE>(a, beg + cl + u * L, on, p, j);
      const Vec<HV> raw = seg_raw<SIDE, HV>(a, own, p, j, h0);
      const Vec<HV> al = vec_load<HV>(a.val + (size_t)p * H + h0);
      Vec<HV> da = vec_load<HV>(a.dval + (size_t)p * H + h0);
      if constexpr (kDrop) {  // dalpha = keep ? fl(dout * scale) : +0, kept in dv for both passes
        if (ok) drop_slab<HV>(drop, p, h0, da.v);
      }
      pp[u] = ok ? p : -1;
#pragma unroll
      for (int i = 0; i < HV; ++i) {
        gv[u][i] = raw.v[i] > 0.f ? 1.f : a.slope;
        av[u][i] = al.v[i];
        dv[u][i] = da.v[i];
        dot[i] = ok ? dot[i] + av[u][i] * dv[u][i] : dot[i];
      }
    }
    group_join<false, HV>(dot, L);
#pragma unroll
    for (int i = 0; i < HV; ++i) dsum[i] = 0.f;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool on = cl + u * L < len;
      if (NS > 1 && !__any(on)) break;
#pragma unroll
      for (int i = 0; i < HV; ++i) {
        const float ds = (av[u][i] * (dv[u][i] - dot[i])) * gv[u][i];
        dsum[i] = pp[u] >= 0 ? dsum[i] + ds : dsum[i];
        o4[i] = pp[u] >= 0 ? ds : 0.f;
      }
      if (SIDE) {
        if (pp[u] >= 0) vec_store<HV>(a.out_entry + (size_t)pp[u] * H + h0, o4);
      } else if (on) {
        vec_store<HV>(a.out_entry + (size_t)(beg + cl + u * L) * H + h0, o4);
      }
    }
    if (a.out_seg) {
      group_join<false, HV>(dsum, L);
      if (act && cl == 0) vec_store<HV>(a.out_seg + (size_t)seg * H + h0, dsum);
    }
  } else {
    float s[HV];
#pragma unroll
    for (int i = 0; i < HV; ++i) s[i] = 0.f;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool on = cl + u * L < len;
      if (NS > 1 && !__any(on)) break;
      int p, j;
      const bool ok = seg_entry<SIDE>(a, beg + cl + u * L, on, p, j);
      const Vec<HV> v = vec_load<HV>(a.val + (size_t)p * H + h0);
#pragma unroll
      for (int i = 0; i < HV; ++i) s[i] = ok ? s[i] + v.v[i] : s[i];
    }
    group_join<false, HV>(s, L);
    if (act && cl == 0) vec_store<HV>(a.out_seg + (size_t)seg * H + h0, s);
  }
}

// The heads h0 .. h0 + HV - 1 of one side-1 segment of more than HG_TABLE_SEQ_MAX entries, by the whole workgroup: thread
// t takes beg + t, beg + t + 256 .. and gathers its logits again in every pass.
template <int BODY, int HV, typename DROP>
__device__ __forceinline__ void block_segment(const HeadsSoftmaxArgs &a, const DROP &drop, int h0, int seg, int beg, int end,
                                              int t, float (*slot)[kTableWaves][kMaxHV], int &buf) {
  constexpr bool kDrop = std::is_same_v<DROP, Drop>;
  const int w = t >> 6, lane = t & 63;
  const unsigned len = (unsigned)(end - beg);
  const size_t H = (size_t)a.H;
  Vec<HV> own{};
  if (BODY != kBodySum && a.node) own = vec_load<HV>(a.node + (size_t)seg * H + h0);
  int p, j;
  if constexpr (BODY == kBodySoftmax || BODY == kBodyStats) {
    float m[HV], s[HV], inv[HV], o4[HV];
#pragma unroll
    for (int i = 0; i < HV; ++i) m[i] = -INFINITY;
    for (unsigned o = t; o < len; o += kSoftBlock) {
      const bool ok = seg_entry<1>(a, beg + (int)o, true, p, j);
      const Vec<HV> raw = seg_raw<1, HV>(a, own, p, j, h0);
#pragma unroll
      for (int i = 0; i < HV; ++i) m[i] = ok ? fmaxf(m[i], leaky(raw.v[i], a.slope)) : m[i];
    }
    block_join<true, HV>(m, slot, buf, w, lane);
#pragma unroll
    for (int i = 0; i < HV; ++i) s[i] = 0.f;
    for (unsigned o = t; o < len; o += kSoftBlock) {
      const bool ok = seg_entry<1>(a, beg + (int)o, true, p, j);
      const Vec<HV> raw = seg_raw<1, HV>(a, own, p, j, h0);
#pragma unroll
      for (int i = 0; i < HV; ++i) {
        const float e = __expf(leaky(raw.v[i], a.slope) - m[i]);
        s[i] = ok ? s[i] + e : s[i];
      }
    }
    block_join<false, HV>(s, slot, buf, w, lane);
#pragma unroll
    for (int i = 0; i < HV; ++i) inv[i] = 1.f / s[i];
    if constexpr (BODY == kBodyStats) {
#pragma unroll
      for (int i = 0; i < HV; ++i) {
        o4[i] = s[i] == 0.f ? 0.f : m[i];
        inv[i] = s[i] == 0.f ? 0.f : inv[i];
      }
      if (t == 0) {
        vec_store<HV>(a.out_seg + (size_t)seg * H + h0, o4);
        vec_store<HV>(a.out_inv + (size_t)seg * H + h0, inv);
      }
      return;
    }
    for (unsigned o = t; o < len; o += kSoftBlock) {
      const bool ok = seg_entry<1>(a, beg + (int)o, true, p, j);
      const Vec<HV> raw = seg_raw<1, HV>(a, own, p, j, h0);
#pragma unroll
      for (int i = 0; i < HV; ++i) o4[i] = __expf(leaky(raw.v[i], a.slope) - m[i]) * inv[i];
      if (ok) vec_store<HV>(a.out_entry + (size_t)p * H + h0, o4);
      if constexpr (kDrop) {
        if (ok) {
          drop_slab<HV>(drop, p, h0, o4);
          vec_store<HV>(a.out_drop + (size_t)p * H + h0, o4);
        }
      }
    }
  } else if constexpr (BODY == kBodySoftmaxBwd) {
    float dot[HV], dsum[HV], o4[HV];
#pragma unroll
    for (int i = 0; i < HV; ++i) dot[i] = 0.f;
    for (unsigned o = t; o < len; o += kSoftBlock) {
      const bool ok = seg_entry<1>(a, beg + (int)o, true, p, j);
      const Vec<HV> al = vec_load<HV>(a.val + (size_t)p * H + h0);
      Vec<HV> da = vec_load<HV>(a.dval + (size_t)p * H + h0);
      if constexpr (kDrop) {
        if (ok) drop_slab<HV>(drop, p, h0, da.v);
      }
#pragma unroll
      for (int i = 0; i < HV; ++i) {
        const float term = al.v[i] * da.v[i];
        dot[i] = ok ? dot[i] + term : dot[i];
      }
    }
    block_join<false, HV>(dot, slot, buf, w, lane);
#pragma unroll
    for (int i = 0; i < HV; ++i) dsum[i] = 0.f;
    for (unsigned o = t; o < len; o += kSoftBlock) {
      const bool ok = seg_entry<1>(a, beg + (int)o, true, p, j);
      const Vec<HV> raw = seg_raw<1, HV>(a, own, p, j, h0);
      const Vec<HV> al = vec_load<HV>(a.val + (size_t)p * H + h0);
      Vec<HV> da = vec_load<HV>(a.dval + (size_t)p * H + h0);
      if constexpr (kDrop) {  // no entry is kept between the passes of a long segment: the mask is formed again
        if (ok) drop_slab<HV>(drop, p, h0, da.v);
      }
#pragma unroll
      for (int i = 0; i < HV; ++i) {
        const float g = raw.v[i] > 0.f ? 1.f : a.slope;
        const float ds = (al.v[i] * (da.v[i] - dot[i])) * g;
        dsum[i] = ok ? dsum[i] + ds : dsum[i];
        o4[i] = ds;
      }
      if (ok) vec_store<HV>(a.out_entry + (size_t)p * H + h0, o4);
    }
    if (a.out_seg) {
      block_join<false, HV>(dsum, slot, buf, w, lane);
      if (t == 0) vec_store<HV>(a.out_seg + (size_t)seg * H + h0, dsum);
    }
  } else {
    float s[HV];
#pragma unroll
    for (int i = 0; i < HV; ++i) s[i] = 0.f;
    for (unsigned o = t; o < len; o += kSoftBlock) {
      const bool ok = seg_entry<1>(a, beg + (int)o, true, p, j);
      const Vec<HV> v = vec_load<HV>(a.val + (size_t)p * H + h0);
#pragma unroll
      for (int i = 0; i < HV; ++i) s[i] = ok ? s[i] + v.v[i] : s[i];
    }
    block_join<false, HV>(s, slot, buf, w, lane);
    if (t == 0) vec_store<HV>(a.out_seg + (size_t)seg * H + h0, s);
  }
}

template <int SIDE, int BODY, int HV, bool DROP = false>
__global__ __launch_bounds__(kSoftBlock) void table_softmax_heads_kernel(HeadsSoftmaxArgs a) {
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int L = a.L, R = a.R, H = a.H;
  const int sub = lane / L, cl = lane - sub * L;
  const int RW = R * kTableWaves;
  using DropT = std::conditional_t<DROP, Drop, NoDrop>;
  DropT drop{};
  if constexpr (DROP) drop = Drop{drop_rng(a.rng[0], a.rng[1]), a.T, a.scale};  // both state words, once per thread

  if constexpr (SIDE == 1 && BODY != kBodySum && BODY != kBodyStats) {
    // the positions no vertex owns, every head of them: this workgroup's slice of the table
    const int64_t chunk = ((int64_t)a.entries + gridDim.x - 1) / gridDim.x;
    const int64_t pb = (int64_t)blockIdx.x * chunk, pe = min(pb + chunk, (int64_t)a.entries);
    for (int64_t e = pb * H + t; e < pe * H; e += kSoftBlock)
      if ((unsigned)a.idx[e / H] >= (unsigned)a.n) {
        a.out_entry[e] = 0.f;
        if constexpr (DROP && BODY == kBodySoftmax) a.out_drop[e] = 0.f;
      }
  }

  const int64_t seg0 = (int64_t)blockIdx.x * RW;
  const int64_t seg64 = seg0 + w * R + sub;
  const bool seg_on = seg64 < a.nseg;
  const int seg = seg_on ? (int)seg64 : 0;
  int beg = 0, end = 0;
  if (seg_on) seg_range<SIDE>(a, seg, beg, end);
  const bool is_long = SIDE == 1 && end - beg > kTableSeqMax;
  const bool act = seg_on && !is_long;
  for (int h0 = 0; h0 < H; h0 += HV)
    group_segment<SIDE, BODY, SIDE ? kSoftKeep : 1, HV>(a, drop, h0, seg, act, beg, act ? end : beg, L, cl);

  if constexpr (SIDE == 1) {
    __shared__ float slot[2][kTableWaves][kMaxHV];
    __shared__ unsigned long long long_rows[kTableWaves];
    const unsigned long long mine = __ballot(seg_on && is_long && cl == 0);
    if (lane == 0) long_rows[w] = mine;
    __syncthreads();
    int buf = 0;
    for (int ww = 0; ww < kTableWaves; ++ww) {
      const unsigned long long mm = long_rows[ww];
      unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)mm), hi = __builtin_amdgcn_readfirstlane((unsigned)(mm >> 32));
      unsigned long long m = ((unsigned long long)hi << 32) | lo;
      while (m) {
        const int ln = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int lseg = (int)(seg0 + ww * R + ln / L);
        int lbeg, lend;
        seg_range<1>(a, lseg, lbeg, lend);
        for (int h0 = 0; h0 < H; h0 += HV) block_segment<BODY, HV>(a, drop, h0, lseg, lbeg, lend, t, slot, buf);
      }
    }
  }
}

int pow2_at_least(int k) {
  int L = 1;
  while (L < k) L <<= 1;
  return L;
}

bool aligned16(std::initializer_list<const void *> arrays) {
  for (const void *p : arrays)
    if ((uintptr_t)p % 16) return false;
  return true;
}

template <int BODY, bool DROP = false>
int launch_softmax_heads(const char *entry, int side, HeadsSoftmaxArgs a, hg_stream_t stream) {
  a.entries = a.rows * a.k;
  a.nseg = side ? a.n : a.rows;
  a.L = side ? std::max(kSoftMinL, pow2_at_least(a.k)) : pow2_at_least(a.k);  // the single-head call's, per head
  a.R = 64 / a.L;
  const int RW = a.R * kTableWaves;
  const bool slab4 = a.H % 4 == 0 && aligned16({a.node, a.edge, a.entry, a.val, a.dval, a.out_entry, a.out_seg, a.out_drop, a.out_inv});
  const dim3 grid((unsigned)(((int64_t)a.nseg + RW - 1) / RW)), block(kSoftBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (side && slab4) hipLaunchKernelGGL((table_softmax_heads_kernel<1, BODY, 4, DROP>), grid, block, 0, s, a);
  else if (side) hipLaunchKernelGGL((table_softmax_heads_kernel<1, BODY, 1, DROP>), grid, block, 0, s, a);
  else if (slab4) hipLaunchKernelGGL((table_softmax_heads_kernel<0, BODY, 4, DROP>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((table_softmax_heads_kernel<0, BODY, 1, DROP>), grid, block, 0, s, a);
  return launch_check(entry);
}

int heads_refusal(const char *entry, int32_t heads) {
  if (heads < 1) return fail(entry, HG_ERR_INVALID, "heads must be at least 1, got " + std::to_string(heads));
  return HG_OK;
}

// what the three entries refuse, in the single-head entries' order with the heads after the sizes
struct DropCall {  // what a dropout entry adds to the call
  float p_drop;
  const uint64_t *rng_dev;
};

// drop (the dropout entries; else null): p_drop and the state's address, after the null pointers and before the sizes
int softmax_refusal(const char *entry, const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t heads, int32_t side,
                    const char *side_name, const int32_t *ptr_v, const int32_t *pos_v, bool arrays_given, const char *null_text,
                    std::initializer_list<const void *> arrays, const DropCall *drop = nullptr) {
  if (!idx) return fail(entry, HG_ERR_INVALID, "null idx");
  if (!arrays_given) return fail(entry, HG_ERR_INVALID, null_text);
  if (side == HG_TABLE_VERTEX && (!ptr_v || !pos_v))
    return fail(entry, HG_ERR_INVALID, std::string("null ptr_v or pos_v (") + side_name + " = HG_TABLE_VERTEX walks the transpose)");
  if (drop) {
    if (!(drop->p_drop >= 0.f && drop->p_drop < 1.f))  // NaN fails both comparisons
      return fail(entry, HG_ERR_INVALID, "p_drop must lie in [0, 1) (at 1 the scale 1 / (1 - p_drop) is infinite)");
    if (!drop->rng_dev || (uintptr_t)drop->rng_dev % 8) return fail(entry, HG_ERR_INVALID, "rng_dev is null or not 8-byte aligned");
  }
  if (const int st = size_refusal(entry, rows, k, n, 1)) return st;
  if (const int st = heads_refusal(entry, heads)) return st;
  if (side != HG_TABLE_HYPEREDGE && side != HG_TABLE_VERTEX)
    return fail(entry, HG_ERR_INVALID,
                std::string(side_name) + " must be HG_TABLE_HYPEREDGE or HG_TABLE_VERTEX, got " + std::to_string(side));
  for (const void *p : {(const void *)idx, (const void *)ptr_v, (const void *)pos_v})
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, "the table, its transpose and every array must be 4-byte aligned");
  for (const void *p : arrays)
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, "the table, its transpose and every array must be 4-byte aligned");
  return HG_OK;
}

HeadsSoftmaxArgs softmax_args(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t heads, const float *node,
                              const float *edge, const float *entry_score, float slope, const int32_t *ptr_v,
                              const int32_t *pos_v) {
  HeadsSoftmaxArgs a{};
  a.idx = idx;
  a.ptr_v = ptr_v;
  a.pos_v = pos_v;
  a.node = node;
  a.edge = edge;
  a.entry = entry_score;
  a.slope = slope;
  a.rows = rows;
  a.k = k;
  a.n = n;
  a.H = heads;
  return a;
}

// ---- the two sum gathers with a weight per entry and head --------------------------------------------------------------------

struct HeadsGatherArgs {
  const int32_t *idx;            // the table [rows, k] (the hyperedge gather)
  const int32_t *ptr_v, *pos_v;  // its transpose (the vertex gather)
  const float *src, *w, *src_scale, *dst_scale;  // w [rows k, H], never null
  float *dst;
  int32_t nrows, nsrc;  // destination and source rows
  int32_t k, F, entries, H, Ch;
  int32_t L, R;         // lanes per row, rows per wave: the plain gathers' at this F
  int32_t P2;           // the power of two at or above kTableWaves R
};

// acc += the terms of the entries [beg, end), ascending, for the columns c .. c + V - 1: table_row_sum of hg_table.hip with
// the weight of each column's head.  WN weights an entry: 1 where the lane's columns share a head, else V.
template <bool T, int V, int WN>
__device__ __forceinline__ void heads_row_sum(const HeadsGatherArgs &a, int beg, int end, int c, float (&acc)[V]) {
  int hd[WN];
#pragma unroll
  for (int i = 0; i < WN; ++i) hd[i] = (c + i) / a.Ch;
  for (int b = beg; b < end; b += kTableBatch) {
    Vec<V> x[kTableBatch];
    float wv[kTableBatch][WN], sv[kTableBatch];
    bool ok[kTableBatch];
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u) {
      const int q = b + u;
      bool o = q < end;
      int p, j;
      if (T) {
        p = a.pos_v[o ? q : 0];
        o = o && (unsigned)p < (unsigned)a.entries;
        p = o ? p : 0;
        j = p / a.k;
      } else {
        p = o ? q : 0;
        j = a.idx[p];
        o = o && (unsigned)j < (unsigned)a.nsrc;
        j = o ? j : 0;
      }
      ok[u] = o;
#pragma unroll
      for (int i = 0; i < WN; ++i) wv[u][i] = a.w[(size_t)p * a.H + hd[i]];
      sv[u] = a.src_scale ? a.src_scale[j] : 1.f;
      x[u] = vec_load<V>(a.src + (size_t)j * a.F + c);
    }
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float term = x[u].v[i];
        if (a.src_scale) term = term * sv[u];
        term = term * wv[u][WN == 1 ? 0 : i];
        acc[i] = ok[u] ? acc[i] + term : acc[i];
      }
  }
}

template <bool T, int V, int WN>
__global__ __launch_bounds__(64 * kTableWaves) void table_gather_heads_kernel(HeadsGatherArgs a) {
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int L = a.L, R = a.R, F = a.F;
  const int sub = lane / L, cl = lane - sub * L;
  const bool lane_on = sub < R;
  const int RW = R * kTableWaves;
  const int64_t row0 = (int64_t)blockIdx.x * RW;
  const int64_t row64 = row0 + w * R + sub;
  const bool row_on = lane_on && row64 < a.nrows;
  const int row = row_on ? (int)row64 : 0;
  int beg = 0, end = 0;
  if (row_on) {
    if (T) {
      beg = max(a.ptr_v[row], 0);
      end = min(a.ptr_v[row + 1], a.entries);
    } else {
      beg = row * a.k;
      end = beg + a.k;
    }
  }
  const bool is_long = T && end - beg > kTableSeqMax;

  if (row_on && !is_long) {
    const float ds = a.dst_scale ? a.dst_scale[row] : 1.f;
    for (int c0 = 0; c0 < F; c0 += L * V) {  // with F > 64 V a lane's head changes between the passes
      const int c = c0 + cl * V;
      if (c >= F) continue;
      float acc[V];
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] = 0.f;
      heads_row_sum<T, V, WN>(a, beg, end, c, acc);
      if (a.dst_scale && end > beg) {  // an empty row stays +0.0 whatever its scale
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = ds * acc[i];
      }
      vec_store<V>(a.dst + (size_t)row * F + c, acc);
    }
  }

  if constexpr (T) {
    // the tile's long rows, one after the other, by the whole workgroup: the plain gather's pieces and tree
    __shared__ __attribute__((aligned(16))) float part[kTableWaves * 64 * V];
    __shared__ unsigned long long long_rows[kTableWaves];
    const unsigned long long mine = __ballot(row_on && is_long && cl == 0);
    if (lane == 0) long_rows[w] = mine;
    __syncthreads();
    const int P = RW, g = w * R + sub;
    for (int ww = 0; ww < kTableWaves; ++ww) {
      const unsigned long long mm = long_rows[ww];
      unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)mm), hi = __builtin_amdgcn_readfirstlane((unsigned)(mm >> 32));
      unsigned long long m = ((unsigned long long)hi << 32) | lo;
      while (m) {
        const int ln = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int lrow = (int)(row0 + ww * R + ln / L);
        const int lbeg = max(a.ptr_v[lrow], 0), lend = min(a.ptr_v[lrow + 1], a.entries);
        const int64_t len = lend - lbeg, chunk = (len + P - 1) / P;
        const int gb = lbeg + (int)min((int64_t)g * chunk, len), ge = lbeg + (int)min((int64_t)(g + 1) * chunk, len);
        const float ds = a.dst_scale ? a.dst_scale[lrow] : 1.f;
        for (int c0 = 0; c0 < F; c0 += L * V) {
          const int c = c0 + cl * V;
          const bool on = lane_on && c < F;
          float *mypart = part + (size_t)(g * L + cl) * V;
          if (on) {
            float acc[V];
#pragma unroll
            for (int i = 0; i < V; ++i) acc[i] = 0.f;
            heads_row_sum<T, V, WN>(a, gb, ge, c, acc);
#pragma unroll
            for (int i = 0; i < V; ++i) mypart[i] = acc[i];
          }
          __syncthreads();
          for (int s = a.P2 >> 1; s >= 1; s >>= 1) {
            if (on && g < s && g + s < P) {
              const float *other = part + (size_t)((g + s) * L + cl) * V;
#pragma unroll
              for (int i = 0; i < V; ++i) mypart[i] = mypart[i] + other[i];
            }
            __syncthreads();
          }
          if (on && g == 0) {
            float out[V];
#pragma unroll
            for (int i = 0; i < V; ++i) out[i] = a.dst_scale ? ds * mypart[i] : mypart[i];
            vec_store<V>(a.dst + (size_t)lrow * F + c, out);
          }
          __syncthreads();
        }
      }
    }
  }
}

// what the two gathers refuse about the table and the rows, in the plain gathers' order with the heads after the sizes
int gather_refusal(const char *entry, int32_t rows, int32_t k, int32_t n, int32_t F, int32_t heads, const float *src,
                   const float *w, const float *src_scale, const float *dst_scale, const float *dst) {
  if (!src || !dst) return fail(entry, HG_ERR_INVALID, "null src or dst");
  if (!w) return fail(entry, HG_ERR_INVALID, "null w (without weights the plain entry is the call)");
  if (const int st = size_refusal(entry, rows, k, n, F)) return st;
  if (const int st = heads_refusal(entry, heads)) return st;
  if (F % heads) return fail(entry, HG_ERR_INVALID, "F = " + std::to_string(F) + " is no multiple of heads = " + std::to_string(heads));
  for (const void *p : {(const void *)src, (const void *)w, (const void *)src_scale, (const void *)dst_scale, (const void *)dst})
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, "src, w, the scales and dst must be 4-byte aligned");
  return HG_OK;
}

template <bool T>
int launch_gather_heads(const char *entry, const int32_t *idx, const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k,
                        int32_t n, int32_t F, int32_t heads, const float *src, const float *w, const float *src_scale,
                        const float *dst_scale, float *dst, hg_stream_t stream) {
  HeadsGatherArgs a{};
  a.idx = idx;
  a.ptr_v = ptr_v;
  a.pos_v = pos_v;
  a.src = src;
  a.w = w;
  a.src_scale = src_scale;
  a.dst_scale = dst_scale;
  a.dst = dst;
  a.nrows = T ? n : rows;
  a.nsrc = T ? rows : n;
  a.k = k;
  a.F = F;
  a.H = heads;
  a.Ch = F / heads;
  a.entries = rows * k;
  // the geometry is the plain gathers' at this F: the long rows' pieces and tree follow from it
  const bool vec4 = F % 4 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
  const int V = vec4 ? 4 : 1;
  a.L = std::min((F + V - 1) / V, 64);
  a.R = 64 / a.L;
  a.P2 = 1;
  while (a.P2 < a.R * kTableWaves) a.P2 <<= 1;
  const int RW = a.R * kTableWaves;
  const dim3 grid((unsigned)(((int64_t)a.nrows + RW - 1) / RW)), block(64 * kTableWaves);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec4 && a.Ch % 4 == 0) hipLaunchKernelGGL((table_gather_heads_kernel<T, 4, 1>), grid, block, 0, s, a);
  else if (vec4) hipLaunchKernelGGL((table_gather_heads_kernel<T, 4, 4>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((table_gather_heads_kernel<T, 1, 1>), grid, block, 0, s, a);
  return launch_check(entry);
}

// ---- the dot products of a table's entries, per head ---------------------------------------------------------------------------

struct HeadsDotArgs {
  const int32_t *idx;
  const float *A, *a_scale, *B, *C, *D;
  float *out;  // [rows k, H]
  int32_t rows, n, k, F, H, Ch;
  int32_t L, R;  // lanes per (table row, head) (a power of two), such groups per wave
};

// out[p, h] = a_scale[j] <A[j, head h], B[i, head h]> + <C[j, head h], D[i, head h]>: table_dot_kernel of hg_table.hip at
// width Ch on the columns h Ch .. of rows F apart.  Lane group G of the launch owns (table row G / H, head G % H), so the
// groups of a row follow each other and their loads of A[j] / C[j] cover the row end to end.
template <int V, bool TWO>
__global__ __launch_bounds__(64 * kTableWaves) void table_dot_heads_kernel(HeadsDotArgs a) {
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int L = a.L, R = a.R, F = a.F, Ch = a.Ch, k = a.k, H = a.H;
  const int sub = lane / L, cl = lane - sub * L;
  const int64_t G = ((int64_t)blockIdx.x * kTableWaves + w) * R + sub;
  const bool row_on = G < (int64_t)a.rows * H;  // a whole lane group is on or off; an off group computes (0, 0), stores nothing
  const int row = row_on ? (int)(G / H) : 0;
  const int hc = (row_on ? (int)(G % H) : 0) * Ch;  // the head's first column
  const int step = L * V;
  const bool one_pass = Ch <= step;
  const int cfirst = cl * V;
  const bool on0 = cfirst < Ch;
  const size_t brow = (size_t)row * F + hc;
  const Vec<V> b0 = vec_load<V>(a.B + brow + (on0 ? cfirst : 0));
  Vec<V> d0{};
  if constexpr (TWO) d0 = vec_load<V>(a.D + brow + (on0 ? cfirst : 0));
  for (int s0 = 0; s0 < k; s0 += kTableDotBatch) {
    int jv[kTableDotBatch];
    bool ok[kTableDotBatch];
    float sc[kTableDotBatch], s1[kTableDotBatch], s2[kTableDotBatch];
#pragma unroll
    for (int u = 0; u < kTableDotBatch; ++u) {
      const int s = s0 + u;
      const int j = a.idx[(size_t)row * k + (s < k ? s : 0)];
      ok[u] = s < k && (unsigned)j < (unsigned)a.n;
      jv[u] = ok[u] ? j : 0;
      sc[u] = a.a_scale ? a.a_scale[jv[u]] : 1.f;
      s1[u] = 0.f;
      s2[u] = 0.f;
    }
    for (int c0 = 0; c0 < Ch; c0 += step) {
      const int c = c0 + cfirst;
      const bool on = c < Ch;
      const int ce = on ? c : 0;
      Vec<V> bv = b0, dv = d0;
      if (!one_pass && c0 > 0) {
        bv = vec_load<V>(a.B + brow + ce);
        if constexpr (TWO) dv = vec_load<V>(a.D + brow + ce);
      }
      Vec<V> av[kTableDotBatch], cv[kTableDotBatch];
#pragma unroll
      for (int u = 0; u < kTableDotBatch; ++u) {
        av[u] = vec_load<V>(a.A + (size_t)jv[u] * F + hc + ce);
        if constexpr (TWO) cv[u] = vec_load<V>(a.C + (size_t)jv[u] * F + hc + ce);
      }
#pragma unroll
      for (int u = 0; u < kTableDotBatch; ++u)
#pragma unroll
        for (int i = 0; i < V; ++i) {
          s1[u] = on ? __builtin_fmaf(av[u].v[i], bv.v[i], s1[u]) : s1[u];
          if constexpr (TWO) s2[u] = on ? __builtin_fmaf(cv[u].v[i], dv.v[i], s2[u]) : s2[u];
        }
    }
#pragma unroll
    for (int u = 0; u < kTableDotBatch; ++u) {
      float tt = a.a_scale ? sc[u] * s1[u] : s1[u];
      if constexpr (TWO) tt = tt + s2[u];
      for (int o = L >> 1; o >= 1; o >>= 1) tt = tt + __shfl_xor(tt, o, 64);
      if (row_on && cl == 0 && s0 + u < k) a.out[((size_t)row * k + s0 + u) * H + hc / Ch] = ok[u] ? tt : 0.f;
    }
  }
}

}  // namespace
}  // namespace hg

extern "C" {

int hg_table_softmax_heads_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t heads, int32_t group,
                               const float *node_score, const float *edge_score, const float *entry_score, float slope,
                               const int32_t *ptr_v, const int32_t *pos_v, float *alpha, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_softmax_heads_f32";
  if (const int st = softmax_refusal(entry, idx, rows, k, n, heads, group, "group", ptr_v, pos_v,
                                     alpha && (node_score || edge_score || entry_score),
                                     "null alpha, or node_score, edge_score and entry_score all null",
                                     {node_score, edge_score, entry_score, alpha}))
    return st;
  HeadsSoftmaxArgs a = softmax_args(idx, rows, k, n, heads, node_score, edge_score, entry_score, slope, ptr_v, pos_v);
  a.out_entry = alpha;
  return launch_softmax_heads<kBodySoftmax>(entry, group, a, stream);
}

int hg_table_softmax_bwd_heads_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t heads, int32_t group,
                                   const float *node_score, const float *edge_score, const float *entry_score, float slope,
                                   const int32_t *ptr_v, const int32_t *pos_v, const float *alpha, const float *dalpha,
                                   float *ds, float *dgroup, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_softmax_bwd_heads_f32";
  if (const int st = softmax_refusal(entry, idx, rows, k, n, heads, group, "group", ptr_v, pos_v,
                                     alpha && dalpha && ds && (node_score || edge_score || entry_score),
                                     "null alpha, dalpha or ds, or node_score, edge_score and entry_score all null",
                                     {node_score, edge_score, entry_score, alpha, dalpha, ds, dgroup}))
    return st;
  HeadsSoftmaxArgs a = softmax_args(idx, rows, k, n, heads, node_score, edge_score, entry_score, slope, ptr_v, pos_v);
  a.val = alpha;
  a.dval = dalpha;
  a.out_entry = ds;
  a.out_seg = dgroup;
  return launch_softmax_heads<kBodySoftmaxBwd>(entry, group, a, stream);
}

int hg_table_softmax_dropout_heads_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t heads, int32_t group,
                                       const float *node_score, const float *edge_score, const float *entry_score, float slope,
                                       float p_drop, const uint64_t *rng_dev, const int32_t *ptr_v, const int32_t *pos_v,
                                       float *alpha_out, float *alpha_drop_out, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_softmax_dropout_heads_f32";
  const DropCall drop{p_drop, rng_dev};
  if (const int st = softmax_refusal(entry, idx, rows, k, n, heads, group, "group", ptr_v, pos_v,
                                     alpha_out && alpha_drop_out && (node_score || edge_score || entry_score),
                                     "null alpha_out or alpha_drop_out, or node_score, edge_score and entry_score all null",
                                     {node_score, edge_score, entry_score, alpha_out, alpha_drop_out}, &drop))
    return st;
  HeadsSoftmaxArgs a = softmax_args(idx, rows, k, n, heads, node_score, edge_score, entry_score, slope, ptr_v, pos_v);
  a.out_entry = alpha_out;
  a.out_drop = alpha_drop_out;
  a.rng = rng_dev;
  a.T = drop_threshold(p_drop);
  a.scale = 1.0f / (1.0f - p_drop);
  return launch_softmax_heads<kBodySoftmax, true>(entry, group, a, stream);
}

int hg_table_softmax_dropout_bwd_heads_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t heads, int32_t group,
                                           const float *node_score, const float *edge_score, const float *entry_score,
                                           float slope, float p_drop, const uint64_t *rng_dev, const int32_t *ptr_v,
                                           const int32_t *pos_v, const float *alpha, const float *dout, float *ds, float *dgroup,
                                           hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_softmax_dropout_bwd_heads_f32";
  const DropCall drop{p_drop, rng_dev};
  if (const int st = softmax_refusal(entry, idx, rows, k, n, heads, group, "group", ptr_v, pos_v,
                                     alpha && dout && ds && (node_score || edge_score || entry_score),
                                     "null alpha, dout or ds, or node_score, edge_score and entry_score all null",
                                     {node_score, edge_score, entry_score, alpha, dout, ds, dgroup}, &drop))
    return st;
  HeadsSoftmaxArgs a = softmax_args(idx, rows, k, n, heads, node_score, edge_score, entry_score, slope, ptr_v, pos_v);
  a.val = alpha;
  a.dval = dout;
  a.out_entry = ds;
  a.out_seg = dgroup;
  a.rng = rng_dev;
  a.T = drop_threshold(p_drop);
  a.scale = 1.0f / (1.0f - p_drop);
  return launch_softmax_heads<kBodySoftmaxBwd, true>(entry, group, a, stream);
}

int hg_table_sum_heads_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t heads, int32_t side,
                           const int32_t *ptr_v, const int32_t *pos_v, const float *val, float *out, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_sum_heads_f32";
  if (const int st = softmax_refusal(entry, idx, rows, k, n, heads, side, "side", ptr_v, pos_v, val && out, "null val or out",
                                     {val, out}))
    return st;
  HeadsSoftmaxArgs a = softmax_args(idx, rows, k, n, heads, nullptr, nullptr, nullptr, 1.f, ptr_v, pos_v);
  a.val = val;
  a.out_seg = out;
  return launch_softmax_heads<kBodySum>(entry, side, a, stream);
}

int hg_table_attention_stats_heads_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t heads, int32_t group,
                                       const float *node_score, const float *edge_score, float slope, const int32_t *ptr_v,
                                       const int32_t *pos_v, float *seg_max, float *seg_inv, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_attention_stats_heads_f32";
  if (const int st = softmax_refusal(entry, idx, rows, k, n, heads, group, "group", ptr_v, pos_v,
                                     seg_max && seg_inv && (node_score || edge_score),
                                     "null seg_max or seg_inv, or node_score and edge_score both null",
                                     {node_score, edge_score, seg_max, seg_inv}))
    return st;
  HeadsSoftmaxArgs a = softmax_args(idx, rows, k, n, heads, node_score, edge_score, nullptr, slope, ptr_v, pos_v);
  a.out_seg = seg_max;
  a.out_inv = seg_inv;
  return launch_softmax_heads<kBodyStats>(entry, group, a, stream);
}

int hg_table_gather_heads_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, int32_t heads, const float *src,
                              const float *w, const float *src_scale, const float *dst_scale, float *dst, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_gather_heads_f32";
  if (!idx) return fail(entry, HG_ERR_INVALID, "null idx");
  if (const int st = gather_refusal(entry, rows, k, n, F, heads, src, w, src_scale, dst_scale, dst)) return st;
  if ((uintptr_t)idx % 4) return fail(entry, HG_ERR_UNSUPPORTED, "idx must be 4-byte aligned");
  return launch_gather_heads<false>(entry, idx, nullptr, nullptr, rows, k, n, F, heads, src, w, src_scale, dst_scale, dst, stream);
}

int hg_table_gather_t_heads_f32(const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k, int32_t n, int32_t F,
                                int32_t heads, const float *src, const float *w, const float *src_scale, const float *dst_scale,
                                float *dst, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_gather_t_heads_f32";
  if (!ptr_v || !pos_v) return fail(entry, HG_ERR_INVALID, "null ptr_v or pos_v");
  if (const int st = gather_refusal(entry, rows, k, n, F, heads, src, w, src_scale, dst_scale, dst)) return st;
  if ((uintptr_t)ptr_v % 4 || (uintptr_t)pos_v % 4) return fail(entry, HG_ERR_UNSUPPORTED, "ptr_v and pos_v must be 4-byte aligned");
  return launch_gather_heads<true>(entry, nullptr, ptr_v, pos_v, rows, k, n, F, heads, src, w, src_scale, dst_scale, dst, stream);
}

int hg_table_dot_heads_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, int32_t heads, const float *A,
                           const float *a_scale, const float *B, const float *C, const float *D, float *out,
                           hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_dot_heads_f32";
  if (!idx) return fail(entry, HG_ERR_INVALID, "null idx");
  if (!A || !B || !out) return fail(entry, HG_ERR_INVALID, "null A, B or out");
  if (!C != !D) return fail(entry, HG_ERR_INVALID, "C and D must both be given or both be null");
  if (const int st = size_refusal(entry, rows, k, n, F)) return st;
  if (const int st = heads_refusal(entry, heads)) return st;
  if (F % heads) return fail(entry, HG_ERR_INVALID, "F = " + std::to_string(F) + " is no multiple of heads = " + std::to_string(heads));
  for (const void *p : {(const void *)idx, (const void *)A, (const void *)a_scale, (const void *)B, (const void *)C,
                        (const void *)D, (const void *)out})
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, "idx, A, a_scale, B, C, D and out must be 4-byte aligned");
  HeadsDotArgs a{};
  a.idx = idx;
  a.A = A;
  a.a_scale = a_scale;
  a.B = B;
  a.C = C;
  a.D = D;
  a.out = out;
  a.rows = rows;
  a.n = n;
  a.k = k;
  a.F = F;
  a.H = heads;
  a.Ch = F / heads;
  const bool vec4 = a.Ch % 4 == 0 && aligned16({A, B, C, D});
  const int V = vec4 ? 4 : 1;
  a.L = 1;
  while (a.L < std::min((a.Ch + V - 1) / V, 64)) a.L <<= 1;  // DOT ORDER at width Ch
  a.R = 64 / a.L;
  const int RW = a.R * kTableWaves;
  const dim3 grid((unsigned)(((int64_t)rows * heads + RW - 1) / RW)), block(64 * kTableWaves);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec4 && C) hipLaunchKernelGGL((table_dot_heads_kernel<4, true>), grid, block, 0, s, a);
  else if (vec4) hipLaunchKernelGGL((table_dot_heads_kernel<4, false>), grid, block, 0, s, a);
  else if (C) hipLaunchKernelGGL((table_dot_heads_kernel<1, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((table_dot_heads_kernel<1, false>), grid, block, 0, s, a);
  return launch_check(entry);
}

}  // extern "C"
