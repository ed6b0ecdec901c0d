// Fused attention aggregation over a dense neighbour table idx [rows, k] (include/hg_aggr.h, hg_table_attention_gather_heads_f32
// and hg_table_attention_gather_t_heads_f32): the two weighted sum gathers of hg_table_heads.hip with the weight w[p, h] never
// read from memory.  A coefficient is formed where it is used, from the two score rows of its position and the two numbers per
// (segment, head) that hg_table_attention_stats_heads_f32 (hg_table_heads.hip, kBodyStats) wrote:
//     alpha(p, h) = __expf(leaky(own + other, slope) - seg_max[seg, h]) * seg_inv[seg, h]
// -- the softmax kernel's own expression on its own operands, so alpha has the bits hg_table_softmax_heads_f32 would have
// stored, and dst the bits of the heads gathers on that array.  Ownership, lanes, the kTableBatch row loads in flight, the
// ascending order, the long rows' pieces and LDS tree are table_gather_heads_kernel's, at the same F.
//
// The two sides of a gather: the DESTINATION row r (table row i in the hyperedge gather, vertex v in the transposed one) and
// the SOURCE row js of an entry (vertex j = idx[p], or table row i = p / k).  Scores and statistics are passed by side: rs
// [nrows, H] the destination side's score, es [nsrc, H] the source side's; the segment of a position is its destination
// row (seg_row: the hyperedge gather under the hyperedge group, the transposed one under the vertex group) or its source row.
// What belongs to the destination row -- its score and, under seg_row, m and inv -- is loaded once per (row, head), never
// per entry.
//
// Who forms a coefficient.  Ch / 4 lanes of a row share a head, and each forming its own coefficient repeats the source
// side's score loads, the leaky relu and the exponential Ch / 4 times per entry.  So where lanes share a head (16-byte lanes,
// Ch % 4 == 0, Ch >= kSlabMinCh = 16) the WAVE forms the coefficients of a batch once, in a slab of LDS of its own:
//   rc[3][R x HP]              the row constants (score, m, inv) of the wave's R rows and the HP heads of this column pass
//   cf[(r, u, hh)]             alpha of row r's entry u of the batch, head hlo + hh: R x kTableBatch x HP floats
// The wave's 64 lanes are spread over the items (r, u, hh) in that order, item e to lane e % 64: a lane reads its row's
// entry range by a shuffle, the entry's source row from idx / pos_v, the source side's score (and m, inv where the segment is
// the source row), and stores one float.  The gather loop then reads cf[(sub, u, c / Ch - hlo)]: one address for all the
// lanes of a head, a broadcast.  R x HP <= kSlabCap for every Ch >= 8: 256 / Ch <= 32 (row, head) pairs in a wave that holds
// whole rows, at most 255 / Ch + 2 <= 33 heads in one 256-column pass of a wider row.  A slab belongs to one wave, LDS
// operations of a wave complete in issue order, and a wave-scope fence keeps the compiler from moving them: no __syncthreads
// in the short-row path.  The batch loop runs to the longest short row of the wave, every lane in the coefficient phase, the
// row's lanes in the adds.
// Elsewhere -- 4-byte lanes, a lane that straddles heads, Ch < 16 (two lanes a head repay no slab), and the long rows of the
// transposed gather, whose pieces are cut per lane group -- a lane forms its own coefficients in registers.  The expression
// is the same: the bits do not depend on who evaluated it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "hg_aggr.h"
#include "hg_attention.h"
#include "hg_internal.h"
#include "hg_table.h"

namespace hg {
namespace {

#ifndef HG_TABLE_SLAB_MIN_CH
#define HG_TABLE_SLAB_MIN_CH 16  // measured (profiles/table_attention_fused.md): at Ch = 8 the slab loses; a huge value: no slab
#endif
constexpr int kSlabMinCh = HG_TABLE_SLAB_MIN_CH;
constexpr int kSlabCap = 34;   // (row, head) pairs of a wave in one column pass: see above

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

struct AttnGatherArgs {
  const int32_t *idx;            // the table [rows, k] (the hyperedge gather)
  const int32_t *ptr_v, *pos_v;  // its transpose (the vertex gather)
  const float *src, *src_scale, *dst_scale;
  const float *rs, *es;              // the scores of the destination side [nrows, H] and of the source side [nsrc, H]; one may be null
  const float *seg_max, *seg_inv;    // [segments, H]
  float *dst;
  float slope;
  int32_t nrows, nsrc;  // destination and source rows
  int32_t k, F, entries, H, Ch;
  int32_t L, R;         // lanes per row, rows per wave: the plain gathers' at this F
  int32_t P2;           // the power of two at or above kTableWaves R
  int32_t seg_row;      // the segment of a position is its destination row (else its source row)
};

// alpha(p, h) of an entry whose source row is js.  (s, m, inv): the destination row's score and, under seg_row, its statistics.
// raw is seg_raw's: the segment's own score first, an absent score no addition.
__device__ __forceinline__ float coefficient(const AttnGatherArgs &a, float s, float m, float inv, int js, int h) {
  const size_t e = (size_t)js * a.H + h;
  float raw;
  if (a.seg_row) {
    raw = a.rs ? s : 0.f;
    if (a.es) raw = a.rs ? raw + a.es[e] : a.es[e];
  } else {
    raw = a.es ? a.es[e] : 0.f;
    if (a.rs) raw = a.es ? raw + s : s;
    m = a.seg_max[e];
    inv = a.seg_inv[e];
  }
  return __expf(leaky(raw, a.slope) - m) * inv;
}

// Entry q of a destination row: its source row, 0 where the entry is no candidate
template <bool T>
__device__ __forceinline__ bool entry_source(const AttnGatherArgs &a, int q, bool on, int &js) {
  if (T) {
    const int p = a.pos_v[on ? q : 0];
    on = on && (unsigned)p < (unsigned)a.entries;
    js = on ? p / a.k : 0;
  } else {
    js = a.idx[on ? q : 0];
    on = on && (unsigned)js < (unsigned)a.nsrc;
    js = on ? js : 0;
  }
  return on;
}

// acc += the terms of the entries [b, min(b + kTableBatch, end)), ascending, for the columns c .. c + V - 1: one batch of
// heads_row_sum (hg_table_heads.hip).  weight(u, i, js): the coefficient of entry b + u for the lane's i-th head.  An entry
// that is no candidate has js = 0 -- nothing is read through its index -- and whatever weight returns for it is not added.
template <bool T, int V, int WN, typename WF>
__device__ __forceinline__ void batch_sum(const AttnGatherArgs &a, int b, int end, int c, float (&acc)[V], WF weight) {
  Vec<V> x[kTableBatch];
  float wv[kTableBatch][WN], sv[kTableBatch];
  bool ok[kTableBatch];
#pragma unroll
  for (int u = 0; u < kTableBatch; ++u) {
    int js;
    ok[u] = entry_source<T>(a, b + u, b + u < end, js);
#pragma unroll
    for (int i = 0; i < WN; ++i) wv[u][i] = weight(u, i, js);
    sv[u] = a.src_scale ? a.src_scale[js] : 1.f;
    x[u] = vec_load<V>(a.src + (size_t)js * a.F + c);
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

// acc += the entries [beg, end) of destination row `row`, every lane forming its own coefficients: the row's constants for
// the lane's WN heads once, then batch after batch.
template <bool T, int V, int WN>
__device__ __forceinline__ void lane_row_sum(const AttnGatherArgs &a, int row, int beg, int end, int c, float (&acc)[V]) {
  int hd[WN];
  float s[WN], m[WN], inv[WN];
#pragma unroll
  for (int i = 0; i < WN; ++i) {
    hd[i] = (c + i) / a.Ch;
    const size_t e = (size_t)row * a.H + hd[i];
    s[i] = a.rs ? a.rs[e] : 0.f;
    m[i] = a.seg_row ? a.seg_max[e] : 0.f;
    inv[i] = a.seg_row ? a.seg_inv[e] : 0.f;
  }
  for (int b = beg; b < end; b += kTableBatch)
    batch_sum<T, V, WN>(a, b, end, c, acc, [&](int, int i, int js) { return coefficient(a, s[i], m[i], inv[i], js, hd[i]); });
}

// LDS operations of one wave complete in the order they were issued; this keeps the compiler to that order as well
__device__ __forceinline__ void wave_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool T, int V, int WN, bool SLAB>
__global__ __launch_bounds__(64 * kTableWaves) void table_attention_gather_kernel(AttnGatherArgs a) {
  static_assert(!SLAB || (V == 4 && WN == 1), "the slab serves 16-byte lanes whose columns share a head");
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
  const bool short_on = row_on && !is_long;
  const float ds = short_on && a.dst_scale ? a.dst_scale[row] : 1.f;

  if constexpr (SLAB) {
    __shared__ float rc[kTableWaves][3][kSlabCap];
    __shared__ float cf[kTableWaves][kTableBatch * kSlabCap];
    const int send = short_on ? end : beg;  // a long row and an absent one take no part here
    const int H = a.H, Ch = a.Ch;
    for (int c0 = 0; c0 < F; c0 += L * V) {  // with F > 64 V the heads of a lane change between the passes
      const int c = c0 + cl * V;
      const bool col_on = short_on && c < F;
      const int hlo = c0 / Ch, HP = (min(c0 + L * V, F) - 1) / Ch - hlo + 1;
      for (int e = lane; e < R * HP; e += 64) {  // the rows' constants, once per (row, head)
        const int r = e / HP, hh = e - r * HP;
        const int64_t rr = row0 + w * R + r;
        const size_t at = (size_t)(rr < a.nrows ? rr : 0) * H + hlo + hh;
        rc[w][0][e] = a.rs ? a.rs[at] : 0.f;
        rc[w][1][e] = a.seg_row ? a.seg_max[at] : 0.f;
        rc[w][2][e] = a.seg_row ? a.seg_inv[at] : 0.f;
      }
      wave_order();
      float acc[V];
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] = 0.f;
      const int items = R * kTableBatch * HP;
      for (int b = 0; __any(beg + b < send); b += kTableBatch) {
        for (int e0 = 0; e0 < items; e0 += 64) {  // the batch's coefficients, one item a lane; every lane shuffles
          const int e = e0 + lane;
          const bool on = e < items;
          const int ru = (on ? e : 0) / HP, hh = (on ? e : 0) - ru * HP;
          const int r = ru / kTableBatch, u = ru % kTableBatch;
          const int q = __shfl(beg, r * L, 64) + b + u, qe = __shfl(send, r * L, 64);
          int js;
          if (entry_source<T>(a, q, on && q < qe, js))
            cf[w][e] = coefficient(a, rc[w][0][r * HP + hh], rc[w][1][r * HP + hh], rc[w][2][r * HP + hh], js, hlo + hh);
        }
        wave_order();
        if (col_on && beg + b < send) {
          const float *mine = &cf[w][(size_t)sub * kTableBatch * HP + (c / Ch - hlo)];
          batch_sum<T, V, 1>(a, beg + b, send, c, acc, [&](int u, int, int) { return mine[u * HP]; });
        }
        wave_order();  // the next batch's stores stay behind these loads
      }
      if (col_on) {
        if (a.dst_scale && end > beg) {  // an empty row stays +0.0 whatever its scale
#pragma unroll
          for (int i = 0; i < V; ++i) acc[i] = ds * acc[i];
        }
        vec_store<V>(a.dst + (size_t)row * F + c, acc);
      }
      wave_order();  // the next pass's row constants likewise
    }
  } else {
    if (short_on) {
      for (int c0 = 0; c0 < F; c0 += L * V) {
        const int c = c0 + cl * V;
        if (c >= F) continue;
        float acc[V];
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = 0.f;
        lane_row_sum<T, V, WN>(a, row, beg, end, c, acc);
        if (a.dst_scale && end > beg) {
#pragma unroll
          for (int i = 0; i < V; ++i) acc[i] = ds * acc[i];
        }
        vec_store<V>(a.dst + (size_t)row * F + c, acc);
      }
    }
  }

  if constexpr (T) {
    // the tile's long rows, one after the other, by the whole workgroup: the plain gather's pieces and tree, per-lane coefficients
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
        const float lds = a.dst_scale ? a.dst_scale[lrow] : 1.f;
        for (int c0 = 0; c0 < F; c0 += L * V) {
          const int c = c0 + cl * V;
          const bool on = lane_on && c < F;
          float *mypart = part + (size_t)(g * L + cl) * V;
          if (on) {
            float acc[V];
#pragma unroll
            for (int i = 0; i < V; ++i) acc[i] = 0.f;
            lane_row_sum<T, V, WN>(a, lrow, gb, ge, c, acc);
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
            for (int i = 0; i < V; ++i) out[i] = a.dst_scale ? lds * mypart[i] : mypart[i];
            vec_store<V>(a.dst + (size_t)lrow * F + c, out);
          }
          __syncthreads();
        }
      }
    }
  }
}

// what the two gathers refuse, in the heads gathers' order (no w here), then what the coefficients add
int attention_gather_refusal(const char *entry, int32_t rows, int32_t k, int32_t n, int32_t F, int32_t heads,
                             const float *src, const float *node, const float *edge, const float *seg_max, const float *seg_inv,
                             const float *src_scale, const float *dst_scale, const float *dst) {
  if (!src || !dst) return fail(entry, HG_ERR_INVALID, "null src or dst");
  if (const int st = size_refusal(entry, rows, k, n, F)) return st;
  if (heads < 1) return fail(entry, HG_ERR_INVALID, "heads must be at least 1, got " + std::to_string(heads));
  if (F % heads) return fail(entry, HG_ERR_INVALID, "F = " + std::to_string(F) + " is no multiple of heads = " + std::to_string(heads));
  for (const void *p : {(const void *)src, (const void *)node, (const void *)edge, (const void *)seg_max, (const void *)seg_inv,
                        (const void *)src_scale, (const void *)dst_scale, (const void *)dst})
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, "src, the scores, seg_max, seg_inv, the scales and dst must be 4-byte aligned");
  return HG_OK;
}

int coefficient_refusal(const char *entry, int32_t group, const float *node, const float *edge, const float *seg_max,
                        const float *seg_inv) {
  if (!seg_max || !seg_inv) return fail(entry, HG_ERR_INVALID, "null seg_max or seg_inv (hg_table_attention_stats_heads_f32 writes them)");
  if (!node && !edge) return fail(entry, HG_ERR_INVALID, "node_score and edge_score both null");
  if (group != HG_TABLE_HYPEREDGE && group != HG_TABLE_VERTEX)
    return fail(entry, HG_ERR_INVALID, "group must be HG_TABLE_HYPEREDGE or HG_TABLE_VERTEX, got " + std::to_string(group));
  return HG_OK;
}

template <bool T>
int launch_attention_gather(const char *entry, const int32_t *idx, const int32_t *ptr_v, const int32_t *pos_v, int32_t rows,
                            int32_t k, int32_t n, int32_t F, int32_t heads, int32_t group, const float *src, const float *node,
                            const float *edge, float slope, const float *seg_max, const float *seg_inv, const float *src_scale,
                            const float *dst_scale, float *dst, hg_stream_t stream) {
  AttnGatherArgs a{};
  a.idx = idx;
  a.ptr_v = ptr_v;
  a.pos_v = pos_v;
  a.src = src;
  a.src_scale = src_scale;
  a.dst_scale = dst_scale;
  a.rs = T ? node : edge;
  a.es = T ? edge : node;
  a.seg_max = seg_max;
  a.seg_inv = seg_inv;
  a.dst = dst;
  a.slope = slope;
  a.nrows = T ? n : rows;
  a.nsrc = T ? rows : n;
  a.k = k;
  a.F = F;
  a.H = heads;
  a.Ch = F / heads;
  a.entries = rows * k;
  a.seg_row = T == (group == HG_TABLE_VERTEX);
  // the geometry is the plain gathers' at this F: the long rows' pieces and tree follow from it
  const bool vec4 = F % 4 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
  const int V = vec4 ? 4 : 1;
  a.L = std::min((F + V - 1) / V, 64);
  a.R = 64 / a.L;
  a.P2 = 1;
  while (a.P2 < a.R * kTableWaves) a.P2 <<= 1;
  const int RW = a.R * kTableWaves;
  const int pass_heads = F <= 64 * V ? heads : std::min<int>(heads, 255 / a.Ch + 2);  // the most heads one column pass touches
  const bool slab = vec4 && a.Ch % 4 == 0 && a.Ch >= kSlabMinCh && a.R * pass_heads <= kSlabCap;
  const dim3 grid((unsigned)(((int64_t)a.nrows + RW - 1) / RW)), block(64 * kTableWaves);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (slab) hipLaunchKernelGGL((table_attention_gather_kernel<T, 4, 1, true>), grid, block, 0, s, a);
  else if (vec4 && a.Ch % 4 == 0) hipLaunchKernelGGL((table_attention_gather_kernel<T, 4, 1, false>), grid, block, 0, s, a);
  else if (vec4) hipLaunchKernelGGL((table_attention_gather_kernel<T, 4, 4, false>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((table_attention_gather_kernel<T, 1, 1, false>), grid, block, 0, s, a);
  return launch_check(entry);
}

}  // namespace
}  // namespace hg

extern "C" {

int hg_table_attention_gather_heads_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, int32_t heads,
                                        int32_t group, const float *src, const float *node_score, const float *edge_score,
                                        float slope, const float *seg_max, const float *seg_inv, const float *src_scale,
                                        const float *dst_scale, float *dst, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_attention_gather_heads_f32";
  if (!idx) return fail(entry, HG_ERR_INVALID, "null idx");
  if (const int st = attention_gather_refusal(entry, rows, k, n, F, heads, src, node_score, edge_score, seg_max, seg_inv,
                                              src_scale, dst_scale, dst))
    return st;
  if ((uintptr_t)idx % 4) return fail(entry, HG_ERR_UNSUPPORTED, "idx must be 4-byte aligned");
  if (const int st = coefficient_refusal(entry, group, node_score, edge_score, seg_max, seg_inv)) return st;
  return launch_attention_gather<false>(entry, idx, nullptr, nullptr, rows, k, n, F, heads, group, src, node_score, edge_score,
                                        slope, seg_max, seg_inv, src_scale, dst_scale, dst, stream);
}

int hg_table_attention_gather_t_heads_f32(const int32_t *ptr_v, const int32_t *pos_v, const int32_t *idx, int32_t rows, int32_t k,
                                          int32_t n, int32_t F, int32_t heads, int32_t group, const float *src,
                                          const float *node_score, const float *edge_score, float slope, const float *seg_max,
                                          const float *seg_inv, const float *src_scale, const float *dst_scale, float *dst,
                                          hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_attention_gather_t_heads_f32";
  if (!ptr_v || !pos_v || !idx) return fail(entry, HG_ERR_INVALID, "null ptr_v, pos_v or idx");
  if (const int st = attention_gather_refusal(entry, rows, k, n, F, heads, src, node_score, edge_score, seg_max, seg_inv,
                                              src_scale, dst_scale, dst))
    return st;
  if ((uintptr_t)ptr_v % 4 || (uintptr_t)pos_v % 4 || (uintptr_t)idx % 4)
    return fail(entry, HG_ERR_UNSUPPORTED, "ptr_v, pos_v and idx must be 4-byte aligned");
  if (const int st = coefficient_refusal(entry, group, node_score, edge_score, seg_max, seg_inv)) return st;
  return launch_attention_gather<true>(entry, idx, ptr_v, pos_v, rows, k, n, F, heads, group, src, node_score, edge_score, slope,
                                       seg_max, seg_inv, src_scale, dst_scale, dst, stream);
}

}  // extern "C"
