// Dot-product attention over a dense neighbour table idx [rows, k] under the hyperedge group (include/hg_aggr.h,
// hg_table_dot_attention_f32, hg_table_dot_attention_bwd_f32 and hop 1, hg_table_dot_attention_gather_t_f32, further down): the softmax segment is the table row itself, k <= 64
// entries, so one lane group forms a row's logits, its softmax and its weighted sum in one walk -- the flash-attention shape
// on a table.  A member row X[j] is loaded ONCE and used from registers twice: for the logit <query[i], X[j]> and for the sum.
//
// Units.  The unit of work is one (row i, head h): unit u = i H + h.  A group of Gp lanes owns a unit, Gp the power of two at
// or above min(ceil(Ch / c), 64): 64 / Gp units a wave, kTableWaves waves a workgroup, unit u at thread u Gp of the grid.
// Heads are independent: a row wider than a wave is more units, and no state is carried between column passes.
//   c = 4 (Ch % 4 == 0 and 16-byte aligned row arrays): lane g owns the columns 4 g .. 4 g + 3 of its head, one 16-byte access a
//     row.  Ch <= 64 * 4 = 256; lanes with 4 g >= Ch (a padded group, Ch = 80: 20 of 32) load nothing and add +0.0.
//   c = 1: lane g owns the columns g, g + Gp, g + 2 Gp, g + 3 Gp below Ch -- up to four 4-byte accesses, coalesced across the
//     group -- so Ch <= 256 here too.  One slot a lane (<1, false>) where Ch <= 64.
//
// Forward, one walk in ascending s, kTableBatch entries at a time: the batch's indices, then that many row chunks in flight,
// then per entry the lane's fma chain over its columns (ascending), the xor butterfly Gp / 2 .. 1 that leaves the logit in
// every lane, and the online update
//     m' = max(m, a),  corr = __expf(m - m'),  e = __expf(a - m'),  l = l corr + e,  acc = acc corr + e x
// on the chunk already in registers.  The first candidate sets (m, l, acc) = (a, 1, x) outright, so there is no inf - inf, and
// a unit with no candidate stores +0.0.  alpha, where wanted, comes from the same launch: lane s % Gp stores the entry's a at
// alpha[i, s, h] during the walk, and after it reads its own stores back and writes __expf(a - m) (1 / l) over them -- a
// thread reading its own global stores needs no fence -- and +0.0 where the entry is no candidate.
//
// Backward, the same units, g = dst_scale[i] ddst[i, head h] and the query chunk in registers, TWO walks: the first forms
// dalpha(s) = <g, X[j]> + dalpha_ext and D = sum_s alpha dalpha, the second forms dalpha(s) and t(s) again -- the same chains
// and the same two-value butterfly, so the same bits; its loads hit the L2 -- and from them ds and dquery += ds X[j].  Keeping
// the row's dalpha in registers instead would spread k <= 64 values over Gp lanes, 64 registers a lane at Gp = 1 under a
// dynamic index: scratch.  Two walks keep every instance scratch-free at a third of the register budget.
//
// No LDS, no __syncthreads, no atomics, no workspace.  Every lane of a wave runs every shuffle: a unit past the end and a
// padding lane are masked in their loads and stores, never in control flow.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "hg_aggr.h"
#include "hg_attention.h"
#include "hg_internal.h"
#include "hg_table.h"

namespace hg {
namespace {

constexpr int kDotAttnMaxCh = 256;  // 64 lanes x 4 columns

struct DotAttnArgs {
  const int32_t *idx;
  const int32_t *ptr_v, *pos_v;               // hop 1: the table's transpose
  const float *w, *src_scale, *src2, *w2;     // hop 1: the weights [rows k, H], the source rows' scale, the optional second pair
  const float *query, *src, *dst_scale;
  const float *alpha_in, *ddst, *dalpha_ext;  // backward
  float *dst, *alpha;                         // forward; alpha may be null
  float *dquery, *ds;                         // backward
  float scale, slope;
  int32_t rows, k, n, F, H, Ch;
  int32_t Gp, shift;  // lanes a unit and log2 of it
  int32_t entries;    // hop 1: rows k
  int64_t units;      // (rows or n) H
};

// The lane's V columns of head h, as offsets into a row of F columns; on[i]: the column exists
template <int V, bool VEC>
__device__ __forceinline__ void lane_columns(const DotAttnArgs &a, int h, int g, int (&col)[V], bool (&on)[V]) {
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const int c = VEC ? 4 * g + i : g + i * a.Gp;
    on[i] = c < a.Ch;
    col[i] = h * a.Ch + (on[i] ? c : 0);
  }
}

// x = the lane's columns of row `r` of p (+0.0 where the column does not exist or `live` is false: nothing is read then)
template <int V, bool VEC>
__device__ __forceinline__ void chunk_load(const float *p, size_t r, int F, const int (&col)[V], const bool (&on)[V], bool live,
                                           float (&x)[V]) {
  if constexpr (VEC) {
    float4 v = float4{0.f, 0.f, 0.f, 0.f};
    if (live && on[0]) v = *reinterpret_cast<const float4 *>(p + r * F + col[0]);
    x[0] = v.x;
    x[1] = v.y;
    x[2] = v.z;
    x[3] = v.w;
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) x[i] = live && on[i] ? p[r * F + col[i]] : 0.f;
  }
}

template <int V, bool VEC>
__device__ __forceinline__ void chunk_store(float *p, size_t r, int F, const int (&col)[V], const bool (&on)[V], bool live,
                                            const float (&x)[V]) {
  if constexpr (VEC) {
    if (live && on[0]) *reinterpret_cast<float4 *>(p + r * F + col[0]) = float4{x[0], x[1], x[2], x[3]};
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i)
      if (live && on[i]) p[r * F + col[i]] = x[i];
  }
}

// the lane's fma chain over its columns, ascending, from +0.0
template <int V>
__device__ __forceinline__ float chain(const float (&q)[V], const float (&x)[V]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < V; ++i) s = fmaf(q[i], x[i], s);
  return s;
}

// t = t + t[lane xor o], o = Gp / 2 .. 1: every lane of the group ends with the same bits (the add commutes)
__device__ __forceinline__ float group_sum(float t, int Gp) {
  for (int o = Gp >> 1; o >= 1; o >>= 1) t = t + __shfl_xor(t, o, 64);
  return t;
}

// One batch of the walk: the entries s0 .. s0 + kTableBatch - 1 of unit row i.  ok[u]: entry u is a candidate; x[u] its chunk.
template <int V, bool VEC>
__device__ __forceinline__ void batch_load(const DotAttnArgs &a, bool unit_on, size_t i, int s0, const int (&col)[V],
                                           const bool (&on)[V], bool (&ok)[kTableBatch], float (&x)[kTableBatch][V]) {
  int j[kTableBatch];
#pragma unroll
  for (int u = 0; u < kTableBatch; ++u) {
    const bool in = unit_on && s0 + u < a.k;
    j[u] = in ? a.idx[i * a.k + s0 + u] : -1;
  }
#pragma unroll
  for (int u = 0; u < kTableBatch; ++u) {
    ok[u] = (unsigned)j[u] < (unsigned)a.n;
    chunk_load<V, VEC>(a.src, (size_t)(ok[u] ? j[u] : 0), a.F, col, on, ok[u], x[u]);
  }
}

template <int V, bool VEC>
__global__ __launch_bounds__(64 * kTableWaves) void table_dot_attention_kernel(DotAttnArgs a) {
  const int64_t t64 = (int64_t)blockIdx.x * (64 * kTableWaves) + threadIdx.x;
  const int64_t unit = t64 >> a.shift;
  const int g = (int)(t64 & (a.Gp - 1));
  const bool unit_on = unit < a.units;
  const size_t i = unit_on ? (size_t)(unit / a.H) : 0;
  const int h = unit_on ? (int)(unit - (int64_t)i * a.H) : 0;
  int col[V];
  bool on[V];
  lane_columns<V, VEC>(a, h, g, col, on);
  float q[V];
  chunk_load<V, VEC>(a.query, i, a.F, col, on, unit_on, q);
  float *arow = a.alpha ? a.alpha + (i * a.k) * a.H + h : nullptr;  // alpha[i, s, h] = arow[s H]

  float m = 0.f, l = 0.f, acc[V];
  bool have = false;
#pragma unroll
  for (int c = 0; c < V; ++c) acc[c] = 0.f;
  for (int s0 = 0; s0 < a.k; s0 += kTableBatch) {
    bool ok[kTableBatch];
    float x[kTableBatch][V];
    batch_load<V, VEC>(a, unit_on, i, s0, col, on, ok, x);
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u) {
      const float t = a.scale * group_sum(chain<V>(q, x[u]), a.Gp);
      const float v = leaky(t, a.slope);
      if (ok[u]) {  // uniform over the unit; no shuffle inside
        if (arow && ((s0 + u) & (a.Gp - 1)) == g) arow[(size_t)(s0 + u) * a.H] = v;
        const float mn = have ? fmaxf(m, v) : v;
        const float corr = have ? __expf(m - mn) : 0.f;
        const float e = __expf(v - mn);
        l = l * corr + e;
#pragma unroll
        for (int c = 0; c < V; ++c) acc[c] = acc[c] * corr + e * x[u][c];
        m = mn;
        have = true;
      }
    }
  }
  const float inv = have ? 1.f / l : 0.f;
  const float dsc = unit_on && a.dst_scale ? a.dst_scale[i] : 1.f;
  float out[V];
#pragma unroll
  for (int c = 0; c < V; ++c) out[c] = have ? dsc * (acc[c] * inv) : 0.f;
  chunk_store<V, VEC>(a.dst, i, a.F, col, on, unit_on, out);
  if (arow && unit_on) {
    for (int s = g; s < a.k; s += a.Gp) {  // the lane's own stores, read back
      const bool cand = (unsigned)a.idx[i * a.k + s] < (unsigned)a.n;
      arow[(size_t)s * a.H] = cand ? __expf(arow[(size_t)s * a.H] - m) * inv : 0.f;
    }
  }
}

template <int V, bool VEC>
__global__ __launch_bounds__(64 * kTableWaves) void table_dot_attention_bwd_kernel(DotAttnArgs a) {
  const int64_t t64 = (int64_t)blockIdx.x * (64 * kTableWaves) + threadIdx.x;
  const int64_t unit = t64 >> a.shift;
  const int g = (int)(t64 & (a.Gp - 1));
  const bool unit_on = unit < a.units;
  const size_t i = unit_on ? (size_t)(unit / a.H) : 0;
  const int h = unit_on ? (int)(unit - (int64_t)i * a.H) : 0;
  int col[V];
  bool on[V];
  lane_columns<V, VEC>(a, h, g, col, on);
  const bool signs = a.slope != 1.f;  // at slope 1 the leaky factor is 1 whatever t: the second chain is skipped
  float q[V], gr[V];
  chunk_load<V, VEC>(a.query, i, a.F, col, on, unit_on, q);
  chunk_load<V, VEC>(a.ddst, i, a.F, col, on, unit_on, gr);
  const float dsc = unit_on && a.dst_scale ? a.dst_scale[i] : 1.f;
  if (a.dst_scale) {
#pragma unroll
    for (int c = 0; c < V; ++c) gr[c] = dsc * gr[c];
  }
  const size_t p0 = (i * a.k) * a.H + h;  // [i, s, h] = p0 + s H

  float D = 0.f;
  for (int s0 = 0; s0 < a.k; s0 += kTableBatch) {
    bool ok[kTableBatch];
    float x[kTableBatch][V];
    batch_load<V, VEC>(a, unit_on, i, s0, col, on, ok, x);
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u) {
      const float gx = group_sum(chain<V>(gr, x[u]), a.Gp);
      if (ok[u]) {
        const size_t p = p0 + (size_t)(s0 + u) * a.H;
        const float dal = a.dalpha_ext ? gx + a.dalpha_ext[p] : gx;
        D = D + a.alpha_in[p] * dal;
      }
    }
  }

  float dq[V];
#pragma unroll
  for (int c = 0; c < V; ++c) dq[c] = 0.f;
  for (int s0 = 0; s0 < a.k; s0 += kTableBatch) {
    bool ok[kTableBatch];
    float x[kTableBatch][V];
    batch_load<V, VEC>(a, unit_on, i, s0, col, on, ok, x);
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u) {
      float gx = chain<V>(gr, x[u]), t = signs ? chain<V>(q, x[u]) : 0.f;
      for (int o = a.Gp >> 1; o >= 1; o >>= 1) {  // the two-value butterfly
        gx = gx + __shfl_xor(gx, o, 64);
        if (signs) t = t + __shfl_xor(t, o, 64);
      }
      const bool in = unit_on && s0 + u < a.k;
      const size_t p = p0 + (size_t)(in ? s0 + u : 0) * a.H;
      float d = 0.f;
      if (ok[u]) {
        const float dal = a.dalpha_ext ? gx + a.dalpha_ext[p] : gx;
        const float sign = signs && !(a.scale * t > 0.f) ? a.slope : 1.f;
        d = a.alpha_in[p] * (dal - D) * sign * a.scale;
#pragma unroll
        for (int c = 0; c < V; ++c) dq[c] = dq[c] + d * x[u][c];
      }
      if (in && ((s0 + u) & (a.Gp - 1)) == g) a.ds[p] = d;
    }
  }
  chunk_store<V, VEC>(a.dquery, i, a.F, col, on, unit_on, dq);
}

// Hop 1 (hg_table_dot_attention_gather_t_f32): the unit is one (vertex v, head h), the same lane groups, and the unit sums its
// vertex row ptr_v[v] .. ptr_v[v + 1] - 1 in ascending q whatever its length, kTableBatch row chunks in flight.  So the order of
// a head's sum is a function of the vertex row alone -- not of F, heads or the launch -- and head h of Y is the single-head
// call's, hub vertices included, which hg_table_gather_t_heads_f32 (long rows cut by the call's F) does not give.  TWO: a
// second source and weight per entry, added after the first: the backward's value path and key path of dX in one launch.
template <int V, bool VEC, bool TWO>
__global__ __launch_bounds__(64 * kTableWaves) void table_dot_attention_gather_t_kernel(DotAttnArgs a) {
  const int64_t t64 = (int64_t)blockIdx.x * (64 * kTableWaves) + threadIdx.x;
  const int64_t unit = t64 >> a.shift;
  const int g = (int)(t64 & (a.Gp - 1));
  if (unit >= a.units) return;  // no shuffle in this kernel
  const size_t v = (size_t)(unit / a.H);
  const int h = (int)(unit - (int64_t)v * a.H);
  int col[V];
  bool on[V];
  lane_columns<V, VEC>(a, h, g, col, on);
  const int beg = max(a.ptr_v[v], 0), end = min(a.ptr_v[v + 1], a.entries);
  float acc[V];
#pragma unroll
  for (int c = 0; c < V; ++c) acc[c] = 0.f;
  for (int b = beg; b < end; b += kTableBatch) {
    bool ok[kTableBatch];
    float x[kTableBatch][V], x2[kTableBatch][TWO ? V : 1], wv[kTableBatch], w2v[kTableBatch], sv[kTableBatch];
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u) {
      const int p = b + u < end ? a.pos_v[b + u] : -1;
      ok[u] = (unsigned)p < (unsigned)a.entries;
      const size_t i = ok[u] ? (size_t)(p / a.k) : 0;
      const size_t at = (size_t)(ok[u] ? p : 0) * a.H + h;
      wv[u] = a.w[at];
      sv[u] = a.src_scale ? a.src_scale[i] : 1.f;
      chunk_load<V, VEC>(a.src, i, a.F, col, on, ok[u], x[u]);
      if constexpr (TWO) {
        w2v[u] = a.w2[at];
        chunk_load<V, VEC>(a.src2, i, a.F, col, on, ok[u], x2[u]);
      } else {
        w2v[u] = 0.f;
        x2[u][0] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u)
      if (ok[u]) {
#pragma unroll
        for (int c = 0; c < V; ++c) {
          float term = x[u][c];
          if (a.src_scale) term = term * sv[u];
          acc[c] = acc[c] + term * wv[u];
          if constexpr (TWO) acc[c] = acc[c] + x2[u][c] * w2v[u];
        }
      }
  }
  if (a.dst_scale && end > beg) {  // an empty row stays +0.0 whatever its scale
    const float dsc = a.dst_scale[v];
#pragma unroll
    for (int c = 0; c < V; ++c) acc[c] = dsc * acc[c];
  }
  chunk_store<V, VEC>(a.dst, v, a.F, col, on, true, acc);
}

bool misaligned(std::initializer_list<const void *> ps, unsigned to) {
  for (const void *p : ps)
    if ((uintptr_t)p % to) return true;
  return false;
}

// what both entries refuse after their own null pointers, in include/hg_aggr.h's order
int dot_attention_refusal(const char *entry, int32_t rows, int32_t k, int32_t n, int32_t F, int32_t heads) {
  if (const int st = size_refusal(entry, rows, k, n, F)) return st;
  if (heads < 1) return fail(entry, HG_ERR_INVALID, "heads must be at least 1, got " + std::to_string(heads));
  if (F % heads) return fail(entry, HG_ERR_INVALID, "F = " + std::to_string(F) + " is no multiple of heads = " + std::to_string(heads));
  if (F / heads > kDotAttnMaxCh)
    return fail(entry, HG_ERR_UNSUPPORTED, "Ch = F / heads = " + std::to_string(F / heads) + " is above 256 (one lane group holds a head's columns)");
  return HG_OK;
}

// the geometry of a call: c = 4 where vec4, Gp and the grid
template <typename K4, typename K1, typename K1x4>
int launch_dot_attention(const char *entry, DotAttnArgs &a, int64_t unit_rows, bool vec4, K4 k4, K1 k1, K1x4 k1x4,
                         hg_stream_t stream) {
  const int lanes = std::min(vec4 ? a.Ch / 4 : a.Ch, 64);
  a.Gp = 1;
  a.shift = 0;
  while (a.Gp < lanes) {
    a.Gp <<= 1;
    ++a.shift;
  }
  a.units = unit_rows * a.H;
  const int64_t threads = a.units * a.Gp, per = 64 * kTableWaves;
  const int64_t blocks = (threads + per - 1) / per;
  if (blocks > INT32_MAX) return fail(entry, HG_ERR_UNSUPPORTED, "rows * heads * lanes exceeds the grid");
  const dim3 grid((unsigned)blocks), block(64 * kTableWaves);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec4) hipLaunchKernelGGL(k4, grid, block, 0, s, a);
  else if (a.Ch <= 64) hipLaunchKernelGGL(k1, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k1x4, grid, block, 0, s, a);
  return launch_check(entry);
}

}  // namespace
}  // namespace hg

extern "C" {

int hg_table_dot_attention_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, int32_t heads,
                               const float *query, const float *src, float scale, float slope, const float *dst_scale,
                               float *dst, float *alpha, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_dot_attention_f32";
  if (!idx) return fail(entry, HG_ERR_INVALID, "null idx");
  if (!query || !src || !dst) return fail(entry, HG_ERR_INVALID, "null query, src or dst");
  if (const int st = dot_attention_refusal(entry, rows, k, n, F, heads)) return st;
  if (misaligned({idx, query, src, dst_scale, dst, alpha}, 4))
    return fail(entry, HG_ERR_UNSUPPORTED, "idx, query, src, dst_scale, dst and alpha must be 4-byte aligned");
  DotAttnArgs a{};
  a.idx = idx;
  a.query = query;
  a.src = src;
  a.dst_scale = dst_scale;
  a.dst = dst;
  a.alpha = alpha;
  a.scale = scale;
  a.slope = slope;
  a.rows = rows;
  a.k = k;
  a.n = n;
  a.F = F;
  a.H = heads;
  a.Ch = F / heads;
  const bool vec4 = a.Ch % 4 == 0 && !misaligned({query, src, dst}, 16);
  return launch_dot_attention(entry, a, rows, vec4, table_dot_attention_kernel<4, true>, table_dot_attention_kernel<1, false>,
                              table_dot_attention_kernel<4, false>, stream);
}

int hg_table_dot_attention_bwd_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, int32_t heads,
                                   const float *query, const float *src, float scale, float slope, const float *dst_scale,
                                   const float *alpha, const float *ddst, const float *dalpha_ext, float *dquery, float *ds,
                                   hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_dot_attention_bwd_f32";
  if (!idx) return fail(entry, HG_ERR_INVALID, "null idx");
  if (!query || !src || !alpha || !ddst || !dquery || !ds)
    return fail(entry, HG_ERR_INVALID, "null query, src, alpha, ddst, dquery or ds");
  if (const int st = dot_attention_refusal(entry, rows, k, n, F, heads)) return st;
  if (misaligned({idx, query, src, dst_scale, alpha, ddst, dalpha_ext, dquery, ds}, 4))
    return fail(entry, HG_ERR_UNSUPPORTED, "idx, query, src, dst_scale, alpha, ddst, dalpha_ext, dquery and ds must be 4-byte aligned");
  DotAttnArgs a{};
  a.idx = idx;
  a.query = query;
  a.src = src;
  a.dst_scale = dst_scale;
  a.alpha_in = alpha;
  a.ddst = ddst;
  a.dalpha_ext = dalpha_ext;
  a.dquery = dquery;
  a.ds = ds;
  a.scale = scale;
  a.slope = slope;
  a.rows = rows;
  a.k = k;
  a.n = n;
  a.F = F;
  a.H = heads;
  a.Ch = F / heads;
  const bool vec4 = a.Ch % 4 == 0 && !misaligned({query, src, ddst, dquery}, 16);
  return launch_dot_attention(entry, a, rows, vec4, table_dot_attention_bwd_kernel<4, true>, table_dot_attention_bwd_kernel<1, false>,
                              table_dot_attention_bwd_kernel<4, false>, stream);
}

int hg_table_dot_attention_gather_t_f32(const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k, int32_t n, int32_t F,
                                        int32_t heads, const float *src, const float *w, const float *src_scale,
                                        const float *src2, const float *w2, const float *dst_scale, float *dst,
                                        hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_dot_attention_gather_t_f32";
  if (!ptr_v || !pos_v) return fail(entry, HG_ERR_INVALID, "null ptr_v or pos_v");
  if (!src || !w || !dst) return fail(entry, HG_ERR_INVALID, "null src, w or dst");
  if (!src2 != !w2) return fail(entry, HG_ERR_INVALID, "src2 and w2 must both be given or both be null");
  if (const int st = dot_attention_refusal(entry, rows, k, n, F, heads)) return st;
  if (misaligned({ptr_v, pos_v, src, w, src_scale, src2, w2, dst_scale, dst}, 4))
    return fail(entry, HG_ERR_UNSUPPORTED, "ptr_v, pos_v, src, w, src_scale, src2, w2, dst_scale and dst must be 4-byte aligned");
  DotAttnArgs a{};
  a.ptr_v = ptr_v;
  a.pos_v = pos_v;
  a.src = src;
  a.w = w;
  a.src_scale = src_scale;
  a.src2 = src2;
  a.w2 = w2;
  a.dst_scale = dst_scale;
  a.dst = dst;
  a.rows = rows;
  a.k = k;
  a.n = n;
  a.F = F;
  a.H = heads;
  a.Ch = F / heads;
  a.entries = rows * k;
  const bool vec4 = a.Ch % 4 == 0 && !misaligned({src, src2, dst}, 16);
  if (src2)
    return launch_dot_attention(entry, a, n, vec4, table_dot_attention_gather_t_kernel<4, true, true>,
                                table_dot_attention_gather_t_kernel<1, false, true>,
                                table_dot_attention_gather_t_kernel<4, false, true>, stream);
  return launch_dot_attention(entry, a, n, vec4, table_dot_attention_gather_t_kernel<4, true, false>,
                              table_dot_attention_gather_t_kernel<1, false, false>,
                              table_dot_attention_gather_t_kernel<4, false, false>, stream);
}

}  // extern "C"
