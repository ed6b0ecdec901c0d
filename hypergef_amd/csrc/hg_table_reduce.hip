// Max and min over a dense neighbour table idx [rows, k] (include/hg_aggr.h, hg_table_reduce_* / hg_table_select_*): one hop
// with a comparison in place of the sum, the winner's position recorded, and the select-gather that is its gradient.
// hg_table.h has the lanes of the table gathers, which these kernels keep: a lane group of L = min(ceil(F / V), 64) lanes
// owns a destination row, V = 4 columns a lane on 16-byte rows (else 1), 64 / L rows a wave, kTableWaves waves a workgroup,
// kTableBatch row loads in flight.
//
// Reduce: a lane carries (best value, best position) per column; "none" is position -1, never a sentinel value.  The order
// (value, then the smaller position) is total, so a row may be cut any way.  A vertex row longer than HG_TABLE_SEQ_MAX is
// taken by its whole workgroup: lane group g of the P = kTableWaves R reads the batches g, g + P, g + 2 P .. of kTableBatch
// consecutive entries (neighbouring groups read neighbouring pos_v, and no group has more than one batch above another);
// the R groups of a wave meet in registers (R' / 2 .. 1 strides of L lanes, by lane shuffles), the four waves through one
// LDS slot each, and the row costs one barrier per column pass: the slots alternate between two buffers, so the barrier
// of pass t + 1 is what frees the buffer of pass t.  No tree in LDS, no atomics, no workspace.
//
// Select: the sum gather with the term (arg[r, c] == p ? gs[r, c] : nothing) -- a select, so a non-selected inf adds
// nothing -- in the sum gather's order: ascending entries, and a long vertex row in the pieces and the LDS tree of
// hg_aggr.h's ORDER paragraph.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "hg_aggr.h"
#include "hg_internal.h"
#include "hg_table.h"

namespace hg {
namespace {

template <typename E>
using Quad = E __attribute__((ext_vector_type(4)));

template <typename E, int V>
struct Lane {
  E v[V];
};

template <typename E, int V>
__device__ __forceinline__ Lane<E, V> lane_load(const E *p) {
  Lane<E, V> r;
  if constexpr (V == 4) {
    const Quad<E> x = *reinterpret_cast<const Quad<E> *>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[i] = x[i];
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <typename E, int V>
__device__ __forceinline__ void lane_store(E *p, const E (&v)[V]) {
  if constexpr (V == 4) {
    Quad<E> x;
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = v[i];
    *reinterpret_cast<Quad<E> *>(p) = x;
  } else {
    *p = v[0];
  }
}

// One entry q of a destination row: its table position p and the source row it names, or p = -1 where it is out of range
// (row 0 is then loaded and never used).  T: q indexes pos_v and the source is the hyperedge p / k; else p = q and the
// source is idx[p].
struct TableWalk {
  const int32_t *idx, *ptr_v, *pos_v;
  int32_t nrows, nsrc;  // destination and source rows
  int32_t k, F, entries;
  int32_t L, R;         // lanes per row, rows per wave
  int32_t R2, P2;       // the powers of two at or above R and kTableWaves R
};

template <bool T>
__device__ __forceinline__ void table_entry(const TableWalk &a, int q, bool o, int &p, int &j) {
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
  p = o ? p : -1;
}

template <bool T>
__device__ __forceinline__ void table_row_range(const TableWalk &a, int row, int &beg, int &end) {
  if (T) {
    beg = max(a.ptr_v[row], 0);
    end = min(a.ptr_v[row + 1], a.entries);
  } else {
    beg = row * a.k;
    end = beg + a.k;
  }
}

// ---- reduce -----------------------------------------------------------------------------------------------------------

struct TableReduceArgs {
  TableWalk t;
  const float *src, *dst_scale;
  float *dst;
  int32_t *arg;
};

// (v, p) replaces the best where it is a candidate and the best is none, or worse, or equal at a greater position
template <bool MAX>
__device__ __forceinline__ void best_take(float v, int p, float &bv, int &bp) {
  const bool wins = p >= 0 && (bp < 0 || (MAX ? v > bv : v < bv) || (v == bv && p < bp));
  bv = wins ? v : bv;
  bp = wins ? p : bp;
}

// the entries [beg, end) against the best of the columns c .. c + V - 1, a batch of row loads issued before the first compare
template <bool T, bool MAX, int V>
__device__ __forceinline__ void table_row_best(const TableReduceArgs &a, int beg, int end, int c, float (&bv)[V], int (&bp)[V]) {
  for (int b = beg; b < end; b += kTableBatch) {
    Lane<float, V> x[kTableBatch];
    int pp[kTableBatch];
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u) {
      int j;
      table_entry<T>(a.t, b + u, b + u < end, pp[u], j);
      x[u] = lane_load<float, V>(a.src + (size_t)j * a.t.F + c);
    }
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) best_take<MAX>(x[u].v[i], pp[u], bv[i], bp[i]);
  }
}

template <bool ARG, int V>
__device__ __forceinline__ void best_store(const TableReduceArgs &a, int row, int c, const float (&bv)[V], const int (&bp)[V]) {
  const float ds = a.dst_scale ? a.dst_scale[row] : 1.f;
  float out[V];
#pragma unroll
  for (int i = 0; i < V; ++i) out[i] = bp[i] < 0 ? 0.f : a.dst_scale ? ds * bv[i] : bv[i];  // no candidate: +0.0, no scale
  lane_store<float, V>(a.dst + (size_t)row * a.t.F + c, out);
  if constexpr (ARG) lane_store<int32_t, V>(a.arg + (size_t)row * a.t.F + c, bp);
}

template <bool T, bool MAX, bool ARG, int V>
__global__ __launch_bounds__(64 * kTableWaves) void table_reduce_kernel(TableReduceArgs a) {
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int L = a.t.L, R = a.t.R, F = a.t.F;
  const int sub = lane / L, cl = lane - sub * L;
  const bool lane_on = sub < R;
  const int RW = R * kTableWaves;
  const int64_t row0 = (int64_t)blockIdx.x * RW;
  const int64_t row64 = row0 + w * R + sub;
  const bool row_on = lane_on && row64 < a.t.nrows;
  const int row = row_on ? (int)row64 : 0;
  int beg = 0, end = 0;
  if (row_on) table_row_range<T>(a.t, row, beg, end);
  const bool is_long = T && end - beg > kTableSeqMax;

  if (row_on && !is_long) {
    for (int c0 = 0; c0 < F; c0 += L * V) {
      const int c = c0 + cl * V;
      if (c >= F) continue;
      float bv[V];
      int bp[V];
#pragma unroll
      for (int i = 0; i < V; ++i) bv[i] = 0.f, bp[i] = -1;
      table_row_best<T, MAX, V>(a, beg, end, c, bv, bp);
      best_store<ARG, V>(a, row, c, bv, bp);
    }
  }

  if constexpr (T) {
    // the tile's long rows, each by the whole workgroup in interleaved batches
    __shared__ __attribute__((aligned(16))) float wave_v[2][kTableWaves][64 * V];
    __shared__ __attribute__((aligned(16))) int wave_p[2][kTableWaves][64 * V];
    __shared__ unsigned long long long_rows[kTableWaves];
    const unsigned long long mine = __ballot(row_on && is_long && cl == 0);
    if (lane == 0) long_rows[w] = mine;
    __syncthreads();
    const int g = w * R + sub, stride = RW * kTableBatch;
    int buf = 0;
    for (int ww = 0; ww < kTableWaves; ++ww) {
      const unsigned long long mm = long_rows[ww];
      unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)mm), hi = __builtin_amdgcn_readfirstlane((unsigned)(mm >> 32));
      unsigned long long m = ((unsigned long long)hi << 32) | lo;
      while (m) {
        const int ln = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int lrow = (int)(row0 + ww * R + ln / L);
        int lbeg, lend;
        table_row_range<T>(a.t, lrow, lbeg, lend);
        for (int c0 = 0; c0 < F; c0 += L * V) {
          const int c = c0 + cl * V;
          const bool on = lane_on && c < F;
          float bv[V];
          int bp[V];
#pragma unroll
          for (int i = 0; i < V; ++i) bv[i] = 0.f, bp[i] = -1;
          if (on)
            for (int64_t b = (int64_t)lbeg + g * kTableBatch; b < lend; b += stride)
              table_row_best<T, MAX, V>(a, (int)b, (int)min(b + kTableBatch, (int64_t)lend), c, bv, bp);
          // the wave's R lane groups: every lane shuffles, a lane off or past F carries "none"
          for (int s = a.t.R2 >> 1; s >= 1; s >>= 1) {
            const int from = (lane + s * L) & 63;
            const bool has = sub + s < R;
#pragma unroll
            for (int i = 0; i < V; ++i) {
              const float ov = __shfl(bv[i], from, 64);
              const int op = __shfl(bp[i], from, 64);
              best_take<MAX>(ov, has ? op : -1, bv[i], bp[i]);
            }
          }
          if (sub == 0) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
              wave_v[buf][w][cl * V + i] = bv[i];
              wave_p[buf][w][cl * V + i] = bp[i];
            }
          }
          __syncthreads();
          if (w == 0 && sub == 0 && on) {
#pragma unroll
            for (int o = 1; o < kTableWaves; ++o)
#pragma unroll
              for (int i = 0; i < V; ++i) best_take<MAX>(wave_v[buf][o][cl * V + i], wave_p[buf][o][cl * V + i], bv[i], bp[i]);
            best_store<ARG, V>(a, lrow, c, bv, bp);
          }
          buf ^= 1;
        }
      }
    }
  }
}

// ---- select -----------------------------------------------------------------------------------------------------------

struct TableSelectArgs {
  TableWalk t;
  const float *gs;     // [source rows, F]: the reduce's incoming gradient, scaled
  const int32_t *arg;  // [source rows, F]: the reduce's winners
  float *dsrc;         // [destination rows, F]
};

// acc += gs[j, c ..] of the entries [beg, end) whose position is the winner of row j, ascending
template <bool T, int V>
__device__ __forceinline__ void table_row_select(const TableSelectArgs &a, int beg, int end, int c, float (&acc)[V]) {
  for (int b = beg; b < end; b += kTableBatch) {
    Lane<float, V> x[kTableBatch];
    Lane<int32_t, V> won[kTableBatch];
    int pp[kTableBatch];
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u) {
      int j;
      table_entry<T>(a.t, b + u, b + u < end, pp[u], j);
      x[u] = lane_load<float, V>(a.gs + (size_t)j * a.t.F + c);
      won[u] = lane_load<int32_t, V>(a.arg + (size_t)j * a.t.F + c);
    }
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] = (pp[u] >= 0 && won[u].v[i] == pp[u]) ? acc[i] + x[u].v[i] : acc[i];
  }
}

template <bool T, int V>
__global__ __launch_bounds__(64 * kTableWaves) void table_select_kernel(TableSelectArgs a) {
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int L = a.t.L, R = a.t.R, F = a.t.F;
  const int sub = lane / L, cl = lane - sub * L;
  const bool lane_on = sub < R;
  const int RW = R * kTableWaves;
  const int64_t row0 = (int64_t)blockIdx.x * RW;
  const int64_t row64 = row0 + w * R + sub;
  const bool row_on = lane_on && row64 < a.t.nrows;
  const int row = row_on ? (int)row64 : 0;
  int beg = 0, end = 0;
  if (row_on) table_row_range<T>(a.t, row, beg, end);
  const bool is_long = T && end - beg > kTableSeqMax;

  if (row_on && !is_long) {
    for (int c0 = 0; c0 < F; c0 += L * V) {
      const int c = c0 + cl * V;
      if (c >= F) continue;
      float acc[V];
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] = 0.f;
      table_row_select<T, V>(a, beg, end, c, acc);
      lane_store<float, V>(a.dsrc + (size_t)row * F + c, acc);
    }
  }

  if constexpr (T) {
    // the tile's long rows in the sum gather's order: P consecutive pieces, then the tree part[g] += part[g + s]
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
        int lbeg, lend;
        table_row_range<T>(a.t, lrow, lbeg, lend);
        const int64_t len = lend - lbeg, chunk = (len + P - 1) / P;
        const int gb = lbeg + (int)min((int64_t)g * chunk, len), ge = lbeg + (int)min((int64_t)(g + 1) * chunk, len);
        for (int c0 = 0; c0 < F; c0 += L * V) {
          const int c = c0 + cl * V;
          const bool on = lane_on && c < F;
          float *mypart = part + (size_t)(g * L + cl) * V;
          if (on) {
            float acc[V];
#pragma unroll
            for (int i = 0; i < V; ++i) acc[i] = 0.f;
            table_row_select<T, V>(a, gb, ge, c, acc);
#pragma unroll
            for (int i = 0; i < V; ++i) mypart[i] = acc[i];
          }
          __syncthreads();
          for (int s = a.t.P2 >> 1; s >= 1; s >>= 1) {
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
            for (int i = 0; i < V; ++i) out[i] = mypart[i];
            lane_store<float, V>(a.dsrc + (size_t)lrow * F + c, out);
          }
          __syncthreads();
        }
      }
    }
  }
}

// ---- launchers --------------------------------------------------------------------------------------------------------

// The walk of one hop over a table of [rows, k] entries that name n vertices, on the table gathers' lanes.  T: through the
// transpose, n destination rows out of `rows` source rows; else through idx, the other way round.
TableWalk table_walk(bool T, const int32_t *idx, const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k, int32_t n,
                     int32_t F, bool vec4) {
  TableWalk t{};
  t.idx = idx;
  t.ptr_v = ptr_v;
  t.pos_v = pos_v;
  t.nrows = T ? n : rows;
  t.nsrc = T ? rows : n;
  t.k = k;
  t.F = F;
  t.entries = rows * k;
  const int V = vec4 ? 4 : 1;
  t.L = std::min((F + V - 1) / V, 64);
  t.R = 64 / t.L;
  t.R2 = 1;
  while (t.R2 < t.R) t.R2 <<= 1;
  t.P2 = 1;
  while (t.P2 < t.R * kTableWaves) t.P2 <<= 1;
  return t;
}

dim3 table_grid(const TableWalk &t) {
  const int RW = t.R * kTableWaves;
  return dim3((unsigned)(((int64_t)t.nrows + RW - 1) / RW));
}

// what the four entries refuse, in the table gathers' order; a, b, c: the two row arrays read or written and the third
// (arg of a reduce may be null)
int reduce_refusal(const char *entry, const void *i0, const void *i1, const char *inames, int32_t rows, int32_t k, int32_t n,
                   int32_t F, const int32_t *op, const void *a, const void *b, const void *c, bool c_needed, const void *scale,
                   const char *null_text, const char *align_text) {
  if (!i0 || !i1) return fail(entry, HG_ERR_INVALID, std::string("null ") + inames);
  if (!a || !b || (c_needed && !c)) return fail(entry, HG_ERR_INVALID, null_text);
  if (const int st = size_refusal(entry, rows, k, n, F)) return st;
  if (op && *op != HG_REDUCE_MAX && *op != HG_REDUCE_MIN)
    return fail(entry, HG_ERR_INVALID, "op must be HG_REDUCE_MAX or HG_REDUCE_MIN, got " + std::to_string(*op));
  for (const void *p : {i0, i1, a, b, c, scale})
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, align_text);
  return HG_OK;
}

bool rows16(int32_t F, const void *a, const void *b, const void *c) {
  return F % 4 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0 && (uintptr_t)c % 16 == 0;
}

template <bool T, bool MAX, bool ARG>
void launch_reduce_v(const TableReduceArgs &a, bool vec4, hipStream_t s) {
  const dim3 grid = table_grid(a.t), block(64 * kTableWaves);
  if (vec4) hipLaunchKernelGGL((table_reduce_kernel<T, MAX, ARG, 4>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((table_reduce_kernel<T, MAX, ARG, 1>), grid, block, 0, s, a);
}

template <bool T>
int launch_table_reduce(const char *entry, const int32_t *idx, const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k,
                        int32_t n, int32_t F, int32_t op, const float *src, const float *dst_scale, float *dst, int32_t *arg,
                        hg_stream_t stream) {
  const bool vec4 = rows16(F, src, dst, arg);
  TableReduceArgs a{};
  a.t = table_walk(T, idx, ptr_v, pos_v, rows, k, n, F, vec4);
  a.src = src;
  a.dst_scale = dst_scale;
  a.dst = dst;
  a.arg = arg;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool mx = op == HG_REDUCE_MAX;
  if (mx && arg) launch_reduce_v<T, true, true>(a, vec4, s);
  else if (mx) launch_reduce_v<T, true, false>(a, vec4, s);
  else if (arg) launch_reduce_v<T, false, true>(a, vec4, s);
  else launch_reduce_v<T, false, false>(a, vec4, s);
  return launch_check(entry);
}

template <bool T>
int launch_table_select(const char *entry, const int32_t *idx, const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k,
                        int32_t n, int32_t F, const float *gs, const int32_t *arg, float *dsrc, hg_stream_t stream) {
  const bool vec4 = rows16(F, gs, arg, dsrc);
  TableSelectArgs a{};
  a.t = table_walk(T, idx, ptr_v, pos_v, rows, k, n, F, vec4);
  a.gs = gs;
  a.arg = arg;
  a.dsrc = dsrc;
  const dim3 grid = table_grid(a.t), block(64 * kTableWaves);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec4) hipLaunchKernelGGL((table_select_kernel<T, 4>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((table_select_kernel<T, 1>), grid, block, 0, s, a);
  return launch_check(entry);
}

const char *const kReduceNull = "null src or dst";
const char *const kReduceAlign = "the table, src, dst_scale, dst and arg must be 4-byte aligned";
const char *const kSelectNull = "null gs, arg or dsrc";
const char *const kSelectAlign = "the table, gs, arg and dsrc must be 4-byte aligned";

}  // namespace
}  // namespace hg

extern "C" {

int hg_table_reduce_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, int32_t op, const float *src,
                        const float *dst_scale, float *dst, int32_t *arg, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_reduce_f32";
  if (const int st = reduce_refusal(entry, idx, idx, "idx", rows, k, n, F, &op, src, dst, arg, false, dst_scale, kReduceNull, kReduceAlign))
    return st;
  return launch_table_reduce<false>(entry, idx, nullptr, nullptr, rows, k, n, F, op, src, dst_scale, dst, arg, stream);
}

int hg_table_reduce_t_f32(const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k, int32_t n, int32_t F, int32_t op,
                          const float *src, const float *dst_scale, float *dst, int32_t *arg, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_reduce_t_f32";
  if (const int st = reduce_refusal(entry, ptr_v, pos_v, "ptr_v or pos_v", rows, k, n, F, &op, src, dst, arg, false, dst_scale,
                                    kReduceNull, kReduceAlign))
    return st;
  return launch_table_reduce<true>(entry, nullptr, ptr_v, pos_v, rows, k, n, F, op, src, dst_scale, dst, arg, stream);
}

int hg_table_select_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, const float *gs, const int32_t *arg,
                        float *dsrc, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_select_f32";
  if (const int st = reduce_refusal(entry, idx, idx, "idx", rows, k, n, F, nullptr, gs, dsrc, arg, true, nullptr, kSelectNull, kSelectAlign))
    return st;
  return launch_table_select<false>(entry, idx, nullptr, nullptr, rows, k, n, F, gs, arg, dsrc, stream);
}

int hg_table_select_t_f32(const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k, int32_t n, int32_t F,
                          const float *gs, const int32_t *arg, float *dsrc, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_select_t_f32";
  if (const int st = reduce_refusal(entry, ptr_v, pos_v, "ptr_v or pos_v", rows, k, n, F, nullptr, gs, dsrc, arg, true, nullptr,
                                    kSelectNull, kSelectAlign))
    return st;
  return launch_table_select<true>(entry, nullptr, ptr_v, pos_v, rows, k, n, F, gs, arg, dsrc, stream);
}

}  // extern "C"
