// Aggregation over a dense neighbour table idx [rows, k] (include/hg_aggr.h, hg_table_*): the table's transpose and the
// two row gathers, with no plan and no host step.  hg_table.h has the layout of the work; the order of every sum is in
// include/hg_aggr.h.  The library is built without contraction, and nothing here asks for an fma: every term is rounded
// on its own and added with one rounded add.  No floating-point atomics; the transpose's only atomics count integers in
// LDS.
#include <hip/hip_runtime.h>

#include <string>

#include "hg_aggr.h"
#include "hg_internal.h"
#include "hg_table.h"

namespace hg {

TableLayout table_layout(int64_t rows, int k, int64_t n) {
  TableLayout L;
  L.entries = rows * k;
  L.tiles = (L.entries + kTableTile - 1) / kTableTile;
  int bits = 0;
  while (((int64_t)1 << bits) <= n) ++bits;  // the largest key is n itself
  L.passes = (bits + kTableRadixBits - 1) / kTableRadixBits;
  L.alt = 0;
  L.hist = ((size_t)L.entries * 4 + 255) / 256 * 256;
  L.total = L.hist + (size_t)kTableBins * (size_t)L.tiles * 4;
  return L;
}

namespace {

static_assert(kTableBlock == kTableBins, "one thread per bin");
static_assert(kTableBlock == 64 * 4, "four waves rank a tile");

// ---- transpose --------------------------------------------------------------------------------------------------------

struct SortArgs {
  const int32_t *idx;
  const int32_t *in;  // the positions in the order of the pass before, or null: 0, 1, 2 ..
  int32_t *out;
  int32_t *hist;      // [kTableBins, tiles]: counts, then (scanned) where each tile's run of a digit starts
  int32_t entries, n, tiles, shift;
};

// an entry that names no vertex sorts behind every vertex
__device__ __forceinline__ int table_key(const int32_t *idx, int n, int p) {
  const unsigned v = (unsigned)idx[p];
  return v < (unsigned)n ? (int)v : n;
}

__global__ __launch_bounds__(kTableBlock) void table_hist_kernel(SortArgs a) {
  __shared__ int cnt[kTableBins];
  const int t = threadIdx.x;
  cnt[t] = 0;
  __syncthreads();
  const unsigned base = blockIdx.x * (unsigned)kTableTile;
#pragma unroll
  for (int e = 0; e < kTableItems; ++e) {
    const unsigned i = base + e * kTableBlock + t;
    if (i < (unsigned)a.entries) {
      const int p = a.in ? a.in[i] : (int)i;
      atomicAdd(&cnt[(table_key(a.idx, a.n, p) >> a.shift) & (kTableBins - 1)], 1);
    }
  }
  __syncthreads();
  a.hist[(size_t)t * a.tiles + blockIdx.x] = cnt[t];
}

// exclusive scan of h[0 .. m) in place, by one workgroup
__global__ __launch_bounds__(kTableScanBlock) void table_scan_kernel(int32_t *h, int64_t m) {
  constexpr int kWaves = kTableScanBlock / 64;
  __shared__ int wsum[kWaves];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int carry = 0;
  for (int64_t b = 0; b < m; b += kTableScanBlock * 4) {
    const int64_t i0 = b + (int64_t)t * 4;
    int v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = i0 + u < m ? h[i0 + u] : 0;
    const int s = v[0] + v[1] + v[2] + v[3];
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int x = __shfl_up(inc, o, 64);
      if (lane >= o) inc += x;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < kWaves; ++j) {
      const int x = wsum[j];
      if (j < w) before += x;
      total += x;
    }
    int ex = carry + before + inc - s;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i0 + u < m) h[i0 + u] = ex;
      ex += v[u];
    }
    carry += total;
    __syncthreads();
  }
}

// A tile's positions in ascending order are (wave w, round e, lane): slot w kTableItems + e holds 64 of them.  A position's
// place is its digit's start for this tile, plus the digit's count in the slots before, plus its rank among the slot's
// lanes with the same digit: the order within a digit is the order of the input.
__global__ __launch_bounds__(kTableBlock) void table_scatter_kernel(SortArgs a) {
  constexpr int kSlots = 4 * kTableItems;
  __shared__ int cnt[kSlots][kTableBins];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
  for (int s = 0; s < kSlots; ++s) cnt[s][t] = 0;
  __syncthreads();
  const unsigned base = blockIdx.x * (unsigned)kTableTile;
  int pv[kTableItems], dg[kTableItems], rk[kTableItems];
#pragma unroll
  for (int e = 0; e < kTableItems; ++e) {
    const int slot = w * kTableItems + e;
    const unsigned i = base + slot * 64 + lane;
    const bool ok = i < (unsigned)a.entries;
    const int p = ok ? (a.in ? a.in[i] : (int)i) : 0;
    const int d = (table_key(a.idx, a.n, p) >> a.shift) & (kTableBins - 1);
    unsigned long long same = __ballot(ok);
#pragma unroll
    for (int b = 0; b < kTableRadixBits; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long have = __ballot(ok && bit);
      same &= bit ? have : ~have;
    }
    const int rank = __popcll(same & ((1ull << lane) - 1ull));
    if (ok && rank == 0) cnt[slot][d] = __popcll(same);
    pv[e] = p;
    dg[e] = ok ? d : -1;
    rk[e] = rank;
  }
  __syncthreads();
  {
    int run = a.hist[(size_t)t * a.tiles + blockIdx.x];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
      const int c = cnt[s][t];
      cnt[s][t] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kTableItems; ++e)
    if (dg[e] >= 0) {
      const unsigned at = (unsigned)(cnt[w * kTableItems + e][dg[e]] + rk[e]);
      if (at < (unsigned)a.entries) a.out[at] = pv[e];
    }
}

// pos is sorted by key: vertex u's entries start where the first key >= u stands
__global__ __launch_bounds__(256) void table_ptr_kernel(const int32_t *idx, const int32_t *pos, int32_t entries, int32_t n,
                                                       int32_t *ptr_v) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q > (unsigned)entries) return;
  const int before = q == 0 ? -1 : table_key(idx, n, pos[q - 1]);
  const int here = q == (unsigned)entries ? n : table_key(idx, n, pos[q]);
  for (int u = before + 1; u <= here; ++u) ptr_v[u] = (int32_t)q;
}

// ---- gathers ----------------------------------------------------------------------------------------------------------

struct TableGatherArgs {
  const int32_t *idx;            // the table [rows, k] (the hyperedge gather)
  const int32_t *ptr_v, *pos_v;  // its transpose (the vertex gather)
  const float *src, *w, *src_scale, *dst_scale;
  float *dst;
  int32_t nrows, nsrc;  // destination and source rows
  int32_t k, F, entries;
  int32_t L, R;         // lanes per row, rows per wave
  int32_t P2;           // the power of two at or above kTableWaves R
  const float *ctr;     // the difference gathers' centre rows [destination rows, F]; last: the plain instances' offsets stay
};

template <int V>
struct Cols {
  float v[V];
};

template <int V>
__device__ __forceinline__ Cols<V> cols_load(const float *p) {
  Cols<V> r;
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
__device__ __forceinline__ void cols_store(float *p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = float4{v[0], v[1], v[2], v[3]};
  else *p = v[0];
}

// acc += the terms of the entries [beg, end), ascending, for the columns c .. c + V - 1.  T: an entry q is position
// pos_v[q] of the table and gathers the hyperedge's row; else it is position q itself and gathers row idx[q].  A batch of
// row loads is issued, then added in order.  An entry that is out of range loads row 0 and is not added.  D (the
// difference gathers): the term starts from cv - src[j], cv the destination row's centre columns, rounded on its own.
template <bool T, int V, bool D>
__device__ __forceinline__ void table_row_sum(const TableGatherArgs &a, int beg, int end, int c, const Cols<V> &cv,
                                              float (&acc)[V]) {
  for (int b = beg; b < end; b += kTableBatch) {
    Cols<V> x[kTableBatch];
    float wv[kTableBatch], sv[kTableBatch];
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
      wv[u] = a.w ? a.w[p] : 1.f;
      sv[u] = a.src_scale ? a.src_scale[j] : 1.f;
      x[u] = cols_load<V>(a.src + (size_t)j * a.F + c);
    }
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float term = x[u].v[i];
        if constexpr (D) term = cv.v[i] - term;
        if (a.src_scale) term = term * sv[u];
        if (a.w) term = term * wv[u];
        acc[i] = ok[u] ? acc[i] + term : acc[i];
      }
  }
}

template <bool T, int V, bool D = false>
__global__ __launch_bounds__(64 * kTableWaves) void table_gather_kernel(TableGatherArgs a) {
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
    for (int c0 = 0; c0 < F; c0 += L * V) {
      const int c = c0 + cl * V;
      if (c >= F) continue;
      float acc[V];
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] = 0.f;
      Cols<V> cv{};
      if constexpr (D) cv = cols_load<V>(a.ctr + (size_t)row * F + c);
      table_row_sum<T, V, D>(a, beg, end, c, cv, acc);
      if (a.dst_scale && end > beg) {  // an empty row stays +0.0 whatever its scale
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = ds * acc[i];
      }
      cols_store<V>(a.dst + (size_t)row * F + c, acc);
    }
  }

  if constexpr (T) {
    // the tile's long rows, one after the other, by the whole workgroup
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
            Cols<V> cv{};
            if constexpr (D) cv = cols_load<V>(a.ctr + (size_t)lrow * F + c);
            table_row_sum<T, V, D>(a, gb, ge, c, cv, acc);
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
            cols_store<V>(a.dst + (size_t)lrow * F + c, out);
          }
          __syncthreads();
        }
      }
    }
  }
}

// ---- distances of a table, and the dot products of its entries -------------------------------------------------------------

struct TableDistArgs {
  const int32_t *idx;
  const float *Q, *X;
  float *dist;
  int32_t n, k, F, entries;
};

// One lane per table position p: the chain d2 = fma(q - x, q - x, d2) over c = 0 .. F - 1 cannot be cut without moving
// bits, so a lane walks both rows, kTableDistLoads loads of each in flight.  V columns a load; the bits do not depend on V.
template <int V>
__global__ __launch_bounds__(kTableBlock) void table_dist_kernel(TableDistArgs a) {
  const int64_t p64 = (int64_t)blockIdx.x * kTableBlock + threadIdx.x;
  if (p64 >= a.entries) return;
  const int p = (int)p64, F = a.F;
  const int j = a.idx[p];
  if ((unsigned)j >= (unsigned)a.n) {  // names no row: +0.0, and nothing is read through it
    a.dist[p] = 0.f;
    return;
  }
  const float *q = a.Q + (size_t)(p / a.k) * F, *x = a.X + (size_t)j * F;
  constexpr int kStep = V * kTableDistLoads;
  float acc = 0.f;
  int c = 0;
  for (; c + kStep <= F; c += kStep) {
    Cols<V> qv[kTableDistLoads], xv[kTableDistLoads];
#pragma unroll
    for (int u = 0; u < kTableDistLoads; ++u) {
      qv[u] = cols_load<V>(q + c + u * V);
      xv[u] = cols_load<V>(x + c + u * V);
    }
#pragma unroll
    for (int u = 0; u < kTableDistLoads; ++u)
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float d = qv[u].v[i] - xv[u].v[i];
        acc = __builtin_fmaf(d, d, acc);
      }
  }
  for (; c < F; c += V) {
    const Cols<V> qv = cols_load<V>(q + c), xv = cols_load<V>(x + c);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float d = qv.v[i] - xv.v[i];
      acc = __builtin_fmaf(d, d, acc);
    }
  }
  a.dist[p] = acc;
}

struct TableDotArgs {
  const int32_t *idx;
  const float *A, *a_scale, *B, *C, *D;
  float *out;
  int32_t rows, n, k, F;
  int32_t L, R;  // lanes per table row (a power of two), rows per wave
};

// out[p] = a_scale[j] <A[j], B[i]> + <C[j], D[i]> for p = (i, s), j = idx[p].  A lane group of L lanes owns table row i;
// lane l of it owns the columns c0 + l V .. + V - 1 of every pass c0 = 0, L V, 2 L V ..  Per entry a lane runs one fma
// chain per product over its columns in ascending order, forms t = a_scale[j] * s1 + s2 (each step rounded, no fma) and
// the group adds the t in the xor butterfly t += t[lane ^ o], o = L / 2 .. 1.  B[i] / D[i] of the first pass stay in
// registers over the row's entries (every pass where F <= L V); kTableDotBatch gathered rows are in flight per group.
template <int V, bool TWO>
__global__ __launch_bounds__(64 * kTableWaves) void table_dot_kernel(TableDotArgs a) {
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int L = a.L, R = a.R, F = a.F, k = a.k;
  const int sub = lane / L, cl = lane - sub * L;
  const int64_t row64 = ((int64_t)blockIdx.x * kTableWaves + w) * R + sub;
  const bool row_on = row64 < a.rows;  // a whole lane group is on or off; an off group computes row 0 and stores nothing
  const int row = row_on ? (int)row64 : 0;
  const int step = L * V;
  const bool one_pass = F <= step;
  const int cfirst = cl * V;
  const bool on0 = cfirst < F;
  const size_t brow = (size_t)row * F;
  const Cols<V> b0 = cols_load<V>(a.B + brow + (on0 ? cfirst : 0));
  Cols<V> d0{};
  if constexpr (TWO) d0 = cols_load<V>(a.D + brow + (on0 ? cfirst : 0));
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
    for (int c0 = 0; c0 < F; c0 += step) {
      const int c = c0 + cfirst;
      const bool on = c < F;
      const int ce = on ? c : 0;
      Cols<V> bv = b0, dv = d0;
      if (!one_pass && c0 > 0) {
        bv = cols_load<V>(a.B + brow + ce);
        if constexpr (TWO) dv = cols_load<V>(a.D + brow + ce);
      }
      Cols<V> av[kTableDotBatch], cv[kTableDotBatch];
#pragma unroll
      for (int u = 0; u < kTableDotBatch; ++u) {
        av[u] = cols_load<V>(a.A + (size_t)jv[u] * F + ce);
        if constexpr (TWO) cv[u] = cols_load<V>(a.C + (size_t)jv[u] * F + ce);
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
      if (row_on && cl == 0 && s0 + u < k) a.out[(size_t)row * k + s0 + u] = ok[u] ? tt : 0.f;
    }
  }
}

// what every table entry refuses about k and the table's size
int table_refusal(const char *entry, int32_t rows, int32_t k) {
  if (k < 1 || k > kTableMaxK) return fail(entry, HG_ERR_INVALID, "k must be in 1 .. 64, got " + std::to_string(k));
  if ((int64_t)rows * k > INT32_MAX) return fail(entry, HG_ERR_INVALID, "rows * k must be below 2^31");
  return HG_OK;
}

// the sizes' refusals of every entry that takes rows of F columns, in the order include/hg_aggr.h gives
int size_refusal(const char *entry, int32_t rows, int32_t k, int32_t n, int32_t F) {
  if (rows < 1 || n < 1 || F < 1) return fail(entry, HG_ERR_INVALID, "rows, n and F must be at least 1");
  return table_refusal(entry, rows, k);
}

// what the four gathers refuse about the table and the rows, in the same order
int gather_refusal(const char *entry, int32_t rows, int32_t k, int32_t n, int32_t F, const float *src, const float *w,
                   const float *src_scale, const float *dst_scale, const float *dst) {
  if (!src || !dst) return fail(entry, HG_ERR_INVALID, "null src or dst");
  if (const int st = size_refusal(entry, rows, k, n, F)) return st;
  for (const void *p : {(const void *)src, (const void *)w, (const void *)src_scale, (const void *)dst_scale, (const void *)dst})
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, "src, w, the scales and dst must be 4-byte aligned");
  return HG_OK;
}

int launch_check(const char *entry) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(entry, HG_ERR_HIP, std::string("launch: ") + hipGetErrorString(e));
  return HG_OK;
}

// One of the four gathers over a table of [rows, k] entries that name n vertices.  T: the vertex gather through the
// transpose (ptr_v, pos_v; idx is null), n destination rows out of `rows` source rows; else the hyperedge gather through
// idx, the other way round.  D: the difference gather, with the destination rows' centres ctr (else null).
template <bool T, bool D>
int launch_table_gather(const char *entry, const int32_t *idx, const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k,
                        int32_t n, int32_t F, const float *src, const float *w, const float *src_scale, const float *dst_scale,
                        const float *ctr, float *dst, hg_stream_t stream) {
  TableGatherArgs a{};
  a.idx = idx;
  a.ptr_v = ptr_v;
  a.pos_v = pos_v;
  a.src = src;
  a.w = w;
  a.src_scale = src_scale;
  a.dst_scale = dst_scale;
  a.ctr = ctr;
  a.dst = dst;
  a.nrows = T ? n : rows;
  a.nsrc = T ? rows : n;
  a.k = k;
  a.F = F;
  a.entries = rows * k;
  const bool vec4 = F % 4 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0 && (!D || (uintptr_t)ctr % 16 == 0);
  const int V = vec4 ? 4 : 1;
  a.L = std::min((F + V - 1) / V, 64);
  a.R = 64 / a.L;
  a.P2 = 1;
  while (a.P2 < a.R * kTableWaves) a.P2 <<= 1;
  const int RW = a.R * kTableWaves;
  const dim3 grid((unsigned)(((int64_t)a.nrows + RW - 1) / RW)), block(64 * kTableWaves);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec4) hipLaunchKernelGGL((table_gather_kernel<T, 4, D>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((table_gather_kernel<T, 1, D>), grid, block, 0, s, a);
  return launch_check(entry);
}

}  // namespace
}  // namespace hg

extern "C" {

int hg_table_seq_max(void) { return hg::kTableSeqMax; }

size_t hg_table_transpose_workspace_bytes(int32_t rows, int32_t k, int32_t n) {
  if (rows < 1 || n < 1 || k < 1 || k > hg::kTableMaxK || (int64_t)rows * k > INT32_MAX) return 0;
  return hg::table_layout(rows, k, n).total;
}

int hg_table_transpose(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t *ptr_v, int32_t *pos_v,
                       void *workspace, size_t workspace_bytes, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_transpose";
  if (!idx || !ptr_v || !pos_v) return fail(entry, HG_ERR_INVALID, "null idx, ptr_v or pos_v");
  if (rows < 1 || n < 1) return fail(entry, HG_ERR_INVALID, "rows and n must be at least 1");
  if (const int st = table_refusal(entry, rows, k)) return st;
  for (const void *p : {(const void *)idx, (const void *)ptr_v, (const void *)pos_v})
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, "idx, ptr_v and pos_v must be 4-byte aligned");
  const TableLayout L = table_layout(rows, k, n);
  if (!workspace || workspace_bytes < L.total || (uintptr_t)workspace % 4)
    return fail(entry, HG_ERR_WORKSPACE, "workspace of " + std::to_string(workspace_bytes) +
                                             " bytes, hg_table_transpose_workspace_bytes asks for " + std::to_string(L.total) +
                                             " (4-byte aligned)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  int32_t *alt = reinterpret_cast<int32_t *>(ws + L.alt);
  SortArgs a{};
  a.idx = idx;
  a.hist = reinterpret_cast<int32_t *>(ws + L.hist);
  a.entries = (int32_t)L.entries;
  a.n = n;
  a.tiles = (int32_t)L.tiles;
  for (int pass = 0; pass < L.passes; ++pass) {
    a.shift = pass * kTableRadixBits;
    a.out = (L.passes - 1 - pass) % 2 == 0 ? pos_v : alt;  // the last pass writes pos_v
    hipLaunchKernelGGL(table_hist_kernel, dim3((unsigned)L.tiles), dim3(kTableBlock), 0, s, a);
    hipLaunchKernelGGL(table_scan_kernel, dim3(1), dim3(kTableScanBlock), 0, s, a.hist, (int64_t)kTableBins * L.tiles);
    hipLaunchKernelGGL(table_scatter_kernel, dim3((unsigned)L.tiles), dim3(kTableBlock), 0, s, a);
    if (const int st = launch_check(entry)) return st;
    a.in = a.out;
  }
  hipLaunchKernelGGL(table_ptr_kernel, dim3((unsigned)(L.entries / 256 + 1)), dim3(256), 0, s, idx, (const int32_t *)pos_v,
                     a.entries, n, ptr_v);
  return launch_check(entry);
}

int hg_table_gather_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, const float *src, const float *w,
                        const float *src_scale, const float *dst_scale, float *dst, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_gather_f32";
  if (!idx) return fail(entry, HG_ERR_INVALID, "null idx");
  if (const int st = gather_refusal(entry, rows, k, n, F, src, w, src_scale, dst_scale, dst)) return st;
  if ((uintptr_t)idx % 4) return fail(entry, HG_ERR_UNSUPPORTED, "idx must be 4-byte aligned");
  return launch_table_gather<false, false>(entry, idx, nullptr, nullptr, rows, k, n, F, src, w, src_scale, dst_scale, nullptr, dst, stream);
}

int hg_table_gather_t_f32(const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k, int32_t n, int32_t F,
                          const float *src, const float *w, const float *src_scale, const float *dst_scale, float *dst,
                          hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_gather_t_f32";
  if (!ptr_v || !pos_v) return fail(entry, HG_ERR_INVALID, "null ptr_v or pos_v");
  if (const int st = gather_refusal(entry, rows, k, n, F, src, w, src_scale, dst_scale, dst)) return st;
  if ((uintptr_t)ptr_v % 4 || (uintptr_t)pos_v % 4) return fail(entry, HG_ERR_UNSUPPORTED, "ptr_v and pos_v must be 4-byte aligned");
  return launch_table_gather<true, false>(entry, nullptr, ptr_v, pos_v, rows, k, n, F, src, w, src_scale, dst_scale, nullptr, dst, stream);
}

int hg_table_gather_diff_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, const float *src,
                             const float *w, const float *src_scale, const float *dst_scale, const float *ctr, float *dst,
                             hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_gather_diff_f32";
  if (!idx) return fail(entry, HG_ERR_INVALID, "null idx");
  if (!ctr) return fail(entry, HG_ERR_INVALID, "null ctr");
  if (const int st = gather_refusal(entry, rows, k, n, F, src, w, src_scale, dst_scale, dst)) return st;
  if ((uintptr_t)idx % 4 || (uintptr_t)ctr % 4) return fail(entry, HG_ERR_UNSUPPORTED, "idx and ctr must be 4-byte aligned");
  return launch_table_gather<false, true>(entry, idx, nullptr, nullptr, rows, k, n, F, src, w, src_scale, dst_scale, ctr, dst, stream);
}

int hg_table_gather_t_diff_f32(const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k, int32_t n, int32_t F,
                               const float *src, const float *w, const float *src_scale, const float *dst_scale,
                               const float *ctr, float *dst, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_gather_t_diff_f32";
  if (!ptr_v || !pos_v) return fail(entry, HG_ERR_INVALID, "null ptr_v or pos_v");
  if (!ctr) return fail(entry, HG_ERR_INVALID, "null ctr");
  if (const int st = gather_refusal(entry, rows, k, n, F, src, w, src_scale, dst_scale, dst)) return st;
  if ((uintptr_t)ptr_v % 4 || (uintptr_t)pos_v % 4 || (uintptr_t)ctr % 4)
    return fail(entry, HG_ERR_UNSUPPORTED, "ptr_v, pos_v and ctr must be 4-byte aligned");
  return launch_table_gather<true, true>(entry, nullptr, ptr_v, pos_v, rows, k, n, F, src, w, src_scale, dst_scale, ctr, dst, stream);
}

int hg_table_dist_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, const float *Q, const float *X,
                      float *dist, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_dist_f32";
  if (!idx || !Q || !X || !dist) return fail(entry, HG_ERR_INVALID, "null idx, Q, X or dist");
  if (const int st = size_refusal(entry, rows, k, n, F)) return st;
  for (const void *p : {(const void *)idx, (const void *)Q, (const void *)X, (const void *)dist})
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, "idx, Q, X and dist must be 4-byte aligned");
  TableDistArgs a{};
  a.idx = idx;
  a.Q = Q;
  a.X = X;
  a.dist = dist;
  a.n = n;
  a.k = k;
  a.F = F;
  a.entries = rows * k;
  const bool vec4 = F % 4 == 0 && (uintptr_t)Q % 16 == 0 && (uintptr_t)X % 16 == 0;
  const dim3 grid((unsigned)(((int64_t)a.entries + kTableBlock - 1) / kTableBlock)), block(kTableBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec4) hipLaunchKernelGGL(table_dist_kernel<4>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(table_dist_kernel<1>, grid, block, 0, s, a);
  return launch_check(entry);
}

int hg_table_dot_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, const float *A, const float *a_scale,
                     const float *B, const float *C, const float *D, float *out, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_dot_f32";
  if (!idx) return fail(entry, HG_ERR_INVALID, "null idx");
  if (!A || !B || !out) return fail(entry, HG_ERR_INVALID, "null A, B or out");
  if (!C != !D) return fail(entry, HG_ERR_INVALID, "C and D must both be given or both be null");
  if (const int st = size_refusal(entry, rows, k, n, F)) return st;
  for (const void *p : {(const void *)idx, (const void *)A, (const void *)a_scale, (const void *)B, (const void *)C,
                        (const void *)D, (const void *)out})
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, "idx, A, a_scale, B, C, D and out must be 4-byte aligned");
  TableDotArgs a{};
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
  bool vec4 = F % 4 == 0;
  for (const void *p : {(const void *)A, (const void *)B, (const void *)C, (const void *)D}) vec4 = vec4 && (uintptr_t)p % 16 == 0;
  const int V = vec4 ? 4 : 1;
  a.L = 1;
  while (a.L < std::min((F + V - 1) / V, 64)) a.L <<= 1;
  a.R = 64 / a.L;
  const int RW = a.R * kTableWaves;
  const dim3 grid((unsigned)(((int64_t)rows + RW - 1) / RW)), block(64 * kTableWaves);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec4 && C) hipLaunchKernelGGL((table_dot_kernel<4, true>), grid, block, 0, s, a);
  else if (vec4) hipLaunchKernelGGL((table_dot_kernel<4, false>), grid, block, 0, s, a);
  else if (C) hipLaunchKernelGGL((table_dot_kernel<1, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((table_dot_kernel<1, false>), grid, block, 0, s, a);
  return launch_check(entry);
}

}  // extern "C"
