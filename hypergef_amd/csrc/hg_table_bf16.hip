// bfloat16 feature rows over a neighbour table (include/hg_aggr.h, hg_table_*_bf16): the row gathers, the distances and the
// dot products of hg_table.hip on rows of half the bytes.  hg_table.h has the layout of the work.  Every instance widens a
// bfloat16 element in the load (a 16-bit shift, exact), runs the float32 instance's arithmetic on the floats that instance
// would see -- every term rounded on its own, one rounded add, the dist and dot chains one explicit fma a column -- and
// rounds a bfloat16 result once, to nearest-even, in the store.  So a call equals the float32 call on the widened rows bit
// for bit.  A file of its own: it is built without the packed float32 instructions, hg_table.hip is built as it always was.
#include <hip/hip_runtime.h>

#include <string>

#include "hg_aggr.h"
#include "hg_internal.h"
#include "hg_table.h"

namespace hg {
namespace {

typedef uint16_t bf16_t;  // a bfloat16 element in memory

__device__ __forceinline__ float widen_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float widen_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ unsigned narrow2(float lo, float hi) {  // v_cvt_pk_bf16_f32: round to nearest even
  return (unsigned)__builtin_bit_cast(uint16_t, (__bf16)lo) | ((unsigned)__builtin_bit_cast(uint16_t, (__bf16)hi) << 16);
}

// V consecutive columns of a row of element type E as they travel: one 16-byte access for 8 bfloat16 or 4 float32 columns,
// two for 8 float32 columns, one 8-byte access for 4 bfloat16 columns (the long rows of the transposed gather).  A chunk
// stays packed while its load is in flight and is widened where it is used.
template <int V, typename E>
struct Chunk;

template <>
struct Chunk<8, bf16_t> {
  uint4 x;
  __device__ __forceinline__ void load(const bf16_t *p) { x = *reinterpret_cast<const uint4 *>(p); }
  __device__ __forceinline__ void get(float (&v)[8]) const {
    v[0] = widen_lo(x.x), v[1] = widen_hi(x.x), v[2] = widen_lo(x.y), v[3] = widen_hi(x.y);
    v[4] = widen_lo(x.z), v[5] = widen_hi(x.z), v[6] = widen_lo(x.w), v[7] = widen_hi(x.w);
  }
  __device__ __forceinline__ static void store(bf16_t *p, const float (&v)[8]) {
    *reinterpret_cast<uint4 *>(p) = uint4{narrow2(v[0], v[1]), narrow2(v[2], v[3]), narrow2(v[4], v[5]), narrow2(v[6], v[7])};
  }
};

template <>
struct Chunk<4, bf16_t> {
  uint2 x;
  __device__ __forceinline__ void load(const bf16_t *p) { x = *reinterpret_cast<const uint2 *>(p); }
  __device__ __forceinline__ void get(float (&v)[4]) const {
    v[0] = widen_lo(x.x), v[1] = widen_hi(x.x), v[2] = widen_lo(x.y), v[3] = widen_hi(x.y);
  }
  __device__ __forceinline__ static void store(bf16_t *p, const float (&v)[4]) {
    *reinterpret_cast<uint2 *>(p) = uint2{narrow2(v[0], v[1]), narrow2(v[2], v[3])};
  }
};

template <>
struct Chunk<8, float> {
  float4 x, y;
  __device__ __forceinline__ void load(const float *p) {
    x = *reinterpret_cast<const float4 *>(p);
    y = *reinterpret_cast<const float4 *>(p + 4);
  }
  __device__ __forceinline__ void get(float (&v)[8]) const {
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w, v[4] = y.x, v[5] = y.y, v[6] = y.z, v[7] = y.w;
  }
  __device__ __forceinline__ static void store(float *p, const float (&v)[8]) {
    *reinterpret_cast<float4 *>(p) = float4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<float4 *>(p + 4) = float4{v[4], v[5], v[6], v[7]};
  }
};

template <>
struct Chunk<4, float> {
  float4 x;
  __device__ __forceinline__ void load(const float *p) { x = *reinterpret_cast<const float4 *>(p); }
  __device__ __forceinline__ void get(float (&v)[4]) const { v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w; }
  __device__ __forceinline__ static void store(float *p, const float (&v)[4]) {
    *reinterpret_cast<float4 *>(p) = float4{v[0], v[1], v[2], v[3]};
  }
};

// ---- gathers ----------------------------------------------------------------------------------------------------------

template <typename ES, typename ED>
struct GatherB16Args {
  const int32_t *idx;            // the table [rows, k] (the hyperedge gather)
  const int32_t *ptr_v, *pos_v;  // its transpose (the vertex gather)
  const ES *src;
  const float *w, *src_scale, *dst_scale;
  const ES *ctr;                 // the difference form's centre rows [destination rows, F], of the source's type
  ED *dst;
  int32_t nrows, nsrc;  // destination and source rows
  int32_t k, F, entries;
  int32_t L8, R8;       // the 16-byte geometry: lanes per row at 8 columns a lane, rows per wave
  int32_t L, R, P2;     // the float32 call's own geometry at 4 columns a lane: the long rows of the transposed gather
};

// hg_table.hip's table_row_sum on chunks of V columns of type ES: acc += the terms of the entries [beg, end), ascending.
// kTableBatch row loads are issued packed, then widened and added in order.
template <bool T, int V, bool D, typename ES, typename ED>
__device__ __forceinline__ void row_sum_b16(const GatherB16Args<ES, ED> &a, int beg, int end, int c, const float (&cv)[V],
                                            float (&acc)[V]) {
  for (int b = beg; b < end; b += kTableBatch) {
    Chunk<V, ES> x[kTableBatch];
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
      x[u].load(a.src + (size_t)j * a.F + c);
    }
#pragma unroll
    for (int u = 0; u < kTableBatch; ++u) {
      float xv[V];
      x[u].get(xv);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float term = xv[i];
        if constexpr (D) term = cv[i] - term;
        if (a.src_scale) term = term * sv[u];
        if (a.w) term = term * wv[u];
        acc[i] = ok[u] ? acc[i] + term : acc[i];
      }
    }
  }
}

// Rows of at most kTableSeqMax entries: a lane group of L8 lanes owns a destination row, 8 columns and one 16-byte access
// of the bfloat16 side a lane, R8 = 64 / L8 rows a wave.  Longer rows (T only): hg_table.hip's long-row phase, word for
// word, in the float32 call's (L, R, P2) at 4 columns a lane -- the chunks [g c, (g + 1) c), the LDS layout and the tree
// are that call's, so are the bits; only the loads of the bfloat16 side are 8 bytes wide there.
template <bool T, bool D, typename ES, typename ED>
__global__ __launch_bounds__(64 * kTableWaves) void table_gather_b16_kernel(GatherB16Args<ES, ED> a) {
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int F = a.F;
  const int L8 = a.L8, R8 = a.R8;
  const int sub8 = lane / L8, cl8 = lane - sub8 * L8;
  const int64_t row0 = (int64_t)blockIdx.x * (R8 * kTableWaves);
  const int64_t row64 = row0 + w * R8 + sub8;
  const bool row_on = sub8 < R8 && row64 < a.nrows;
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
    for (int c0 = 0; c0 < F; c0 += L8 * 8) {
      const int c = c0 + cl8 * 8;
      if (c >= F) continue;
      float acc[8], cv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = 0.f, cv[i] = 0.f;
      if constexpr (D) {
        Chunk<8, ES> cc;
        cc.load(a.ctr + (size_t)row * F + c);
        cc.get(cv);
      }
      row_sum_b16<T, 8, D>(a, beg, end, c, cv, acc);
      if (a.dst_scale && end > beg) {  // an empty row stays +0.0 whatever its scale
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = ds * acc[i];
      }
      Chunk<8, ED>::store(a.dst + (size_t)row * F + c, acc);
    }
  }

  if constexpr (T) {
    __shared__ __attribute__((aligned(16))) float part[kTableWaves * 64 * 4];
    __shared__ unsigned long long long_rows[kTableWaves];
    const unsigned long long mine = __ballot(row_on && is_long && cl8 == 0);
    if (lane == 0) long_rows[w] = mine;
    __syncthreads();
    const int L = a.L, R = a.R;
    const int sub = lane / L, cl = lane - sub * L;
    const bool lane_on = sub < R;
    const int P = R * kTableWaves, g = w * R + sub;
    for (int ww = 0; ww < kTableWaves; ++ww) {
      const unsigned long long mm = long_rows[ww];
      unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)mm), hi = __builtin_amdgcn_readfirstlane((unsigned)(mm >> 32));
      unsigned long long m = ((unsigned long long)hi << 32) | lo;
      while (m) {
        const int ln = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int lrow = (int)(row0 + ww * R8 + ln / L8);
        const int lbeg = max(a.ptr_v[lrow], 0), lend = min(a.ptr_v[lrow + 1], a.entries);
        const int64_t len = lend - lbeg, chunk = (len + P - 1) / P;
        const int gb = lbeg + (int)min((int64_t)g * chunk, len), ge = lbeg + (int)min((int64_t)(g + 1) * chunk, len);
        const float ds = a.dst_scale ? a.dst_scale[lrow] : 1.f;
        for (int c0 = 0; c0 < F; c0 += L * 4) {
          const int c = c0 + cl * 4;
          const bool on = lane_on && c < F;
          float *mypart = part + (size_t)(g * L + cl) * 4;
          if (on) {
            float acc[4], cv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = 0.f, cv[i] = 0.f;
            if constexpr (D) {
              Chunk<4, ES> cc;
              cc.load(a.ctr + (size_t)lrow * F + c);
              cc.get(cv);
            }
            row_sum_b16<T, 4, D>(a, gb, ge, c, cv, acc);
#pragma unroll
            for (int i = 0; i < 4; ++i) mypart[i] = acc[i];
          }
          __syncthreads();
          for (int s = a.P2 >> 1; s >= 1; s >>= 1) {
            if (on && g < s && g + s < P) {
              const float *other = part + (size_t)((g + s) * L + cl) * 4;
#pragma unroll
              for (int i = 0; i < 4; ++i) mypart[i] = mypart[i] + other[i];
            }
            __syncthreads();
          }
          if (on && g == 0) {
            float out[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) out[i] = a.dst_scale ? ds * mypart[i] : mypart[i];
            Chunk<4, ED>::store(a.dst + (size_t)lrow * F + c, out);
          }
          __syncthreads();
        }
      }
    }
  }
}

// ---- distances and dot products -------------------------------------------------------------------------------------------

struct DistB16Args {
  const int32_t *idx;
  const bf16_t *Q, *X;
  float *dist;
  int32_t n, k, F, entries;
};

// hg_table.hip's table_dist_kernel on bfloat16 rows: one lane per table position, 8 columns a load, kTableDistLoads loads of
// each row in flight, the one fma chain in ascending c.
__global__ __launch_bounds__(kTableBlock) void table_dist_b16_kernel(DistB16Args a) {
  const int64_t p64 = (int64_t)blockIdx.x * kTableBlock + threadIdx.x;
  if (p64 >= a.entries) return;
  const int p = (int)p64, F = a.F;
  const int j = a.idx[p];
  if ((unsigned)j >= (unsigned)a.n) {  // names no row: +0.0, and nothing is read through it
    a.dist[p] = 0.f;
    return;
  }
  const bf16_t *q = a.Q + (size_t)(p / a.k) * F, *x = a.X + (size_t)j * F;
  constexpr int kStep = 8 * kTableDistLoads;
  float acc = 0.f;
  int c = 0;
  for (; c + kStep <= F; c += kStep) {
    Chunk<8, bf16_t> qc[kTableDistLoads], xc[kTableDistLoads];
#pragma unroll
    for (int u = 0; u < kTableDistLoads; ++u) {
      qc[u].load(q + c + u * 8);
      xc[u].load(x + c + u * 8);
    }
#pragma unroll
    for (int u = 0; u < kTableDistLoads; ++u) {
      float qv[8], xv[8];
      qc[u].get(qv);
      xc[u].get(xv);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = qv[i] - xv[i];
        acc = __builtin_fmaf(d, d, acc);
      }
    }
  }
  for (; c < F; c += 8) {
    Chunk<8, bf16_t> qc, xc;
    qc.load(q + c);
    xc.load(x + c);
    float qv[8], xv[8];
    qc.get(qv);
    xc.get(xv);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float d = qv[i] - xv[i];
      acc = __builtin_fmaf(d, d, acc);
    }
  }
  a.dist[p] = acc;
}

struct DotB16Args {
  const int32_t *idx;
  const bf16_t *A, *C;
  const float *a_scale, *B, *D;
  float *out;
  int32_t rows, n, k, F;
  int32_t L, R;  // lanes per table row (a power of two), rows per wave: the float32 call's at 4 columns a lane
};

// hg_table.hip's table_dot_kernel<4, TWO> with bfloat16 gathered rows A / C (8-byte loads): the DOT ORDER of include/hg_aggr.h
// fixes the lane that owns a column and the butterfly, so the geometry is the float32 call's and only the loads differ.
template <bool TWO>
__global__ __launch_bounds__(64 * kTableWaves) void table_dot_b16_kernel(DotB16Args a) {
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int L = a.L, R = a.R, F = a.F, k = a.k;
  const int sub = lane / L, cl = lane - sub * L;
  const int64_t row64 = ((int64_t)blockIdx.x * kTableWaves + w) * R + sub;
  const bool row_on = row64 < a.rows;  // a whole lane group is on or off; an off group computes row 0 and stores nothing
  const int row = row_on ? (int)row64 : 0;
  const int step = L * 4;
  const bool one_pass = F <= step;
  const int cfirst = cl * 4;
  const bool on0 = cfirst < F;
  const size_t brow = (size_t)row * F;
  Chunk<4, float> b0, d0{};
  b0.load(a.B + brow + (on0 ? cfirst : 0));
  if constexpr (TWO) d0.load(a.D + brow + (on0 ? cfirst : 0));
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
      Chunk<4, float> bc = b0, dc = d0;
      if (!one_pass && c0 > 0) {
        bc.load(a.B + brow + ce);
        if constexpr (TWO) dc.load(a.D + brow + ce);
      }
      Chunk<4, bf16_t> ac[kTableDotBatch], cc[kTableDotBatch];
#pragma unroll
      for (int u = 0; u < kTableDotBatch; ++u) {
        ac[u].load(a.A + (size_t)jv[u] * F + ce);
        if constexpr (TWO) cc[u].load(a.C + (size_t)jv[u] * F + ce);
      }
      float bv[4], dv[4] = {0.f, 0.f, 0.f, 0.f};
      bc.get(bv);
      if constexpr (TWO) dc.get(dv);
#pragma unroll
      for (int u = 0; u < kTableDotBatch; ++u) {
        float av[4], cv[4] = {0.f, 0.f, 0.f, 0.f};
        ac[u].get(av);
        if constexpr (TWO) cc[u].get(cv);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s1[u] = on ? __builtin_fmaf(av[i], bv[i], s1[u]) : s1[u];
          if constexpr (TWO) s2[u] = on ? __builtin_fmaf(cv[i], dv[i], s2[u]) : s2[u];
        }
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

// ---- the entries' refusals and launches -------------------------------------------------------------------------------------

bool aligned(const void *p, size_t a) { return (uintptr_t)p % a == 0; }

// The bf16 instances move whole 16-byte lanes: anything else is HG_ERR_UNSUPPORTED, and the caller widens
int lanes_refusal(const char *entry, int32_t F, std::initializer_list<const void *> rows) {
  if (F % 8) return fail(entry, HG_ERR_UNSUPPORTED, "the bf16 instances need F % 8 == 0, got F = " + std::to_string(F));
  for (const void *p : rows)
    if (!aligned(p, 16)) return fail(entry, HG_ERR_UNSUPPORTED, "the bf16 instances need 16-byte aligned rows");
  return HG_OK;
}

// T: through the transpose (idx null), n destination rows out of `rows` source rows; else through idx, the other way round
template <bool T, bool D, typename ES, typename ED>
int launch_gather_b16(const char *entry, const int32_t *idx, const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k,
                      int32_t n, int32_t F, const void *src, const float *w, const float *src_scale, const float *dst_scale,
                      const void *ctr, void *dst, hg_stream_t stream) {
  GatherB16Args<ES, ED> a{};
  a.idx = idx;
  a.ptr_v = ptr_v;
  a.pos_v = pos_v;
  a.src = static_cast<const ES *>(src);
  a.w = w;
  a.src_scale = src_scale;
  a.dst_scale = dst_scale;
  a.ctr = static_cast<const ES *>(ctr);
  a.dst = static_cast<ED *>(dst);
  a.nrows = T ? n : rows;
  a.nsrc = T ? rows : n;
  a.k = k;
  a.F = F;
  a.entries = rows * k;
  a.L8 = std::min(F / 8, 64);
  a.R8 = 64 / a.L8;
  a.L = std::min(F / 4, 64);  // what hg_table_gather_t_f32 computes from F for its 4-column instance
  a.R = 64 / a.L;
  a.P2 = 1;
  while (a.P2 < a.R * kTableWaves) a.P2 <<= 1;
  const int RW = a.R8 * kTableWaves;
  const dim3 grid((unsigned)(((int64_t)a.nrows + RW - 1) / RW)), block(64 * kTableWaves);
  hipLaunchKernelGGL((table_gather_b16_kernel<T, D, ES, ED>), grid, block, 0, static_cast<hipStream_t>(stream), a);
  return launch_check(entry);
}

template <bool T>
int gather_b16_entry(const char *entry, const int32_t *idx, const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k,
                     int32_t n, int32_t F, const void *src, const float *w, const float *src_scale, const float *dst_scale,
                     const void *ctr, void *dst, int32_t io, hg_stream_t stream) {
  if (T ? (!ptr_v || !pos_v) : !idx) return fail(entry, HG_ERR_INVALID, T ? "null ptr_v or pos_v" : "null idx");
  if (!src || !dst) return fail(entry, HG_ERR_INVALID, "null src or dst");
  if (const int st = size_refusal(entry, rows, k, n, F)) return st;
  if (io != HG_ROWS_SRC_BF16 && io != HG_ROWS_DST_BF16)
    return fail(entry, HG_ERR_INVALID, "io must be HG_ROWS_SRC_BF16 or HG_ROWS_DST_BF16, got " + std::to_string(io));
  if (ctr && io == HG_ROWS_DST_BF16)
    return fail(entry, HG_ERR_INVALID, "the difference form (ctr) takes HG_ROWS_SRC_BF16 only");
  for (const void *p : {(const void *)idx, (const void *)ptr_v, (const void *)pos_v, (const void *)w, (const void *)src_scale,
                        (const void *)dst_scale})
    if (!aligned(p, 4)) return fail(entry, HG_ERR_UNSUPPORTED, "the table, w and the scales must be 4-byte aligned");
  const bool sb = io == HG_ROWS_SRC_BF16;
  if (!aligned(src, sb ? 2 : 4) || !aligned(dst, sb ? 4 : 2) || !aligned(ctr, 2))
    return fail(entry, HG_ERR_UNSUPPORTED, "bfloat16 rows must be 2-byte aligned, float32 rows 4-byte aligned");
  if (const int st = lanes_refusal(entry, F, {src, ctr, (const void *)dst})) return st;
  if (!sb) return launch_gather_b16<T, false, float, bf16_t>(entry, idx, ptr_v, pos_v, rows, k, n, F, src, w, src_scale, dst_scale, nullptr, dst, stream);
  if (ctr) return launch_gather_b16<T, true, bf16_t, float>(entry, idx, ptr_v, pos_v, rows, k, n, F, src, w, src_scale, dst_scale, ctr, dst, stream);
  return launch_gather_b16<T, false, bf16_t, float>(entry, idx, ptr_v, pos_v, rows, k, n, F, src, w, src_scale, dst_scale, nullptr, dst, stream);
}

}  // namespace
}  // namespace hg

extern "C" {

int hg_table_gather_bf16(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, const void *src, const float *w,
                         const float *src_scale, const float *dst_scale, const void *ctr, void *dst, int32_t io,
                         hg_stream_t stream) {
  return hg::gather_b16_entry<false>("hg_table_gather_bf16", idx, nullptr, nullptr, rows, k, n, F, src, w, src_scale, dst_scale, ctr,
                                     dst, io, stream);
}

int hg_table_gather_t_bf16(const int32_t *ptr_v, const int32_t *pos_v, int32_t rows, int32_t k, int32_t n, int32_t F,
                           const void *src, const float *w, const float *src_scale, const float *dst_scale, const void *ctr,
                           void *dst, int32_t io, hg_stream_t stream) {
  return hg::gather_b16_entry<true>("hg_table_gather_t_bf16", nullptr, ptr_v, pos_v, rows, k, n, F, src, w, src_scale, dst_scale, ctr,
                                    dst, io, stream);
}

int hg_table_dist_bf16(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, const uint16_t *Q, const uint16_t *X,
                       float *dist, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_dist_bf16";
  if (!idx || !Q || !X || !dist) return fail(entry, HG_ERR_INVALID, "null idx, Q, X or dist");
  if (const int st = size_refusal(entry, rows, k, n, F)) return st;
  if (!aligned(idx, 4) || !aligned(dist, 4) || !aligned(Q, 2) || !aligned(X, 2))
    return fail(entry, HG_ERR_UNSUPPORTED, "idx and dist must be 4-byte aligned, Q and X 2-byte aligned");
  if (const int st = lanes_refusal(entry, F, {Q, X})) return st;
  DistB16Args a{};
  a.idx = idx;
  a.Q = Q;
  a.X = X;
  a.dist = dist;
  a.n = n;
  a.k = k;
  a.F = F;
  a.entries = rows * k;
  const dim3 grid((unsigned)(((int64_t)a.entries + kTableBlock - 1) / kTableBlock)), block(kTableBlock);
  hipLaunchKernelGGL(table_dist_b16_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return launch_check(entry);
}

int hg_table_dot_bf16(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t F, const uint16_t *A, const float *a_scale,
                      const float *B, const uint16_t *C, const float *D, float *out, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_dot_bf16";
  if (!idx) return fail(entry, HG_ERR_INVALID, "null idx");
  if (!A || !B || !out) return fail(entry, HG_ERR_INVALID, "null A, B or out");
  if (!C != !D) return fail(entry, HG_ERR_INVALID, "C and D must both be given or both be null");
  if (const int st = size_refusal(entry, rows, k, n, F)) return st;
  for (const void *p : {(const void *)idx, (const void *)a_scale, (const void *)B, (const void *)D, (const void *)out})
    if (!aligned(p, 4)) return fail(entry, HG_ERR_UNSUPPORTED, "idx, a_scale, B, D and out must be 4-byte aligned");
  if (!aligned(A, 2) || !aligned(C, 2)) return fail(entry, HG_ERR_UNSUPPORTED, "A and C must be 2-byte aligned");
  if (const int st = lanes_refusal(entry, F, {A, B, C, D})) return st;
  DotB16Args a{};
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
  a.L = 1;
  while (a.L < std::min(F / 4, 64)) a.L <<= 1;  // hg_table_dot_f32's L at 4 columns a lane
  a.R = 64 / a.L;
  const int RW = a.R * kTableWaves;
  const dim3 grid((unsigned)(((int64_t)rows + RW - 1) / RW)), block(64 * kTableWaves);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (C) hipLaunchKernelGGL(table_dot_b16_kernel<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(table_dot_b16_kernel<false>, grid, block, 0, s, a);
  return launch_check(entry);
}

}  // extern "C"
