// gfx950 (MI355X, CDNA4) kernels of libhgaggr: the two hops of the fused
// vertex -> hyperedge -> vertex aggregation as atomic-free row gathers, plus the
// reference-style register-fused push kernel with fp32 atomics.
//
// Layout: a feature row of F floats is spread over LPR consecutive lanes (VEC
// floats each), so a 64-lane wavefront holds G = 64/LPR rows at once and every
// row access is one contiguous LPR*VEC*4-byte segment (F = 32: 8 lanes x
// dwordx4 = one 128-byte line per row, 8 rows per wave instruction).
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "hg_attention.h"  // kSegLong: the row length at which a hyperedge leaves the lane groups (hyperedge_dot_kernel)
#include "hg_kernels.h"

namespace hg {

// Waves per SIMD linear_rows_kernel is compiled for at K <= 64 (tools/linear_probe.py, 2.77 M rows): 64 x 64: 8 waves
// 0.550 ms (spills; rocBLAS 0.427), 7 0.315, 6 0.311; 32 x 32: 8 waves 0.147, 7 0.141, 6 0.149.
constexpr int kRowsWaves = 7;
// Rows of Y leave the panel kernel with the streaming (nt) hint where a row is whole 64-byte units (F % 16 == 0: the
// host sets FusedArgs::y_nt / GatherArgs::nt_dst / StreamArgs::nt_dst): +3..8 % there, F = 16 0.45 -> 0.72 of the
// roofline; rows that end inside a 64-byte unit (F = 4 .. 28, 33) lose 7-50 % with it -- the L2 merges their partial
// lines only on the plain write-back path (profiles/r03_experiments.md; script removed, see git history).
template <int VEC> struct Vec;
template <> struct Vec<1> {
  float x;
  __device__ __forceinline__ static Vec zero() { return Vec{0.f}; }
  __device__ __forceinline__ static Vec load(const float *p) { return Vec{*p}; }
  __device__ __forceinline__ static Vec load_buf(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return Vec{__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0))};
  }
  __device__ __forceinline__ static Vec loadu(const float *p) { return Vec{*p}; }
  __device__ __forceinline__ void store(float *p) const { *p = x; }
  __device__ __forceinline__ void store_n(float *p, int) const { *p = x; }
  __device__ __forceinline__ void store_n_nt(float *p, int) const { __builtin_nontemporal_store(x, p); }
  __device__ __forceinline__ void add(const Vec &o) { x += o.x; }
  __device__ __forceinline__ void fma(const Vec &o, float s) { x = __builtin_fmaf(o.x, s, x); }  // += o * s, one rounding
  __device__ __forceinline__ void mul(float s) { x *= s; }
  __device__ __forceinline__ void xor_reduce(int off) { x += __shfl_xor(x, off, 64); }
};
template <> struct Vec<4> {
  float4 v;
  __device__ __forceinline__ static Vec zero() { return Vec{make_float4(0.f, 0.f, 0.f, 0.f)}; }
  __device__ __forceinline__ static Vec load(const float *p) {
    return Vec{*reinterpret_cast<const float4 *>(p)};
  }
  __device__ __forceinline__ static Vec load_buf(__amdgpu_buffer_rsrc_t r, unsigned off) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    return Vec{__builtin_bit_cast(float4, (u4)__builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0))};
  }
  __device__ __forceinline__ void store(float *p) const { *reinterpret_cast<float4 *>(p) = v; }
  // Rows whose width is not a multiple of four floats (or whose base is only 4-byte aligned) still move as
  // 16-byte accesses: gfx950 takes dword-aligned dwordx4 loads and stores, the lane that holds a row's last
  // columns stores only those (store_n), and what it loaded past the row's end stays in columns nobody reads.
  typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
  __device__ __forceinline__ static Vec loadu(const float *p) {
    const f4u t = *reinterpret_cast<const f4u *>(p);
    return Vec{make_float4(t.x, t.y, t.z, t.w)};
  }
  __device__ __forceinline__ void storeu(float *p) const { *reinterpret_cast<f4u *>(p) = f4u{v.x, v.y, v.z, v.w}; }
  __device__ __forceinline__ void store_n(float *p, int n) const {  // n >= 1 columns of this lane exist
    if (n >= 4) {
      storeu(p);
    } else {
      p[0] = v.x;
      if (n > 1) p[1] = v.y;
      if (n > 2) p[2] = v.z;
    }
  }
  __device__ __forceinline__ void store_nt(float *p) const {
    typedef float f4 __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(f4{v.x, v.y, v.z, v.w}, reinterpret_cast<f4 *>(p));
  }
  // store_n with the streaming hint (global_store_dwordx4 ... nt): rows of Y, which nothing reads again in this launch
  __device__ __forceinline__ void store_n_nt(float *p, int n) const {
    if (n >= 4) {
      __builtin_nontemporal_store(f4u{v.x, v.y, v.z, v.w}, reinterpret_cast<f4u *>(p));
    } else {
      __builtin_nontemporal_store(v.x, p);
      if (n > 1) __builtin_nontemporal_store(v.y, p + 1);
      if (n > 2) __builtin_nontemporal_store(v.z, p + 2);
    }
  }
  __device__ __forceinline__ void add(const Vec &o) {
    v.x += o.v.x; v.y += o.v.y; v.z += o.v.z; v.w += o.v.w;
  }
  __device__ __forceinline__ void fma(const Vec &o, float s) {
    v.x = __builtin_fmaf(o.v.x, s, v.x); v.y = __builtin_fmaf(o.v.y, s, v.y);
    v.z = __builtin_fmaf(o.v.z, s, v.z); v.w = __builtin_fmaf(o.v.w, s, v.w);
  }
  __device__ __forceinline__ void mul(float s) { v.x *= s; v.y *= s; v.z *= s; v.w *= s; }
  __device__ __forceinline__ void xor_reduce(int off) {
    v.x += __shfl_xor(v.x, off, 64); v.y += __shfl_xor(v.y, off, 64);
    v.z += __shfl_xor(v.z, off, 64); v.w += __shfl_xor(v.w, off, 64);
  }
};

// Rows of X and Y in memory, element type T, as the fp32 lanes above.  fp32 rows move through Vec's own accesses.  bf16 rows
// keep the fp32 lane layout -- a VEC = 4 lane still holds four columns, so it moves 8 bytes (buffer_load_dwordx2, an 8-byte
// store) -- and every lane group, tile row and reduction step stays where the fp32 instance has it: same sums, same order.
// Widening is a 16-bit shift (exact); narrowing is the plain cast, v_cvt_pk_bf16_f32 (round to nearest even, NaN stays NaN).
// Only VEC = 4 exists for bf16: a bf16 call has F % 4 == 0 and 8-byte aligned rows (hg_aggr_fused_bf16).
template <typename T, int VEC> struct Rows {
  using V = Vec<VEC>;
  __device__ __forceinline__ static V load(const float *p) { return V::load(p); }
  __device__ __forceinline__ static V load_buf(__amdgpu_buffer_rsrc_t r, unsigned off) { return V::load_buf(r, off); }
  __device__ __forceinline__ static void store(const V &v, float *p) { v.store(p); }
  __device__ __forceinline__ static void store_n(const V &v, float *p, int n) { v.store_n(p, n); }
  __device__ __forceinline__ static void store_n_nt(const V &v, float *p, int n) { v.store_n_nt(p, n); }
};
template <> struct Rows<bf16, 4> {
  using V = Vec<4>;
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  __device__ __forceinline__ static V widen(u2 u) {
    return V{make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                         __uint_as_float(u.y & 0xffff0000u))};
  }
  __device__ __forceinline__ static unsigned pack(float lo, float hi) {
    return (unsigned)__builtin_bit_cast(uint16_t, (__bf16)lo) | ((unsigned)__builtin_bit_cast(uint16_t, (__bf16)hi) << 16);
  }
  __device__ __forceinline__ static u2 narrow(const V &v) { return u2{pack(v.v.x, v.v.y), pack(v.v.z, v.v.w)}; }
  __device__ __forceinline__ static V load(const bf16 *p) { return widen(*reinterpret_cast<const u2 *>(p)); }
  __device__ __forceinline__ static V load_buf(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return widen(__builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
  }
  __device__ __forceinline__ static void store(const V &v, bf16 *p) { *reinterpret_cast<u2 *>(p) = narrow(v); }
  __device__ __forceinline__ static void store_n(const V &v, bf16 *p, int) { store(v, p); }  // whole lanes: F % 4 == 0
  __device__ __forceinline__ static void store_n_nt(const V &v, bf16 *p, int) {
    __builtin_nontemporal_store(narrow(v), reinterpret_cast<u2 *>(p));
  }
};

// The attention coefficient of one gathered entry for the lane's head (gather_rows_kernel's WA instances): the scores of
// the row and of the entry in the order the segment softmax adds them -- the segment's own end first, taken as 0 where
// absent; the other end absent: no addition -- then attention_weight.
__device__ __forceinline__ float attn_weight(const AttnGatherArgs &a, float row_s, float ent_s, float seg_max, float seg_inv) {
  return a.stat_row ? attention_weight(row_s, ent_s, a.ent_score != nullptr, a.slope, seg_max, seg_inv)
                    : attention_weight(ent_s, row_s, a.row_score != nullptr, a.slope, seg_max, seg_inv);
}

// dst[r,:] = scaleB[r] * (scaleA[r] * sum_{p in row r} src[ind[p],:])
//
// Workgroups [0, n_task_blocks) run wave tasks (one long-row slice per wave, its
// entries strided over the wave's G row groups, then a cross-group shuffle
// reduction).  The remaining workgroups each own one row panel: the panel's
// row pointers, row scales and index slice are staged into LDS with coalesced
// loads, then every LPR-lane group walks a contiguous run of the panel's rows as
// one flat entry stream, U row loads in flight, adding in CSR order (so short
// rows reproduce the CPU reference's summation order exactly).  TS / TD: element types of src / dst rows (Rows).
// WT: per-entry weights (WeightedGatherArgs, hg_aggr_incidence_f32): the same walk, each gathered row added as
// acc = fma(row, weight, acc).  Wave tasks load the weight beside the index; panels stage the weights in LDS after
// sind (launch_gather_t sizes those instances' LDS for it).  Partial rows leave already weighted: fixups are unchanged.
// WH: a weight per entry and head (HeadsGatherArgs, hg_aggr_incidence_heads_f32): w is [nnz, H], head fastest, and head h
// owns columns h * C .. (h + 1) * C - 1 of the rows; a lane multiplies its columns by the weight of the head that owns them, taken from the
// lane's absolute column (a column tile may begin inside a head), acc = fma(row, w[pos * H + col / C], acc).  A 16-byte lane
// lies inside one head (the launcher takes VEC = 4 only where C % 4 == 0).  The weights are read where they lie, beside the
// row they scale (4 H contiguous bytes per entry, shared by the lanes of a row); panels stage the entries' positions
// (hop 2: perm) where the WT instances stage the weights, so the LDS does not grow with H.
// WA: the WH walk with the weight formed in the lane (AttnGatherArgs, hg_aggr_incidence_attention_heads_f32): the
// attention coefficient of the entry and the lane's head from the two ends' scores and the segment's statistics,
// attention_weight (hg_attention.h) -- the bits kSegSoftmax writes, so the sums are those of the WH instance on alpha.  What
// belongs to the destination row (its score, and the statistics where the row is the segment) is read once per row: a
// wave task's lanes hold it in registers, a panel stages its rows' [nrows, H] slices behind sind; what belongs to the entry
// is gathered beside the row it weighs.  No weight array, no positions, no perm.
template <bool WT, bool WH, bool WA = false>
using GatherArgsOf =
    std::conditional_t<WA, AttnGatherArgs, std::conditional_t<WH, HeadsGatherArgs, std::conditional_t<WT, WeightedGatherArgs, GatherArgs>>>;
template <int LPR, int VEC, typename TS = float, typename TD = float, bool WT = false, bool WH = false, bool WA = false>
__global__ __launch_bounds__(256) void gather_rows_kernel(const GatherArgsOf<WT, WH, WA> a) {
  static_assert(!(WT && WH) && !(WA && (WT || WH)), "per-entry, per-head or computed weights");
  constexpr int U = 4;           // row loads in flight per lane (8, or two batches in flight: within 3 %, profiles/r01_fused_experiments.md)
  constexpr int G = 64 / LPR;    // row groups per wave
  constexpr int NG = 256 / LPR;  // row groups per workgroup
  using V = Vec<VEC>;
  using RS = Rows<TS, VEC>;
  using RD = Rows<TD, VEC>;
  extern __shared__ int32_t smem[];
  const TS *src = static_cast<const TS *>(a.src);
  TD *dst = static_cast<TD *>(a.dst);

  const int tid = threadIdx.x;
  const int gl = tid & (LPR - 1);
  const int col = (blockIdx.y * LPR + gl) * VEC;
  const bool col_ok = col < a.F;
  const int64_t F = a.F;
  int b = blockIdx.x;
  int hd = 0;  // the head of this lane's columns
  if constexpr (WH || WA) hd = col_ok ? col / a.C : 0;

  if (b < a.n_task_blocks) {
    const int t = __builtin_amdgcn_readfirstlane(b * 4 + (tid >> 6));
    if (t >= a.ntasks) return;
    const Task tk = a.tasks[t];
    const int g = (tid & 63) / LPR;
    V acc = V::zero();
    float rs = 0.f, rm = 0.f, ri = 0.f;  // WA: the row's score and, where the row is the segment, its statistics
    if constexpr (WA) {
      const int64_t rh = (int64_t)tk.row * a.heads + hd;
      if (a.row_score) rs = a.row_score[rh];
      if (a.stat_row) rm = a.seg_max[rh], ri = a.seg_inv[rh];
    }
    for (int p = tk.beg + g; p < tk.end; p += G * U) {
      V v[U];
      float wv[U];
      float es[WA ? U : 1], em[WA ? U : 1], ei[WA ? U : 1];  // WA: the entries' scores and statistics
#pragma unroll
      for (int k = 0; k < U; k++) {
        const int q = p + k * G;
        const bool ok = col_ok && q < tk.end;
        const int64_t idx = ok ? a.ind[q] : 0;
        if constexpr (WT) wv[k] = ok ? a.w[a.wperm ? a.wperm[q] : q] : 0.f;
        if constexpr (WH) wv[k] = ok ? a.w[(int64_t)(a.wperm ? a.wperm[q] : q) * a.heads + hd] : 0.f;
        if constexpr (WA) {
          const int64_t eh = idx * a.heads + hd;
          es[k] = (ok && a.ent_score) ? a.ent_score[eh] : 0.f;
          em[k] = (ok && !a.stat_row) ? a.seg_max[eh] : rm;
          ei[k] = (ok && !a.stat_row) ? a.seg_inv[eh] : ri;
        }
        v[k] = ok ? RS::load(src + idx * F + col) : V::zero();
      }
#pragma unroll
      for (int k = 0; k < U; k++) {
        if constexpr (WA) {
          const bool ok = col_ok && p + k * G < tk.end;
          wv[k] = ok ? attn_weight(a, rs, es[k], em[k], ei[k]) : 0.f;
        }
        if constexpr (WT || WH || WA) acc.fma(v[k], wv[k]);
        else acc.add(v[k]);
      }
    }
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1) acc.xor_reduce(off);
    if (g == 0 && col_ok) {
      if (tk.slot < 0) {
        const int srow = a.scale_map ? a.scale_map[tk.row] : tk.row;
        const int64_t drow = a.dst_map ? a.dst_map[tk.row] : tk.row;
        if (a.scaleA) acc.mul(a.scaleA[srow]);
        if (a.scaleB) acc.mul(a.scaleB[srow]);
        if (a.nt_dst) RD::store_n_nt(acc, dst + drow * F + col, VEC);
        else RD::store(acc, dst + drow * F + col);
      } else {
        acc.store(a.partial + (int64_t)tk.slot * F + col);
      }
    }
    return;
  }

  b -= a.n_task_blocks;
  if (a.xcd_remap) {
    // workgroups are dealt round-robin to the 8 XCDs; give each XCD one
    // contiguous run of panels so neighbouring panels share an L2
    const int x = b & 7, i = b >> 3;
    const int cpx = a.npanels >> 3, rem = a.npanels & 7;
    b = x * cpx + (x < rem ? x : rem) + i;
  }
  const Panel pn = a.panels[b];
  int32_t *sptr = smem;                                         // [panel_rows + 1]
  float *sA = reinterpret_cast<float *>(smem + a.panel_rows + 1);  // [panel_rows]
  float *sB = sA + a.panel_rows;                                // [panel_rows]
  int32_t *sdst = reinterpret_cast<int32_t *>(sB + a.panel_rows);  // [panel_rows]
  int32_t *sind = sdst + a.panel_rows;                             // [panel_nnz]

  for (int i = tid; i <= pn.nrows; i += 256) sptr[i] = a.ptr[pn.row0 + i] - pn.nnz0;
  for (int i = tid; i < pn.nrows; i += 256) {
    const int srow = a.scale_map ? a.scale_map[pn.row0 + i] : pn.row0 + i;
    if (a.scaleA) sA[i] = a.scaleA[srow];
    if (a.scaleB) sB[i] = a.scaleB[srow];
    if (a.dst_map) sdst[i] = a.dst_map[pn.row0 + i];
  }
  for (int i = tid; i < pn.nnz_cnt; i += 256) sind[i] = a.ind[pn.nnz0 + i];
  float *sw = reinterpret_cast<float *>(sind + a.panel_nnz);  // [panel_nnz], WT instances only
  if constexpr (WT) {
    for (int i = tid; i < pn.nnz_cnt; i += 256) {
      const int q = pn.nnz0 + i;
      sw[i] = a.w[a.wperm ? a.wperm[q] : q];
    }
  }
  const int32_t *swp = reinterpret_cast<const int32_t *>(sw);  // WH: the entries' positions in w, where perm gives them
  if constexpr (WH) {
    if (a.wperm)
      for (int i = tid; i < pn.nnz_cnt; i += 256) reinterpret_cast<int32_t *>(sw)[i] = a.wperm[pn.nnz0 + i];
  }
  // WA: the rows' scores [panel_rows, heads] and, where the rows are the segments, their statistics behind them: a panel's
  // rows are consecutive, so each is one contiguous slice of its [rows, heads] array
  float *srs = sw, *srm = sw, *sri = sw;
  if constexpr (WA) {
    srm = srs + (int64_t)a.panel_rows * a.heads;
    sri = srm + (int64_t)a.panel_rows * a.heads;
    const int64_t r0 = (int64_t)pn.row0 * a.heads;
    const int nrh = pn.nrows * a.heads;
    if (a.row_score)
      for (int i = tid; i < nrh; i += 256) srs[i] = a.row_score[r0 + i];
    if (a.stat_row)
      for (int i = tid; i < nrh; i += 256) {
        srm[i] = a.seg_max[r0 + i];
        sri[i] = a.seg_inv[r0 + i];
      }
  }
  __syncthreads();

  const int g = tid / LPR;
  const int rpg = (pn.nrows + NG - 1) / NG;
  int r = min(g * rpg, pn.nrows);
  const int re = min(r + rpg, pn.nrows);
  if (r >= re) return;

  auto flush = [&](int row, V acc) {
    if (sptr[row + 1] > sptr[row]) {  // an empty row stays exactly 0 (degE may be inf)
      if (a.scaleA) acc.mul(sA[row]);
      if (a.scaleB) acc.mul(sB[row]);
    }
    const int64_t drow = a.dst_map ? sdst[row] : pn.row0 + row;
    if (col_ok) {
      if (a.nt_dst) RD::store_n_nt(acc, dst + drow * F + col, VEC);
      else RD::store(acc, dst + drow * F + col);
    }
  };

  int pos = sptr[r];
  const int stop = sptr[re];
  int row_end = sptr[r + 1];
  V acc = V::zero();

  float wv[WH ? U : 1];  // WH: the weights of the rows in flight
  float es[WA ? U : 1], em[WA ? U : 1], ei[WA ? U : 1];  // WA: their entries' scores and statistics
  float rs = 0.f, rm = 0.f, ri = 0.f;                    // WA: what row r itself contributes, read when r changes
  auto load_row = [&](int row) {
    if constexpr (WA) {
      if (a.row_score) rs = srs[row * a.heads + hd];
      if (a.stat_row) rm = srm[row * a.heads + hd], ri = sri[row * a.heads + hd];
    }
  };
  if constexpr (WA) load_row(r);
  auto issue = [&](int p0, int n, V(&v)[U]) {
#pragma unroll
    for (int k = 0; k < U; k++) {
      const int64_t idx = sind[p0 + min(k, n - 1)];
      if constexpr (WH) {
        const int64_t wp = a.wperm ? swp[p0 + min(k, n - 1)] : pn.nnz0 + p0 + min(k, n - 1);
        wv[k] = col_ok ? a.w[wp * a.heads + hd] : 0.f;
      }
      if constexpr (WA) {
        const int64_t eh = idx * a.heads + hd;
        es[k] = (col_ok && a.ent_score) ? a.ent_score[eh] : 0.f;
        em[k] = (col_ok && !a.stat_row) ? a.seg_max[eh] : 0.f;
        ei[k] = (col_ok && !a.stat_row) ? a.seg_inv[eh] : 0.f;
      }
      v[k] = col_ok ? RS::load(src + idx * F + col) : V::zero();
    }
  };
  auto consume = [&](int p0, int n, const V(&v)[U]) {
#pragma unroll
    for (int k = 0; k < U; k++) {
      if (k < n) {
        while (row_end <= p0 + k) {
          flush(r, acc);
          acc = V::zero();
          r++;
          row_end = sptr[r + 1];
          if constexpr (WA) load_row(r);
        }
        if constexpr (WT) acc.fma(v[k], sw[p0 + k]);
        else if constexpr (WH) acc.fma(v[k], wv[k]);
        else if constexpr (WA)
          acc.fma(v[k], col_ok ? attn_weight(a, rs, es[k], a.stat_row ? rm : em[k], a.stat_row ? ri : ei[k]) : 0.f);
        else acc.add(v[k]);
      }
    }
  };

  while (pos < stop) {
    const int n = min(U, stop - pos);
    V v[U];
    issue(pos, n, v);
    consume(pos, n, v);
    pos += n;
  }
  while (r < re) {
    flush(r, acc);
    acc = V::zero();
    r++;
  }
}

// out[row,:] = scaleB * (scaleA * sum_k partial[first+k,:]), slots in order; a first-level
// fixup (pad > 0) leaves its unscaled sum in partial[pad-1] for the final one.  TD: element type of dst rows.
template <int LPR, int VEC, typename TD = float>
__global__ __launch_bounds__(256) void fixup_rows_kernel(const GatherArgs a, const Fixup *fixups,
                                                         int nfix) {
  using V = Vec<VEC>;
  using RD = Rows<TD, VEC>;
  const int tid = threadIdx.x;
  const int gl = tid & (LPR - 1);
  const int col = (blockIdx.y * LPR + gl) * VEC;
  const int f = blockIdx.x * (256 / LPR) + tid / LPR;
  if (f >= nfix || col >= a.F) return;
  const Fixup fx = fixups[f];
  const int64_t F = a.F;
  const float *src = a.partial + (int64_t)fx.first * F + col;
  V acc = V::zero();
  int k = 0;
  for (; k + 4 <= fx.count; k += 4) {  // four slot loads in flight, added in slot order
    V v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = V::loadu(src + (int64_t)(k + j) * F);
#pragma unroll
    for (int j = 0; j < 4; j++) acc.add(v[j]);
  }
  for (; k < fx.count; k++) acc.add(V::loadu(src + (int64_t)k * F));
  if (fx.pad > 0) {
    acc.store_n(a.partial + (int64_t)(fx.pad - 1) * F + col, a.F - col);
    return;
  }
  const int srow = a.scale_map ? a.scale_map[fx.row] : fx.row;
  const int64_t drow = a.dst_map ? a.dst_map[fx.row] : fx.row;
  if (a.scaleA) acc.mul(a.scaleA[srow]);
  if (a.scaleB) acc.mul(a.scaleB[srow]);
  TD *dst = static_cast<TD *>(a.dst);
  if (a.nt_dst) RD::store_n_nt(acc, dst + drow * F + col, a.F - col);
  else RD::store_n(acc, dst + drow * F + col, a.F - col);
}

// ---- comparison reductions in the row gather and their select-gather backward ------------------------------------------
// gather_rows_reduce_kernel is gather_rows_kernel's schedule -- the same panels, wave tasks, partial slots and LDS carve-up
// (the WH instances': an entry's position where those keep its weight's) -- with another reducer.  RMODE 1 / 2 (max / min,
// hg_gather_rows_reduce_f32): a lane carries, per column, the winning value and the winner's position in indices_t (an
// entry's own index on H_T, perm[index] on H), from (-inf / +inf, kNoPos).  An entry (x, p) replaces (v, q) where x > v
// (x < v), or x == v and p < q: -0.0 ties +0.0, the smallest position wins a tie, and an entry of -inf beats the start
// because any position is below kNoPos -- a non-empty row always has a winner.  The order is total, so the lane's walk, the
// butterfly over a wave task's row groups and the fixups over partial slots give the same winner in whatever order they
// meet the entries: every schedule writes the same bits.  The value is never computed with, only copied, then scaled as the
// sum is: dst = (src[ind[p*]] * scaleA) * scaleB, arg = p*; an empty row gets +0.0 and -1, no scale.  NaN: unspecified.
// RMODE 3 (select, hg_gather_rows_select_f32): the sum gather over the other hop's CSR with a select per column, src = gs
// and arg_in = the forward's arg, acc += (arg_in[ind[q], c] == pos(q)) ? gs[ind[q], c] : 0, gs and arg loaded side by side:
// the sum gather's order of addition, float partial slots, fixup_rows_kernel.
constexpr int32_t kNoPos = 0x7fffffff;
template <bool MAX> __device__ __forceinline__ bool beats(float x, int32_t p, float v, int32_t q) {
  return (MAX ? x > v : x < v) || (x == v && p < q);
}
template <int VEC> struct Lane;  // a lane's VEC columns as arrays, floats and int32 positions
template <> struct Lane<1> {
  __device__ __forceinline__ static void unpack(const Vec<1> &v, float (&f)[1]) { f[0] = v.x; }
  __device__ __forceinline__ static Vec<1> pack(const float (&f)[1]) { return Vec<1>{f[0]}; }
  __device__ __forceinline__ static void iload(const int32_t *p, int32_t (&o)[1]) { o[0] = *p; }
  __device__ __forceinline__ static void istore(int32_t *p, const int32_t (&o)[1]) { *p = o[0]; }
};
template <> struct Lane<4> {
  __device__ __forceinline__ static void unpack(const Vec<4> &v, float (&f)[4]) {
    f[0] = v.v.x, f[1] = v.v.y, f[2] = v.v.z, f[3] = v.v.w;
  }
  __device__ __forceinline__ static Vec<4> pack(const float (&f)[4]) { return Vec<4>{make_float4(f[0], f[1], f[2], f[3])}; }
  __device__ __forceinline__ static void iload(const int32_t *p, int32_t (&o)[4]) {
    const int4 t = *reinterpret_cast<const int4 *>(p);
    o[0] = t.x, o[1] = t.y, o[2] = t.z, o[3] = t.w;
  }
  __device__ __forceinline__ static void istore(int32_t *p, const int32_t (&o)[4]) {
    *reinterpret_cast<int4 *>(p) = make_int4(o[0], o[1], o[2], o[3]);
  }
};

template <int LPR, int VEC, int RMODE>
__global__ __launch_bounds__(256) void gather_rows_reduce_kernel(const ReduceGatherArgs a) {
  static_assert(RMODE >= 1 && RMODE <= 3, "max, min or select");
  constexpr bool SEL = RMODE == 3, MAX = RMODE == 1;
  constexpr int U = 4;
  constexpr int G = 64 / LPR;
  constexpr int NG = 256 / LPR;
  using V = Vec<VEC>;
  using L = Lane<VEC>;
  extern __shared__ int32_t smem[];
  const float *src = static_cast<const float *>(a.src);
  float *dst = static_cast<float *>(a.dst);

  const int tid = threadIdx.x;
  const int gl = tid & (LPR - 1);
  const int col = (blockIdx.y * LPR + gl) * VEC;
  const bool col_ok = col < a.F;
  const int64_t F = a.F;
  int b = blockIdx.x;

  float bv[VEC];    // max / min: the winner so far
  int32_t bp[VEC];  // and its position
  V acc;            // select: the sum so far
  auto reset = [&]() {
#pragma unroll
    for (int i = 0; i < VEC; i++) bv[i] = MAX ? -__builtin_inff() : __builtin_inff(), bp[i] = kNoPos;
    acc = V::zero();
  };
  // one gathered entry: its row (of src, or of gs), its position, and for the select the forward's arg row
  auto take = [&](const V &v, const int32_t (&ar)[VEC], int32_t pos, bool ok) {
    float f[VEC];
    L::unpack(v, f);
    if constexpr (SEL) {
#pragma unroll
      for (int i = 0; i < VEC; i++) f[i] = (ok && ar[i] == pos) ? f[i] : 0.f;
      acc.add(L::pack(f));
    } else {
#pragma unroll
      for (int i = 0; i < VEC; i++)
        if (ok && beats<MAX>(f[i], pos, bv[i], bp[i])) bv[i] = f[i], bp[i] = pos;
    }
  };
  // a finished row: scaled value and winner (an empty row: +0.0 and -1, no scale), or the selected sum
  auto store_row = [&](int64_t drow, float sa, float sb) {
    if constexpr (SEL) {
      acc.store(dst + drow * F + col);
    } else {
      float f[VEC];
      int32_t o[VEC];
#pragma unroll
      for (int i = 0; i < VEC; i++) {
        const bool any = bp[i] != kNoPos;
        f[i] = any ? (bv[i] * sa) * sb : 0.f;
        o[i] = any ? bp[i] : -1;
      }
      L::pack(f).store(dst + drow * F + col);
      L::istore(a.arg_out + drow * F + col, o);
    }
  };
  reset();

  if (b < a.n_task_blocks) {
    const int t = __builtin_amdgcn_readfirstlane(b * 4 + (tid >> 6));
    if (t >= a.ntasks) return;
    const Task tk = a.tasks[t];
    const int g = (tid & 63) / LPR;
    for (int p = tk.beg + g; p < tk.end; p += G * U) {
      V v[U];
      int32_t ar[U][VEC], ps[U];
#pragma unroll
      for (int k = 0; k < U; k++) {
        const int q = p + k * G;
        const bool ok = col_ok && q < tk.end;
        const int64_t idx = ok ? a.ind[q] : 0;
        ps[k] = ok ? (a.pperm ? a.pperm[q] : q) : kNoPos;
        v[k] = ok ? V::load(src + idx * F + col) : V::zero();
#pragma unroll
        for (int i = 0; i < VEC; i++) ar[k][i] = -1;
        if constexpr (SEL) {
          if (ok) L::iload(a.arg_in + idx * F + col, ar[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < U; k++) take(v[k], ar[k], ps[k], ps[k] != kNoPos);
    }
    // across the row groups: the select adds as the sum gather does; max / min combine (value, position) by the same rule
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1) {
      if constexpr (SEL) {
        acc.xor_reduce(off);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; i++) {
          const float ov = __shfl_xor(bv[i], off, 64);
          const int32_t op = __shfl_xor(bp[i], off, 64);
          if (beats<MAX>(ov, op, bv[i], bp[i])) bv[i] = ov, bp[i] = op;
        }
      }
    }
    if (g == 0 && col_ok) {
      if (tk.slot < 0) {
        store_row(tk.row, a.scaleA ? a.scaleA[tk.row] : 1.f, a.scaleB ? a.scaleB[tk.row] : 1.f);
      } else if constexpr (SEL) {
        acc.store(a.partial + (int64_t)tk.slot * F + col);
      } else {
        L::pack(bv).store(a.partial + (int64_t)tk.slot * F + col);
        L::istore(a.ipartial + (int64_t)tk.slot * F + col, bp);
      }
    }
    return;
  }

  b -= a.n_task_blocks;
  if (a.xcd_remap) {  // as gather_rows_kernel: each XCD one contiguous run of panels
    const int x = b & 7, i = b >> 3;
    const int cpx = a.npanels >> 3, rem = a.npanels & 7;
    b = x * cpx + (x < rem ? x : rem) + i;
  }
  const Panel pn = a.panels[b];
  int32_t *sptr = smem;                                            // [panel_rows + 1]
  float *sA = reinterpret_cast<float *>(smem + a.panel_rows + 1);  // [panel_rows]
  float *sB = sA + a.panel_rows;                                   // [panel_rows]
  int32_t *sind = reinterpret_cast<int32_t *>(sB + 2 * a.panel_rows);  // [panel_nnz] (gather_rows_kernel's layout)
  int32_t *spos = sind + a.panel_nnz;                              // [panel_nnz]: the entries' positions, where perm gives them

  for (int i = tid; i <= pn.nrows; i += 256) sptr[i] = a.ptr[pn.row0 + i] - pn.nnz0;
  for (int i = tid; i < pn.nrows; i += 256) {
    sA[i] = a.scaleA ? a.scaleA[pn.row0 + i] : 1.f;
    sB[i] = a.scaleB ? a.scaleB[pn.row0 + i] : 1.f;
  }
  for (int i = tid; i < pn.nnz_cnt; i += 256) sind[i] = a.ind[pn.nnz0 + i];
  if (a.pperm)
    for (int i = tid; i < pn.nnz_cnt; i += 256) spos[i] = a.pperm[pn.nnz0 + i];
  __syncthreads();

  const int g = tid / LPR;
  const int rpg = (pn.nrows + NG - 1) / NG;
  int r = min(g * rpg, pn.nrows);
  const int re = min(r + rpg, pn.nrows);
  if (r >= re || !col_ok) return;

  int pos = sptr[r];
  const int stop = sptr[re];
  int row_end = sptr[r + 1];
  while (pos < stop) {  // the flat walk is in position order
    const int n = min(U, stop - pos);
    V v[U];
    int32_t ar[U][VEC];
#pragma unroll
    for (int k = 0; k < U; k++) {
      const int64_t idx = sind[pos + min(k, n - 1)];
      v[k] = V::load(src + idx * F + col);
#pragma unroll
      for (int i = 0; i < VEC; i++) ar[k][i] = -1;
      if constexpr (SEL) L::iload(a.arg_in + idx * F + col, ar[k]);
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
      if (k < n) {
        while (row_end <= pos + k) {
          store_row(pn.row0 + r, sA[r], sB[r]);
          reset();
          r++;
          row_end = sptr[r + 1];
        }
        take(v[k], ar[k], a.pperm ? spos[pos + k] : pn.nnz0 + pos + k, true);
      }
    }
    pos += n;
  }
  while (r < re) {
    store_row(pn.row0 + r, sA[r], sB[r]);
    reset();
    r++;
  }
}

// The fixups of a max / min gather: the winner among a row's partial slots by the same rule, slot order immaterial; a
// first-level fixup (pad > 0) leaves (value, position) in slot pad - 1 of both tables for the final one.
template <int LPR, int VEC, bool MAX>
__global__ __launch_bounds__(256) void fixup_rows_reduce_kernel(const ReduceGatherArgs a, const Fixup *fixups, int nfix) {
  using V = Vec<VEC>;
  using L = Lane<VEC>;
  const int tid = threadIdx.x;
  const int gl = tid & (LPR - 1);
  const int col = (blockIdx.y * LPR + gl) * VEC;
  const int f = blockIdx.x * (256 / LPR) + tid / LPR;
  if (f >= nfix || col >= a.F) return;
  const Fixup fx = fixups[f];
  const int64_t F = a.F;
  const float *pv = a.partial + (int64_t)fx.first * F + col;
  const int32_t *pp = a.ipartial + (int64_t)fx.first * F + col;
  float bv[VEC];
  int32_t bp[VEC];
#pragma unroll
  for (int i = 0; i < VEC; i++) bv[i] = MAX ? -__builtin_inff() : __builtin_inff(), bp[i] = kNoPos;
  for (int k = 0; k < fx.count; k += 4) {  // four slots' loads in flight
    float x[4][VEC];
    int32_t p[4][VEC];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int64_t s = min(k + j, fx.count - 1);  // past the end: the last slot again, which changes nothing
      L::unpack(V::load(pv + s * F), x[j]);
      L::iload(pp + s * F, p[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int i = 0; i < VEC; i++)
        if (beats<MAX>(x[j][i], p[j][i], bv[i], bp[i])) bv[i] = x[j][i], bp[i] = p[j][i];
  }
  if (fx.pad > 0) {
    L::pack(bv).store(a.partial + (int64_t)(fx.pad - 1) * F + col);
    L::istore(a.ipartial + (int64_t)(fx.pad - 1) * F + col, bp);
    return;
  }
  const float sa = a.scaleA ? a.scaleA[fx.row] : 1.f, sb = a.scaleB ? a.scaleB[fx.row] : 1.f;
  int32_t o[VEC];
#pragma unroll
  for (int i = 0; i < VEC; i++) {  // a split row has entries: every column has a winner
    bv[i] = (bv[i] * sa) * sb;
    o[i] = bp[i];
  }
  L::pack(bv).store(static_cast<float *>(a.dst) + (int64_t)fx.row * F + col);
  L::istore(a.arg_out + (int64_t)fx.row * F + col, o);
}

// out[p] = <A[ind[p], :], B[e, :]> for every entry p of the CSR (ptr, ind), e the row that holds p: the gradient of
// a per-entry weight of hg_aggr_incidence_f32.  Work is cut by entries, not rows (a power-law row reaches 4096
// entries): a lane group of LPR lanes owns kDotRun consecutive entries.  It finds the row of its first entry by a
// binary search inside the workgroup's row range (itself two uniform searches over ptr), then steps along.  Each output
// is one lane group's: the lanes' fma chains over their columns, then a fixed butterfly over the LPR lanes --
// deterministic.  The kDotRun entries' row loads are issued together.  TA / TB: element types of A's / B's rows (Rows): a
// bf16 operand is widened in the load (exact), so the fma chain and the butterfly see the floats the fp32 instance sees.
constexpr int kDotRun = 4;
__device__ __forceinline__ int row_of(const int32_t *ptr, int lo, int hi, int64_t p) {  // ptr[lo] <= p < ptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}
template <int LPR, int VEC, typename TA = float, typename TB = float>
__global__ __launch_bounds__(256) void incidence_dot_kernel(const int32_t *ptr, const int32_t *ind, int32_t M, int64_t nnz,
                                                            int32_t F, const TA *A, const TB *B, float *out) {
  using V = Vec<VEC>;
  constexpr int NG = 256 / LPR;
  const int tid = threadIdx.x, gl = tid & (LPR - 1), g = tid / LPR;
  const int64_t c0 = (int64_t)blockIdx.x * NG * kDotRun;
  const int64_t c1 = std::min<int64_t>(c0 + NG * kDotRun, nnz);
  const int64_t p0 = c0 + (int64_t)g * kDotRun;
  if (p0 >= c1) return;
  const int elo = row_of(ptr, 0, M, c0);
  const int ehi = row_of(ptr, elo, M, c1 - 1);
  int e = row_of(ptr, elo, ehi + 1, p0);
  const int n = (int)std::min<int64_t>(kDotRun, nnz - p0);
  int64_t ua[kDotRun], eb[kDotRun];
#pragma unroll
  for (int k = 0; k < kDotRun; k++) {
    const int64_t p = p0 + std::min(k, n - 1);
    while (ptr[e + 1] <= p) e++;
    ua[k] = (int64_t)ind[p] * F;
    eb[k] = (int64_t)e * F;
  }
  float acc[kDotRun];
#pragma unroll
  for (int k = 0; k < kDotRun; k++) acc[k] = 0.f;
  for (int c = gl * VEC; c < F; c += LPR * VEC) {
    V x[kDotRun], y[kDotRun];
#pragma unroll
    for (int k = 0; k < kDotRun; k++) {
      x[k] = Rows<TA, VEC>::load(A + ua[k] + c);
      y[k] = Rows<TB, VEC>::load(B + eb[k] + c);
    }
#pragma unroll
    for (int k = 0; k < kDotRun; k++) {
      if constexpr (VEC == 4) {
        acc[k] = __builtin_fmaf(x[k].v.x, y[k].v.x, acc[k]);
        acc[k] = __builtin_fmaf(x[k].v.y, y[k].v.y, acc[k]);
        acc[k] = __builtin_fmaf(x[k].v.z, y[k].v.z, acc[k]);
        acc[k] = __builtin_fmaf(x[k].v.w, y[k].v.w, acc[k]);
      } else {
        acc[k] = __builtin_fmaf(x[k].x, y[k].x, acc[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kDotRun; k++) {
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) acc[k] += __shfl_xor(acc[k], off, 64);
    if (gl == 0 && k < n) out[p0 + k] = acc[k];
  }
}

// The same per head: out[p, h] = <A[ind[p], hC .. (h+1)C), B[e, hC .. (h+1)C)>, out [nnz, H] with the head fastest.  A lane
// group of LPH lanes (the lanes C columns need, up to 64) owns one head of kDotRun consecutive entries; consecutive lane
// groups take the consecutive heads of the same entries, so a wave reads neighbouring pieces of the same rows.  The
// butterfly runs over a group's LPH lanes only: the lanes of one head are reduced apart from their neighbours, in a
// fixed order.
template <int LPH, int VEC, typename TA = float, typename TB = float>
__global__ __launch_bounds__(256) void incidence_dot_heads_kernel(const int32_t *ptr, const int32_t *ind, int32_t M,
                                                                  int64_t nnz, int32_t H, int32_t C, const TA *A,
                                                                  const TB *B, float *out) {
  using V = Vec<VEC>;
  constexpr int NG = 256 / LPH;
  const int tid = threadIdx.x, gl = tid & (LPH - 1), g = tid / LPH;
  const int64_t F = (int64_t)H * C;
  const int64_t item0 = (int64_t)blockIdx.x * NG;  // items: (run of kDotRun entries, head), head fastest
  const int64_t item = item0 + g;
  const int64_t p0 = item / H * kDotRun;
  const int h = (int)(item % H);
  if (p0 >= nnz) return;
  const int64_t c0 = item0 / H * kDotRun;
  const int64_t c1 = std::min<int64_t>(((item0 + NG - 1) / H + 1) * kDotRun, nnz);
  const int elo = row_of(ptr, 0, M, c0);
  const int ehi = row_of(ptr, elo, M, c1 - 1);
  int e = row_of(ptr, elo, ehi + 1, p0);
  const int n = (int)std::min<int64_t>(kDotRun, nnz - p0);
  int64_t ua[kDotRun], eb[kDotRun];
#pragma unroll
  for (int k = 0; k < kDotRun; k++) {
    const int64_t p = p0 + std::min(k, n - 1);
    while (ptr[e + 1] <= p) e++;
    ua[k] = (int64_t)ind[p] * F + (int64_t)h * C;
    eb[k] = (int64_t)e * F + (int64_t)h * C;
  }
  float acc[kDotRun];
#pragma unroll
  for (int k = 0; k < kDotRun; k++) acc[k] = 0.f;
  for (int c = gl * VEC; c < C; c += LPH * VEC) {
    V x[kDotRun], y[kDotRun];
#pragma unroll
    for (int k = 0; k < kDotRun; k++) {
      x[k] = Rows<TA, VEC>::load(A + ua[k] + c);
      y[k] = Rows<TB, VEC>::load(B + eb[k] + c);
    }
#pragma unroll
    for (int k = 0; k < kDotRun; k++) {
      if constexpr (VEC == 4) {
        acc[k] = __builtin_fmaf(x[k].v.x, y[k].v.x, acc[k]);
        acc[k] = __builtin_fmaf(x[k].v.y, y[k].v.y, acc[k]);
        acc[k] = __builtin_fmaf(x[k].v.z, y[k].v.z, acc[k]);
        acc[k] = __builtin_fmaf(x[k].v.w, y[k].v.w, acc[k]);
      } else {
        acc[k] = __builtin_fmaf(x[k].x, y[k].x, acc[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kDotRun; k++) {
#pragma unroll
    for (int off = 1; off < LPH; off <<= 1) acc[k] += __shfl_xor(acc[k], off, 64);
    if (gl == 0 && k < n) out[(p0 + k) * H + h] = acc[k];
  }
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the
// vector-memory counter, which on CDNA4 counts stores: in a persistent loop that would
// expose the full latency of the Y stores at every panel boundary.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- fp32 MFMA: rows of an LDS tile times Wlin^T ------------------------------------
// The one dense contraction next to the path (the nn.Linear of HGNNConv / UniGIN, reference
// model/ugsys/hgnn.py:22).  v_mfma_f32_16x16x4_f32: exact f32 (a k-ordered fmaf chain), A and
// B one VGPR per lane -- lane l holds A[row l&15][k l>>4] and B[k l>>4][col l&15], D is
// row 4*(l>>4)+i, col l&15 in register i.
// A wave owns 16-column tiles of the output: the K/4 B fragments of a tile (= 16 rows of
// Wlin) sit in K/4 VGPRs, read straight from global memory (L2-resident, 4 KB per tile), and
// are reused for every row of the panel, so Wlin takes no LDS and no barrier.  The A
// fragments come from the panel's rows in LDS (row stride K+4 floats: the 64 lanes of a read
// fall on every bank exactly twice), up to four 16-row tiles at a time = four independent
// accumulators, which is what the 40-cycle dependent latency of the instruction needs.
typedef float hg_f4 __attribute__((ext_vector_type(4)));

struct LinSplit {  // how the four waves share (column tile, row tile) space
  int nt_first, nt_step, rt_first, rt_step;
  bool active;
};
__device__ __forceinline__ LinSplit lin_split(int wid, int NT) {
  const int nwn = NT >= 4 ? 4 : (NT == 3 ? 3 : NT);  // waves across column tiles
  const int nwr = NT >= 3 ? 1 : 4 / nwn;             // waves across row tiles
  LinSplit s;
  s.nt_first = wid % nwn;
  s.nt_step = nwn;
  s.rt_first = wid / nwn;
  s.rt_step = nwr;
  s.active = wid < nwn * nwr;
  return s;
}

// Wlin arrives packed in fragment order (linear_pack_kernel): the K/4 B fragments of a column
// tile are K/16 coalesced dwordx4 reads per lane (two 128-byte lines per 4 fragments).  Read
// straight from the row-major matrix the same fragments touch 16 lines per instruction -- more
// line requests per panel than the whole X gather.
//   wfrag[((nt * K/16 + q) * 64 + lane) * 4 + j] = Wlin[nt*16 + (lane & 15)][(4q + j)*4 + (lane >> 4)]
template <int KSTEPS>
__device__ __forceinline__ void load_bfrag(const float *wfrag, int nt, int lane, float (&bv)[KSTEPS]) {
  const float4 *w = reinterpret_cast<const float4 *>(wfrag) + (int64_t)nt * (KSTEPS / 4) * 64 + lane;
#pragma unroll
  for (int q = 0; q < KSTEPS / 4; q++) {
    const float4 f = w[q * 64];
    bv[q * 4 + 0] = f.x;
    bv[q * 4 + 1] = f.y;
    bv[q * 4 + 2] = f.z;
    bv[q * 4 + 3] = f.w;
  }
}

// K = 128 (32 k-steps): holding all 32 B-fragment registers of a column tile through the matrix phase is what kept the
// LIN instances at 5 waves per SIMD.  There the fragments travel in chunks of 8 k-steps (two dwordx4 per lane), the
// next chunk in flight while the current one feeds the matrix pipe.  BPre<KSTEPS>::N = fragments the caller preloads.
template <int KSTEPS> struct BPre {
  static constexpr int CH = KSTEPS >= 32 ? 8 : KSTEPS;  // k-steps per chunk
  static constexpr int N = CH;
};
template <int KSTEPS>
__device__ __forceinline__ void load_bfrag_chunk(const float *wfrag, int nt, int chunk, int lane, float (&b)[8]) {
  const float4 *w = reinterpret_cast<const float4 *>(wfrag) + ((int64_t)nt * (KSTEPS / 4) + 2 * chunk) * 64 + lane;
  const float4 f0 = w[0], f1 = w[64];
  b[0] = f0.x; b[1] = f0.y; b[2] = f0.z; b[3] = f0.w;
  b[4] = f1.x; b[5] = f1.y; b[6] = f1.z; b[7] = f1.w;
}
template <int KSTEPS>
__device__ __forceinline__ void load_bfrag_pre(const float *wfrag, int nt, int lane, float (&b)[BPre<KSTEPS>::N]) {
  if constexpr (KSTEPS >= 32) load_bfrag_chunk<KSTEPS>(wfrag, nt, 0, lane, b);
  else load_bfrag<KSTEPS>(wfrag, nt, lane, b);
}

__global__ __launch_bounds__(256) void linear_pack_kernel(int32_t F_out, int32_t F_in, const float *Wlin,
                                                          float *wfrag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)F_out * F_in) return;
  const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
  const int64_t u = i >> 8;  // nt * K/16 + q
  const int k16 = F_in >> 4;
  const int q = (int)(u % k16), nt = (int)(u / k16);
  wfrag[i] = Wlin[(int64_t)(nt * 16 + (lane & 15)) * F_in + (4 * q + j) * 4 + (lane >> 4)];
}

// NRT row tiles rt0, rt0 + rt_step, ... against one column tile whose B fragments are in bv.
template <int KSTEPS, int NRT>
__device__ __forceinline__ void mfma_rows(const float *t, int ld, int rt0, int rt_step, const float (&bv)[KSTEPS],
                                          hg_f4 *acc, int lane) {
  const float *ta = t + (rt0 * 16 + (lane & 15)) * ld + (lane >> 4);
  const int tstep = rt_step * 16 * ld;
#pragma unroll
  for (int j = 0; j < NRT; j++) acc[j] = hg_f4{0.f, 0.f, 0.f, 0.f};
  // A fragments two steps ahead of the MFMAs that use them (an LDS read takes about as long as
  // the NRT MFMAs of one step).  The scheduling barriers pin that order: left alone the compiler
  // either hoists all K/4 * NRT reads to the top (3 waves/SIMD) or sinks them next to their use.
  float a0[NRT], a1[NRT], a2[NRT];
#pragma unroll
  for (int j = 0; j < NRT; j++) a0[j] = ta[j * tstep];
  if (KSTEPS > 1) {
#pragma unroll
    for (int j = 0; j < NRT; j++) a1[j] = ta[j * tstep + 4];
  }
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ks++) {
    if (ks + 2 < KSTEPS) {
#pragma unroll
      for (int j = 0; j < NRT; j++) a2[j] = ta[j * tstep + (ks + 2) * 4];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NRT; j++)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], bv[ks], acc[j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NRT; j++) {
      a0[j] = a1[j];
      a1[j] = a2[j];
    }
  }
}

template <int KSTEPS>
__device__ __forceinline__ void mfma_rows_n(int n, const float *t, int ld, int rt0, int rt_step,
                                            const float (&bv)[KSTEPS], hg_f4 *acc, int lane) {
  switch (n) {  // wave-uniform
    case 4: mfma_rows<KSTEPS, 4>(t, ld, rt0, rt_step, bv, acc, lane); break;
    case 3: mfma_rows<KSTEPS, 3>(t, ld, rt0, rt_step, bv, acc, lane); break;
    case 2: mfma_rows<KSTEPS, 2>(t, ld, rt0, rt_step, bv, acc, lane); break;
    case 1: mfma_rows<KSTEPS, 1>(t, ld, rt0, rt_step, bv, acc, lane); break;
    default: break;
  }
}

// The rows t[0 .. nrows) (LDS, stride K+4) times Wlin^T -> Y.  Called by all 256 threads once the
// rows are complete.  bv: the B fragments of the wave's first column tile, which the caller
// loaded ahead of time to hide their latency.
// F_out <= K: the results go back into `t` (two barriers) and leave as whole rows, 16 bytes per
// lane -- a row written as four 64-byte pieces by four waves at four different times costs the
// memory system partial-line writes.  NPW = column tiles per wave (1 or 2).
template <int KSTEPS, int NPW>
__device__ __forceinline__ void panel_times_wt_staged(float *t, int nrows, int F_out, const float *Wlin,
                                                      const int32_t *rowmap, int64_t row0, float *Y, int tid,
                                                      float (&bv)[KSTEPS], int relu) {
  constexpr int K = KSTEPS * 4, LD = K + 4, RPN = 4 / NPW;  // row tiles per column tile and wave
  const int lane = tid & 63;
  const int NT = F_out >> 4, RT = (nrows + 15) >> 4;
  const LinSplit sp = lin_split(tid >> 6, NT);
  hg_f4 acc[4];
  int nrt = 0;
  if (sp.active) {
    nrt = min(RPN, max(0, (RT - sp.rt_first + sp.rt_step - 1) / sp.rt_step));
#pragma unroll
    for (int ni = 0; ni < NPW; ni++) {
      const int nt = sp.nt_first + ni * sp.nt_step;
      if (nt < NT) {
        if (ni > 0) load_bfrag<KSTEPS>(Wlin, nt, lane, bv);
        mfma_rows_n<KSTEPS>(nrt, t, LD, sp.rt_first, sp.rt_step, bv, acc + ni * RPN, lane);
      }
    }
  }
  __syncthreads();  // every wave has read its A fragments: the rows can be overwritten
  if (sp.active) {
#pragma unroll
    for (int ni = 0; ni < NPW; ni++) {
      const int nt = sp.nt_first + ni * sp.nt_step;
      if (nt < NT) {
#pragma unroll
        for (int j = 0; j < RPN; j++)
          if (j < nrt) {
            float *d = t + ((sp.rt_first + j * sp.rt_step) * 16 + 4 * (lane >> 4)) * LD + nt * 16 + (lane & 15);
#pragma unroll
            for (int i = 0; i < 4; i++) d[i * LD] = acc[ni * RPN + j][i];
          }
      }
    }
  }
  __syncthreads();
  const int q = F_out >> 2;  // float4 pieces per row
  for (int i = tid; i < nrows * q; i += 256) {
    const int r = i / q, c = (i - r * q) * 4;
    const int64_t yrow = rowmap ? (int64_t)rowmap[r] : row0 + r;
    float4 o = *reinterpret_cast<const float4 *>(t + r * LD + c);
    if (relu) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
    Vec<4>{o}.store_nt(Y + yrow * F_out + c);
  }
}

// The matrix phase for K = 128: B fragments in chunks of 8 k-steps, double-buffered (16 registers instead of 32 per
// column tile), the A-fragment reads two k-steps ahead of their MFMAs as in mfma_rows.  NRT row tiles (compile time)
// against the wave's NPW column tiles; acc[ni * RPN + j].
template <int KSTEPS, int NPW, int NRT>
__device__ __forceinline__ void mfma_rows_chunked(const float *ta, int tstep, const float *Wlin, const LinSplit &sp, int NT,
                                                  int lane, const float (&bpre)[8], hg_f4 *acc) {
  constexpr int RPN = 4 / NPW, CH = 8, NCH = KSTEPS / CH;
  float bcur[8], bnxt[8];
#pragma unroll
  for (int i = 0; i < 8; i++) bcur[i] = bpre[i];
#pragma unroll
  for (int ni = 0; ni < NPW; ni++) {
    const int nt = sp.nt_first + ni * sp.nt_step;
    if (nt < NT) {  // wave-uniform
      float a0[NRT], a1[NRT], a2[NRT];
#pragma unroll
      for (int j = 0; j < NRT; j++) {
        a0[j] = ta[j * tstep];
        a1[j] = ta[j * tstep + 4];
      }
#pragma unroll
      for (int c = 0; c < NCH; c++) {
        // the next chunk's fragments (this column tile's, or chunk 0 of the wave's next tile) fly during this one's MFMAs
        const int nt2 = sp.nt_first + (ni + 1) * sp.nt_step;
        if (c + 1 < NCH) load_bfrag_chunk<KSTEPS>(Wlin, nt, c + 1, lane, bnxt);
        else if (ni + 1 < NPW && nt2 < NT) load_bfrag_chunk<KSTEPS>(Wlin, nt2, 0, lane, bnxt);
#pragma unroll
        for (int k8 = 0; k8 < CH; k8++) {
          const int ks = c * CH + k8;
          if (ks + 2 < KSTEPS) {
#pragma unroll
            for (int j = 0; j < NRT; j++) a2[j] = ta[j * tstep + (ks + 2) * 4];
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int j = 0; j < NRT; j++)
            acc[ni * RPN + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], bcur[k8], acc[ni * RPN + j], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int j = 0; j < NRT; j++) {
            a0[j] = a1[j];
            a1[j] = a2[j];
          }
        }
        if (c + 1 < NCH || (ni + 1 < NPW && nt2 < NT)) {
#pragma unroll
          for (int i = 0; i < 8; i++) bcur[i] = bnxt[i];
        }
      }
    }
  }
}

// The staged form (see panel_times_wt_staged) on the chunked matrix phase.  bpre: chunk 0 of the wave's first column
// tile, loaded by the caller ahead of the barriers.
template <int KSTEPS, int NPW>
__device__ __forceinline__ void panel_times_wt_staged_chunked(float *t, int nrows, int F_out, const float *Wlin,
                                                              const int32_t *rowmap, int64_t row0, float *Y, int tid,
                                                              float (&bpre)[8], int relu) {
  constexpr int K = KSTEPS * 4, LD = K + 4, RPN = 4 / NPW;
  const int lane = tid & 63;
  const int NT = F_out >> 4, RT = (nrows + 15) >> 4;
  const LinSplit sp = lin_split(tid >> 6, NT);
  hg_f4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; j++) acc[j] = hg_f4{0.f, 0.f, 0.f, 0.f};
  int nrt = 0;
  if (sp.active) {
    nrt = min(RPN, max(0, (RT - sp.rt_first + sp.rt_step - 1) / sp.rt_step));
    const float *ta = t + (sp.rt_first * 16 + (lane & 15)) * LD + (lane >> 4);
    const int tstep = sp.rt_step * 16 * LD;
    switch (nrt) {  // wave-uniform
      case 4: if constexpr (RPN >= 4) mfma_rows_chunked<KSTEPS, NPW, 4>(ta, tstep, Wlin, sp, NT, lane, bpre, acc); break;
      case 3: if constexpr (RPN >= 4) mfma_rows_chunked<KSTEPS, NPW, 3>(ta, tstep, Wlin, sp, NT, lane, bpre, acc); break;
      case 2: if constexpr (RPN >= 2) mfma_rows_chunked<KSTEPS, NPW, 2>(ta, tstep, Wlin, sp, NT, lane, bpre, acc); break;
      case 1: mfma_rows_chunked<KSTEPS, NPW, 1>(ta, tstep, Wlin, sp, NT, lane, bpre, acc); break;
      default: break;
    }
  }
  __syncthreads();  // every wave has read its A fragments: the rows can be overwritten
  if (sp.active) {
#pragma unroll
    for (int ni = 0; ni < NPW; ni++) {
      const int nt = sp.nt_first + ni * sp.nt_step;
      if (nt < NT) {
#pragma unroll
        for (int j = 0; j < RPN; j++)
          if (j < nrt) {
            float *d = t + ((sp.rt_first + j * sp.rt_step) * 16 + 4 * (lane >> 4)) * LD + nt * 16 + (lane & 15);
#pragma unroll
            for (int i = 0; i < 4; i++) d[i * LD] = acc[ni * RPN + j][i];
          }
      }
    }
  }
  __syncthreads();
  const int q = F_out >> 2;  // float4 pieces per row
  for (int i = tid; i < nrows * q; i += 256) {
    const int r = i / q, c = (i - r * q) * 4;
    const int64_t yrow = rowmap ? (int64_t)rowmap[r] : row0 + r;
    float4 o = *reinterpret_cast<const float4 *>(t + r * LD + c);
    if (relu) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
    Vec<4>{o}.store_nt(Y + yrow * F_out + c);
  }
}

// ---- fp32 by six bf16 products (K = 128 staged epilogue, HG_LIN_BF16X6) ---------------------------------------------
// v_mfma_f32_16x16x4_f32 moves 64 FLOP per clock and SIMD, v_mfma_f32_16x16x32_bf16 1024.  A float is the sum of three
// bf16 numbers up to 2^-24 of itself (h = rn(x), m = rn(x - h), l = rn(x - h - m): both differences are exact), a product
// of two bf16 numbers is exact in fp32 and the matrix pipe accumulates in fp32, so
//   a * b = ah bh + (ah bm + am bh) + (ah bl + al bh + am bm) + O(2^-23 |a b|)
// -- six MFMAs of the bf16 form for what eight of the fp32 form do, at a sixteenth of the cycles each (16 against 32 per
// instruction, K = 32 against 4): the matrix phase's pipe time falls to 3/8.  The dropped terms (am bl, al bm, al bl and the
// split's own residual) are below one rounding of the fp32 product; the sum over k is fp32 either way.  What changes is the
// ORDER of the additions (the pipe adds 32 products per instruction, and the six partial products per k land apart), so
// results differ from the fp32 form in the last bits, as any fp32 GEMM's do from another's: tests bound both forms by the
// same 1e-5 x row mass against float64.  (The scheme TPUs call bf16_6x / "highest" precision.)
// Operand rows: three planes of [32 rows][128] bf16 in the tile region (24 KB = the 48 slot rows of the epilogue's
// schedule), 16-byte chunk c of row r stored at chunk c ^ (r & 15): the A-fragment read (ds_read_b128, lane l = row l & 15,
// k-block l >> 4) and the 8-byte writes of hop 2's lanes both touch every bank once per 16 lanes.
typedef __bf16 hg_bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 hg_bf2 __attribute__((ext_vector_type(2)));
typedef float hg_f2 __attribute__((ext_vector_type(2)));
// bytes of one plane: the panel's rows (rows_cap of the schedule, whole groups of 8) of 256 bytes.  A panel of fewer than 32
// rows still has its second 16-row tile multiplied whole: those reads run into the next plane (the last plane's into the rest of
// the tile region, launcher-checked) and the rows they produce are never stored.
__host__ __device__ inline int split_plane_bytes(int rows_cap) { return (rows_cap + 7) / 8 * 8 * 256; }

__device__ __forceinline__ void split_bf16x3(float x, float y, unsigned &h, unsigned &m, unsigned &l) {
  const hg_f2 v{x, y};
  const hg_bf2 hb = __builtin_convertvector(v, hg_bf2);  // v_cvt_pk_bf16_f32: round to nearest even
  const hg_f2 r1 = v - __builtin_convertvector(hb, hg_f2);
  const hg_bf2 mb = __builtin_convertvector(r1, hg_bf2);
  const hg_f2 r2 = r1 - __builtin_convertvector(mb, hg_f2);
  const hg_bf2 lb = __builtin_convertvector(r2, hg_bf2);
  h = __builtin_bit_cast(unsigned, hb);
  m = __builtin_bit_cast(unsigned, mb);
  l = __builtin_bit_cast(unsigned, lb);
}
// byte offset inside a plane of the 8 bytes that hold columns k .. k + 3 of row r (k a multiple of 4)
__device__ __forceinline__ int split_off(int r, int k) { return r * 256 + ((((k >> 3) ^ r) & 15) << 4) + ((k & 4) << 1); }

__device__ __forceinline__ void split_store_row(char *planes, int pstride, int r, int k, const float4 &v) {
  unsigned h0, m0, l0, h1, m1, l1;
  split_bf16x3(v.x, v.y, h0, m0, l0);
  split_bf16x3(v.z, v.w, h1, m1, l1);
  char *p = planes + split_off(r, k);
  *reinterpret_cast<uint2 *>(p) = make_uint2(h0, h1);
  *reinterpret_cast<uint2 *>(p + pstride) = make_uint2(m0, m1);
  *reinterpret_cast<uint2 *>(p + 2 * pstride) = make_uint2(l0, l1);
}

// Wlin's three planes in fragment order, behind the fp32 fragments of linear_pack_kernel (hub rows and the other
// variants' rows still go through linear_rows_kernel):
//   wsplit[(((nt * K/32 + ks) * 3 + p) * 64 + lane)] = 8 bf16: plane p of Wlin[nt*16 + (lane & 15)][ks*32 + 8*(lane >> 4) + j]
__global__ __launch_bounds__(256) void linear_pack_split_kernel(int32_t F_out, int32_t F_in, const float *Wlin, uint4 *wsplit) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (nt, ks, lane)
  const int k32 = F_in >> 5;
  if (i >= (int64_t)(F_out >> 4) * k32 * 64) return;
  const int lane = (int)(i & 63), ks = (int)((i >> 6) % k32), nt = (int)((i >> 6) / k32);
  const float *w = Wlin + (int64_t)(nt * 16 + (lane & 15)) * F_in + ks * 32 + 8 * (lane >> 4);
  unsigned h[4], m[4], l[4];
#pragma unroll
  for (int j = 0; j < 4; j++) split_bf16x3(w[2 * j], w[2 * j + 1], h[j], m[j], l[j]);
  uint4 *o = wsplit + ((int64_t)(nt * k32 + ks) * 3) * 64 + lane;
  o[0] = make_uint4(h[0], h[1], h[2], h[3]);
  o[64] = make_uint4(m[0], m[1], m[2], m[3]);
  o[128] = make_uint4(l[0], l[1], l[2], l[3]);
}

struct SplitB {
  uint4 h, m, l;
};
__device__ __forceinline__ SplitB load_bsplit(const uint4 *wsplit, int nt, int ks, int lane) {
  const uint4 *w = wsplit + ((int64_t)(nt * 4 + ks) * 3) * 64 + lane;
  return SplitB{w[0], w[64], w[128]};
}
__device__ __forceinline__ hg_f4 mfma_bf16(const uint4 &a, const uint4 &b, hg_f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(hg_bf8, a), __builtin_bit_cast(hg_bf8, b), c, 0, 0, 0);
}

// Step t of a wave's matrix phase = (k-step t / npw, the wave's column tile t % npw); a column tile past the last one (F_out not
// a multiple of 64: the last wave has one tile fewer) is clamped -- its products are computed and never written back.
constexpr int kSplitDepth = 2;  // steps of B fragments in registers (12 VGPRs each)
__device__ __forceinline__ SplitB load_bsplit_step(const uint4 *wsplit, const LinSplit &sp, int NT, int npw, int t, int lane) {
  const int ni = npw == 2 ? (t & 1) : 0, ks = npw == 2 ? (t >> 1) : t;
  return load_bsplit(wsplit, min(sp.nt_first + ni * sp.nt_step, NT - 1), ks, lane);
}

// NRT row tiles against the wave's NPW column tiles, K = 128 = four k-steps of 32: 4 * NPW steps of 6 * NRT MFMAs.  The phase is
// bound by the B fragments' way from the L2 (three dwordx4 per step, ~900 cycles under load against ~200 cycles of MFMAs per
// step: with one step in flight the phase took 7.5 k cycles of a wave's life for 1.5 k cycles of matrix pipe, stamps in
// profiles/r04_experiments.md 6).  D steps of fragments live in registers: the first D are loaded by the caller BEFORE hop 2 (they
// arrive during it), and the registers of a finished step take the fragments of step t + D.  A row tile's A fragments (three
// ds_read_b128) are read per step -- held across a k-step's column tiles they would be 12 more registers.  The small products
// go in first.
template <int NPW, int NRT, int D>
__device__ __forceinline__ void mfma_rows_split(const char *planes, int pstride, const uint4 *wsplit, const LinSplit &sp, int NT, int lane,
                                                SplitB (&bq)[D], hg_f4 *acc) {
  constexpr int RPN = 4 / NPW, NS = 4 * NPW, NI = NS * NRT;
  const int r = lane & 15, kb = lane >> 4;
  const char *prow = planes + (sp.rt_first * 16 + r) * 256;
  const int rstep = sp.rt_step * 16 * 256;
  // iteration i = (step t, row tile j): six MFMAs on the A fragments of (k-step, row tile) -- three ds_read_b128, planes h, m, l.
  // An LDS read under six workgroups' traffic takes longer than the 96 cycles of an iteration's MFMAs, and read where they are
  // used every iteration paid that wait (16 iterations: most of the phase's 7 k cycles for 1.5 k cycles of matrix pipe).  A
  // second set of fragment registers does not fit the six-wave budget, so the next iteration's fragments are read IN PLACE: a
  // plane's registers are free once the last MFMA that reads them has issued -- l after the first, m after the third, h after the
  // sixth -- and its next read goes out right there, three to five MFMAs ahead of its first use.  The scheduling barriers pin that
  // order (left alone the compiler gathers the three reads in front of the iteration that uses them).
  auto a_ptr = [&](int i) { const int t = i / NRT, j = i % NRT; return prow + j * rstep + ((((t / NPW * 4 + kb) ^ r) & 15) << 4); };
  uint4 ah, am, al;
  {
    const char *p = a_ptr(0);
    ah = *reinterpret_cast<const uint4 *>(p);
    am = *reinterpret_cast<const uint4 *>(p + pstride);
    al = *reinterpret_cast<const uint4 *>(p + 2 * pstride);
  }
#pragma unroll
  for (int i = 0; i < NI; i++) {
    const int t = i / NRT, j = i % NRT, ni = t % NPW;
    const char *pn = a_ptr(i + 1 < NI ? i + 1 : i);
    const SplitB &b = bq[t % D];
    hg_f4 c = acc[ni * RPN + j];
    const bool rd = i + 1 < NI;
    c = mfma_bf16(al, b.h, c);
    __builtin_amdgcn_sched_barrier(0);
    if (rd) al = *reinterpret_cast<const uint4 *>(pn + 2 * pstride);
    __builtin_amdgcn_sched_barrier(0);
    c = mfma_bf16(am, b.m, c);
    c = mfma_bf16(am, b.h, c);
    __builtin_amdgcn_sched_barrier(0);
    if (rd) am = *reinterpret_cast<const uint4 *>(pn + pstride);
    __builtin_amdgcn_sched_barrier(0);
    c = mfma_bf16(ah, b.l, c);
    c = mfma_bf16(ah, b.m, c);
    c = mfma_bf16(ah, b.h, c);
    acc[ni * RPN + j] = c;
    __builtin_amdgcn_sched_barrier(0);
    if (rd) ah = *reinterpret_cast<const uint4 *>(pn);
    if (j == NRT - 1 && t + D < NS) bq[t % D] = load_bsplit_step(wsplit, sp, NT, NPW, t + D, lane);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// panel_times_wt_staged_chunked on the split operands: planes = the tile region (operand rows as three bf16 planes); the
// fp32 results go back into the same region as [rows][K + 4] floats and leave as whole rows.
template <int NPW>
__device__ __forceinline__ void panel_times_wt_split(float *t, int pstride, int nrows, int F_out, const uint4 *wsplit, const int32_t *rowmap,
                                                     float *Y, int tid, SplitB (&bq)[kSplitDepth], int relu) {
  constexpr int K = 128, LD = K + 4, RPN = 4 / NPW;
  const int lane = tid & 63;
  const int NT = F_out >> 4, RT = (nrows + 15) >> 4;
  const LinSplit sp = lin_split(tid >> 6, NT);
  hg_f4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; j++) acc[j] = hg_f4{0.f, 0.f, 0.f, 0.f};
  int nrt = 0;
  if (sp.active) {
    nrt = min(2, max(0, (RT - sp.rt_first + sp.rt_step - 1) / sp.rt_step));  // at most 32 rows (launcher)
    const char *planes = reinterpret_cast<const char *>(t);
    if constexpr (NPW == 2) {
      // F_out > 64: every wave walks the row tiles from 0 (lin_split) -- both tiles always, no branch around the preloaded
      // fragments (a panel of the epilogue's schedule has 29 of its 32 rows on average; the second tile of a shorter one
      // multiplies whatever the planes hold there, and those rows are never stored)
      nrt = RT;
      mfma_rows_split<NPW, 2, kSplitDepth>(planes, pstride, wsplit, sp, NT, lane, bq, acc);
    } else if (nrt == 2) {
      mfma_rows_split<NPW, 2, kSplitDepth>(planes, pstride, wsplit, sp, NT, lane, bq, acc);
    } else if (nrt == 1) {
      mfma_rows_split<NPW, 1, kSplitDepth>(planes, pstride, wsplit, sp, NT, lane, bq, acc);
    }
  }
  __syncthreads();  // every wave has read its A fragments: the planes can be overwritten
  if (sp.active) {
#pragma unroll
    for (int ni = 0; ni < NPW; ni++) {
      const int nt = sp.nt_first + ni * sp.nt_step;
      if (nt < NT) {
#pragma unroll
        for (int j = 0; j < RPN; j++)
          if (j < nrt) {
            float *d = t + ((sp.rt_first + j * sp.rt_step) * 16 + 4 * (lane >> 4)) * LD + nt * 16 + (lane & 15);
#pragma unroll
            for (int i = 0; i < 4; i++) d[i * LD] = acc[ni * RPN + j][i];
          }
      }
    }
  }
  __syncthreads();
  const int q = F_out >> 2;  // float4 pieces per row
  for (int i = tid; i < nrows * q; i += 256) {
    const int r = i / q, c = (i - r * q) * 4;
    float4 o = *reinterpret_cast<const float4 *>(t + r * LD + c);
    if (relu) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
    Vec<4>{o}.store_nt(Y + (int64_t)rowmap[r] * F_out + c);
  }
}

// ---- native bf16 epilogue (hg_aggr_linear_res_bf16, K = 128) ---------------------------------------------------------
// The split matrix phase with one plane and one product: the combined row, rounded to bf16 once, IS its own h plane, and a
// bf16 weight is its own h plane -- one MFMA per (k-step, row tile, column tile) where the bf16x6 form issues six, one
// ds_read_b128 per A fragment, one dwordx4 per B fragment.  The plane keeps split_off's swizzle (plane stride 0).
//   wb[(nt * K/32 + ks) * 64 + lane] = 8 bf16: Wb[nt*16 + (lane & 15)][ks*32 + 8*(lane >> 4) + j]   (linear_pack_bf16_kernel)
__device__ __forceinline__ unsigned round_bf16x2(float x, float y) {  // v_cvt_pk_bf16_f32: round to nearest even
  return __builtin_bit_cast(unsigned, __builtin_convertvector(hg_f2{x, y}, hg_bf2));
}
__device__ __forceinline__ uint2 round_bf16x4(const float4 &v) { return make_uint2(round_bf16x2(v.x, v.y), round_bf16x2(v.z, v.w)); }

// Steps of B fragments in registers (4 VGPRs each); as in the split form the first kB16Depth are loaded BEFORE hop 2 and
// arrive during it.  Two steps, the split form's depth; a depth of four (every step of a narrow output) compiled to 6-8 more
// VGPRs through hop 2 and was not timed.
constexpr int kB16Depth = 2;
// Row gathers in flight per lane in the bf16 epilogue's instances: twelve (kLinU32, the fp32 epilogue's) spilled 20 bytes per
// lane in the instance with materialised slots and scales at the six-wave budget; ten and eight are scratch-free (66-72 VGPRs).
constexpr int kB16U = 10;
__device__ __forceinline__ uint4 load_b16_step(const uint4 *wb, const LinSplit &sp, int NT, int npw, int t, int lane) {
  const int ni = npw == 2 ? (t & 1) : 0, ks = npw == 2 ? (t >> 1) : t;
  return wb[((int64_t)min(sp.nt_first + ni * sp.nt_step, NT - 1) * 4 + ks) * 64 + lane];
}

// mfma_rows_split's walk: iteration i = (step t, row tile j), here one MFMA on one A fragment, the next iteration's fragment
// read while it runs (a second fragment is 4 registers here, not 12).
template <int NPW, int NRT, int D>
__device__ __forceinline__ void mfma_rows_b16(const char *plane, const uint4 *wb, const LinSplit &sp, int NT, int lane, uint4 (&bq)[D],
                                              hg_f4 *acc) {
  constexpr int RPN = 4 / NPW, NS = 4 * NPW, NI = NS * NRT;
  const int r = lane & 15, kb = lane >> 4;
  const char *prow = plane + (sp.rt_first * 16 + r) * 256;
  const int rstep = sp.rt_step * 16 * 256;
  auto a_ptr = [&](int i) { const int t = i / NRT, j = i % NRT; return prow + j * rstep + ((((t / NPW * 4 + kb) ^ r) & 15) << 4); };
  uint4 an = *reinterpret_cast<const uint4 *>(a_ptr(0));
#pragma unroll
  for (int i = 0; i < NI; i++) {
    const int t = i / NRT, j = i % NRT, ni = t % NPW;
    const uint4 ac = an;
    if (i + 1 < NI) an = *reinterpret_cast<const uint4 *>(a_ptr(i + 1));
    acc[ni * RPN + j] = mfma_bf16(ac, bq[t % D], acc[ni * RPN + j]);
    if (j == NRT - 1 && t + D < NS) bq[t % D] = load_b16_step(wb, sp, NT, NPW, t + D, lane);
  }
}

// panel_times_wt_split on the one plane: the fp32 results go back into the tile region as [rows][K + 4] floats; then the
// optional relu, one rounding to bf16, and the values leave as whole rows of Y.  A row whose rowmap entry has bit 31 set is a
// piece of a split vertex (its sum went to a partial row): multiplied with the others, never stored.
template <int NPW>
__device__ __forceinline__ void panel_times_wt_b16(float *t, int nrows, int F_out, const uint4 *wb, const int32_t *rowmap, bf16 *Y, int tid,
                                                   uint4 (&bq)[kB16Depth], int relu, int y_nt) {
  constexpr int K = 128, LD = K + 4, RPN = 4 / NPW;
  const int lane = tid & 63;
  const int NT = F_out >> 4, RT = (nrows + 15) >> 4;
  const LinSplit sp = lin_split(tid >> 6, NT);
  hg_f4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; j++) acc[j] = hg_f4{0.f, 0.f, 0.f, 0.f};
  int nrt = 0;
  if (sp.active) {
    nrt = min(2, max(0, (RT - sp.rt_first + sp.rt_step - 1) / sp.rt_step));  // at most 32 rows (launcher)
    const char *plane = reinterpret_cast<const char *>(t);
    if constexpr (NPW == 2) {  // both row tiles always, as the split form (the second tile of a short panel is never stored)
      nrt = RT;
      mfma_rows_b16<NPW, 2, kB16Depth>(plane, wb, sp, NT, lane, bq, acc);
    } else if (nrt == 2) {
      mfma_rows_b16<NPW, 2, kB16Depth>(plane, wb, sp, NT, lane, bq, acc);
    } else if (nrt == 1) {
      mfma_rows_b16<NPW, 1, kB16Depth>(plane, wb, sp, NT, lane, bq, acc);
    }
  }
  __syncthreads();  // every wave has read its A fragments: the plane can be overwritten
  if (sp.active) {
#pragma unroll
    for (int ni = 0; ni < NPW; ni++) {
      const int nt = sp.nt_first + ni * sp.nt_step;
      if (nt < NT) {
#pragma unroll
        for (int j = 0; j < RPN; j++)
          if (j < nrt) {
            float *d = t + ((sp.rt_first + j * sp.rt_step) * 16 + 4 * (lane >> 4)) * LD + nt * 16 + (lane & 15);
#pragma unroll
            for (int i = 0; i < 4; i++) d[i * LD] = acc[ni * RPN + j][i];
          }
      }
    }
  }
  __syncthreads();
  const int q = F_out >> 2;  // four-column pieces per row: 8 bytes of Y
  for (int i = tid; i < nrows * q; i += 256) {
    const int r = i / q, c = (i - r * q) * 4;
    const int pr = rowmap[r];
    if (pr < 0) continue;
    float4 o = *reinterpret_cast<const float4 *>(t + r * LD + c);
    if (relu) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
    const uint2 ob = round_bf16x4(o);
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    u2 *dst = reinterpret_cast<u2 *>(Y + (int64_t)pr * F_out + c);
    if (y_nt) __builtin_nontemporal_store(u2{ob.x, ob.y}, dst);
    else *dst = u2{ob.x, ob.y};
  }
}

// WIDE = false: the caller guarantees the staged form applies (F_out <= K and few enough row tiles); the direct form
// for wider outputs is then not compiled in -- its registers would set the budget of the whole kernel.
template <int KSTEPS, bool WIDE = true>
__device__ __forceinline__ void panel_times_wt(float *t, int nrows, int F_out, const float *Wlin,
                                               const int32_t *rowmap, int64_t row0, float *Y, int tid,
                                               float (&bpre)[BPre<KSTEPS>::N], int relu) {
  constexpr int K = KSTEPS * 4, LD = K + 4;
  const int nt_all = F_out >> 4, nwr = nt_all >= 3 ? 1 : 4 / nt_all;  // as lin_split
  const int rt_per_wave = (((nrows + 15) >> 4) + nwr - 1) / nwr;
  if (!WIDE || (F_out <= K && rt_per_wave <= (F_out > 64 ? 2 : 4))) {  // workgroup-uniform
    if constexpr (KSTEPS >= 32) {
      if (F_out > 64) panel_times_wt_staged_chunked<KSTEPS, 2>(t, nrows, F_out, Wlin, rowmap, row0, Y, tid, bpre, relu);
      else panel_times_wt_staged_chunked<KSTEPS, 1>(t, nrows, F_out, Wlin, rowmap, row0, Y, tid, bpre, relu);
    } else {
      if (F_out > 64) panel_times_wt_staged<KSTEPS, 2>(t, nrows, F_out, Wlin, rowmap, row0, Y, tid, bpre, relu);
      else panel_times_wt_staged<KSTEPS, 1>(t, nrows, F_out, Wlin, rowmap, row0, Y, tid, bpre, relu);
    }
    return;
  }
  if constexpr (!WIDE) return;
  // wider output than input: results go straight to Y, 64 bytes per row and instruction
  const int lane = tid & 63;
  const int NT = F_out >> 4, RT = (nrows + 15) >> 4;
  const LinSplit sp = lin_split(tid >> 6, NT);
  if (!sp.active) return;
  auto store_tiles = [&](int nt, int rt, int n, const hg_f4 *acc) {
    float *ycol = Y + nt * 16 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j < n) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int r = (rt + j * sp.rt_step) * 16 + 4 * (lane >> 4) + i;
          if (r < nrows) ycol[(rowmap ? (int64_t)rowmap[r] : row0 + r) * F_out] = relu ? fmaxf(acc[j][i], 0.f) : acc[j][i];
        }
      }
  };
  if constexpr (KSTEPS >= 32) {  // K = 128: the chunked matrix phase here too (32 fragment registers would set the kernel's budget)
    for (int nt = sp.nt_first; nt < NT; nt += sp.nt_step) {
      float b0[8];
      if (nt == sp.nt_first) {
#pragma unroll
        for (int i = 0; i < 8; i++) b0[i] = bpre[i];
      } else {
        load_bfrag_chunk<KSTEPS>(Wlin, nt, 0, lane, b0);
      }
      LinSplit one = sp;
      one.nt_first = nt;
      for (int rt = sp.rt_first; rt < RT; rt += 2 * sp.rt_step) {  // two row tiles at a time: the register budget of the staged form
        const int n = min(2, (RT - rt + sp.rt_step - 1) / sp.rt_step);  // wave-uniform
        hg_f4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = hg_f4{0.f, 0.f, 0.f, 0.f};
        const float *ta = t + (rt * 16 + (lane & 15)) * LD + (lane >> 4);
        const int tstep = sp.rt_step * 16 * LD;
        if (n == 2) mfma_rows_chunked<KSTEPS, 1, 2>(ta, tstep, Wlin, one, NT, lane, b0, acc);
        else mfma_rows_chunked<KSTEPS, 1, 1>(ta, tstep, Wlin, one, NT, lane, b0, acc);
        store_tiles(nt, rt, n, acc);
      }
    }
  } else {
    float bv[KSTEPS];
    for (int nt = sp.nt_first; nt < NT; nt += sp.nt_step) {
      if (nt != sp.nt_first) load_bfrag<KSTEPS>(Wlin, nt, lane, bv);
      else {
#pragma unroll
        for (int i = 0; i < KSTEPS; i++) bv[i] = bpre[i];
      }
      // two row tiles per pass (four would make this path's 16 + 12 + KSTEPS live registers the kernel's budget)
      for (int rt = sp.rt_first; rt < RT; rt += 2 * sp.rt_step) {
        const int n = min(2, (RT - rt + sp.rt_step - 1) / sp.rt_step);  // wave-uniform
        hg_f4 acc[4];
        if (n == 2) mfma_rows<KSTEPS, 2>(t, LD, rt, sp.rt_step, bv, acc, lane);
        else mfma_rows<KSTEPS, 1>(t, LD, rt, sp.rt_step, bv, acc, lane);
        store_tiles(nt, rt, n, acc);
      }
    }
  }
}

// Standalone form: 64 (K = 128: 32) rows of T per workgroup through LDS.  Used where the
// aggregation did not run the fused panels (pull variant, hub vertices).
template <int KSTEPS> struct LinearRows {
  static constexpr int R = KSTEPS >= 32 ? 32 : 64;
};
template <int KSTEPS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KSTEPS >= 32 ? 6 : KSTEPS >= 16 ? kRowsWaves : 8, 8))) void linear_rows_kernel(
    const LinearArgs a) {
  constexpr int K = KSTEPS * 4, LD = K + 4, R = LinearRows<KSTEPS>::R;
  __shared__ float t[R * LD];
  const int64_t row0 = (int64_t)blockIdx.x * R;
  const int nrows = (int)min((int64_t)R, a.nrows - row0);
  float bv[BPre<KSTEPS>::N];
  const LinSplit sp = lin_split(threadIdx.x >> 6, a.F_out >> 4);
  if (sp.active) load_bfrag_pre<KSTEPS>(a.Wlin, sp.nt_first, threadIdx.x & 63, bv);
  constexpr int NL = R * (K / 4) / 256;  // float4 loads per thread, all in flight before the first LDS write
  float4 v[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) {
    const int i = threadIdx.x + j * 256, r = i / (K / 4), c = (i % (K / 4)) * 4;
    v[j] = r < nrows ? *reinterpret_cast<const float4 *>(a.T + (row0 + r) * K + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (a.epi.R || a.epi.ca != 1.f || a.epi.T_out) {  // t' = ca * t + cb * R[row]
    const float cb = a.epi.cb_dev ? *a.epi.cb_dev : a.epi.cb;  // uniform: one scalar load
    // row ids, then the rows of R, each set in flight together and unconditionally (a row past the end reads the block's last
    // one): inside the `r < nrows` branch below every load was followed by s_waitcnt vmcnt(0) -- 2 NL dependent round trips
    int64_t grow[NL];
    float4 rr[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) grow[j] = row0 + min((threadIdx.x + j * 256) / (K / 4), nrows - 1);
    if (a.rowmap) {
      int32_t m[NL];
#pragma unroll
      for (int j = 0; j < NL; j++) m[j] = a.rowmap[grow[j]];
#pragma unroll
      for (int j = 0; j < NL; j++) grow[j] = m[j];
    }
    if (a.epi.R) {
#pragma unroll
      for (int j = 0; j < NL; j++)
        rr[j] = *reinterpret_cast<const float4 *>(a.epi.R + grow[j] * K + ((threadIdx.x + j * 256) % (K / 4)) * 4);
    }
#pragma unroll
    for (int j = 0; j < NL; j++) {
      const int i = threadIdx.x + j * 256, r = i / (K / 4), c = (i % (K / 4)) * 4;
      if (r >= nrows) continue;
      float4 t4 = v[j];
      t4 = make_float4(t4.x * a.epi.ca, t4.y * a.epi.ca, t4.z * a.epi.ca, t4.w * a.epi.ca);
      if (a.epi.R) t4 = make_float4(t4.x + rr[j].x * cb, t4.y + rr[j].y * cb, t4.z + rr[j].z * cb, t4.w + rr[j].w * cb);
      if (a.epi.T_out) *reinterpret_cast<float4 *>(a.epi.T_out + grow[j] * K + c) = t4;
      v[j] = t4;
    }
  }
#pragma unroll
  for (int j = 0; j < NL; j++) {
    const int i = threadIdx.x + j * 256, r = i / (K / 4), c = (i % (K / 4)) * 4;
    *reinterpret_cast<float4 *>(t + r * LD + c) = v[j];
  }
  __syncthreads();
  panel_times_wt<KSTEPS>(t, nrows, a.F_out, a.Wlin, a.rowmap ? a.rowmap + row0 : nullptr, row0, a.Y,
                         threadIdx.x, bv, a.epi.relu);
}

// ---- bf16 rows times Wb^T (hg_linear_rows_bf16; the rows hg_aggr_linear_res_bf16's panels do not take) -----------------
// Wb [F_out, F_in] bf16 in fragment order, linear_pack_split_kernel's layout with one plane and F_in / 32 k-steps:
//   wfrag[(nt * K/32 + ks) * 64 + lane] = 8 bf16: Wb[nt*16 + (lane & 15)][ks*32 + 8*(lane >> 4) + j]
__global__ __launch_bounds__(256) void linear_pack_bf16_kernel(int32_t F_out, int32_t F_in, const uint16_t *Wlin, uint4 *wfrag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (nt, ks, lane)
  const int k32 = F_in >> 5;
  if (i >= (int64_t)(F_out >> 4) * k32 * 64) return;
  const int lane = (int)(i & 63), ks = (int)((i >> 6) % k32), nt = (int)((i >> 6) / k32);
  const uint16_t *w = Wlin + (int64_t)(nt * 16 + (lane & 15)) * F_in + ks * 32 + 8 * (lane >> 4);
  unsigned u[4];
#pragma unroll
  for (int j = 0; j < 4; j++) u[j] = (unsigned)w[2 * j] | ((unsigned)w[2 * j + 1] << 16);
  wfrag[i] = make_uint4(u[0], u[1], u[2], u[3]);
}

// A wave owns 16 rows and computes the TRANSPOSED tiles, D = Wb_tile . t^T: the weight fragment is the A operand, the wave's
// rows the B operand -- both maps put 8 consecutive k of row (lane & 15) in a lane, so a row's fragment is 16 contiguous
// bytes of it, loaded straight from memory (no LDS, no barrier), and lane l ends up with FOUR CONSECUTIVE COLUMNS
// 16 nt + 4 (l >> 4) .. + 3 of row l & 15: one 8-byte store per column tile.  The K/32 row fragments stay in registers for
// every column tile; the tiles' weight fragments come from the L2 (NB tiles in flight).  fp32 accumulation, k-steps in
// ascending order: the bits depend on the widths only.
// TF32: T holds fp32 rows (the aggregation's workspace); t = round_bf16(ca * T + cb * R) formed as the panels form it
// (separate fp32 operations), rounded once, written to T_out where wanted.
typedef unsigned hg_u4a8 __attribute__((ext_vector_type(4), aligned(8)));  // rows of the bf16 entries are 8-byte aligned
template <int KS, bool TF32>
__global__ __launch_bounds__(256) void linear_rows_bf16_kernel(const LinearB16Args a) {
  constexpr int K = KS * 32, NB = KS == 4 ? 2 : 4;
  const int lane = threadIdx.x & 63, kb = lane >> 4;
  const int64_t i0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
  if (i0 >= a.nrows) return;  // wave-uniform; the kernel has no barrier
  const bool row_ok = i0 + (lane & 15) < a.nrows;
  const int64_t ri = min(i0 + (lane & 15), a.nrows - 1);  // a row past the end repeats the last one and stores nothing
  const int64_t row = a.rowmap ? (int64_t)a.rowmap[ri] : ri;
  const uint4 *wb = static_cast<const uint4 *>(a.wfrag);
  uint4 tf[KS];
  if constexpr (TF32) {
    const float *tp = static_cast<const float *>(a.T) + row * K + 8 * kb;
    float4 lo[KS], hi[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      lo[ks] = *reinterpret_cast<const float4 *>(tp + ks * 32);
      hi[ks] = *reinterpret_cast<const float4 *>(tp + ks * 32 + 4);
    }
    hg_u4a8 rb[KS];
    if (a.R) {
#pragma unroll
      for (int ks = 0; ks < KS; ks++) rb[ks] = *reinterpret_cast<const hg_u4a8 *>(a.R + row * K + ks * 32 + 8 * kb);
    }
    const bool comb = a.R || a.ca != 1.f;  // as the fp32 entry: t' = ca * t + cb * R only where asked for
    const float cb = a.R ? (a.cb_dev ? *a.cb_dev : a.cb) : 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      float v[8] = {lo[ks].x, lo[ks].y, lo[ks].z, lo[ks].w, hi[ks].x, hi[ks].y, hi[ks].z, hi[ks].w};
      if (comb) {
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] *= a.ca;
        if (a.R) {
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const unsigned w = rb[ks][e];
            const float r0 = __uint_as_float(w << 16) * cb, r1 = __uint_as_float(w & 0xffff0000u) * cb;
            v[2 * e] += r0;
            v[2 * e + 1] += r1;
          }
        }
      }
      tf[ks] = make_uint4(round_bf16x2(v[0], v[1]), round_bf16x2(v[2], v[3]), round_bf16x2(v[4], v[5]), round_bf16x2(v[6], v[7]));
      if (a.T_out && row_ok)
        *reinterpret_cast<hg_u4a8 *>(a.T_out + row * K + ks * 32 + 8 * kb) = hg_u4a8{tf[ks].x, tf[ks].y, tf[ks].z, tf[ks].w};
    }
  } else {
    const bf16 *tp = static_cast<const bf16 *>(a.T) + row * K + 8 * kb;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      const hg_u4a8 u = *reinterpret_cast<const hg_u4a8 *>(tp + ks * 32);
      tf[ks] = make_uint4(u.x, u.y, u.z, u.w);
    }
  }
  const int NT = a.F_out >> 4;
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  for (int nt0 = 0; nt0 < NT; nt0 += NB) {
    uint4 b[NB][KS];
#pragma unroll
    for (int n = 0; n < NB; n++)
#pragma unroll
      for (int ks = 0; ks < KS; ks++) b[n][ks] = wb[((int64_t)min(nt0 + n, NT - 1) * KS + ks) * 64 + lane];  // past the last tile: clamped, not stored
    hg_f4 acc[NB];
#pragma unroll
    for (int n = 0; n < NB; n++) acc[n] = hg_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ks++)
#pragma unroll
      for (int n = 0; n < NB; n++) acc[n] = mfma_bf16(b[n][ks], tf[ks], acc[n]);
#pragma unroll
    for (int n = 0; n < NB; n++)
      if (nt0 + n < NT && row_ok) {
        float4 o = make_float4(acc[n][0], acc[n][1], acc[n][2], acc[n][3]);
        if (a.relu) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
        const uint2 ob = round_bf16x4(o);
        u2 *dst = reinterpret_cast<u2 *>(a.Y + row * a.F_out + (nt0 + n) * 16 + 4 * kb);
        if (a.y_nt) __builtin_nontemporal_store(u2{ob.x, ob.y}, dst);
        else *dst = u2{ob.x, ob.y};
      }
  }
}

// ---- weight gradient of the layer's linear: C[Fa, Fb] = A^T B over N rows --------------------
// dWlin = dP^T T (and HGNN's dZ^T X): a product whose contraction runs over the N vertices.  rocBLAS
// spends 1.24 ms on [64 x 693 k] x [693 k x 64] (47 % of a UniGCNII training epoch) where reading
// both operands once takes 0.07 ms.  Here every wave streams its share of the rows straight into
// MFMA operands -- lane l holds A[n + (l>>4)][16 i + (l&15)] and B[n + (l>>4)][16 j + (l&15)], the
// 16x16x4 layout with k = 4 consecutive rows -- so each element is loaded exactly once, and keeps
// all TA x TB output tiles in accumulators; waves are reduced through LDS in wave order,
// workgroups through one partial matrix each and a second kernel (fixed order: deterministic).
template <int TA, int TB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TA * TB >= 16 ? 3 : TA * TB >= 8 ? 4 : 1, 8))) void wgrad_kernel(const float *A, const float *B, float *partial, int64_t N,
                                                    int64_t rows_per_wg, int lda, int ldb, int nbb, int nblocks, int nparts) {
  constexpr int FA = TA * 16, FB = TB * 16;
  // A wider product (lda, ldb = the operands' row strides) runs as nblocks independent FA x FB blocks of C over the same rows.
  // The blocks of one row range (part) are dealt to the SAME XCD, eight workgroup ids apart -- dispatched together, so the
  // second read of an operand's half rows is an L2 hit instead of a second trip to HBM: workgroup id = xcd + 8 (nblocks q + b)
  // for part 8 q + xcd, block b (nparts a multiple of 8 then, launcher).
  int part = blockIdx.x, blk = 0;
  if (nblocks > 1) {
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    blk = k % nblocks;
    part = (k / nblocks) * 8 + xcd;
  }
  A += (blk / nbb) * FA;
  B += (blk % nbb) * FB;
  __shared__ float red[FA * FB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kk = lane >> 4, c = lane & 15;
  const int64_t wg0 = min(N, (int64_t)part * rows_per_wg);
  const int64_t wg1 = min(N, wg0 + rows_per_wg);
  const int64_t per_wave = (rows_per_wg / 4 + 3) & ~(int64_t)3;  // multiple of 4 rows
  const int64_t r0 = min(wg1, wg0 + wave * per_wave), r1 = min(wg1, r0 + per_wave);
  hg_f4 acc[TA][TB];
#pragma unroll
  for (int i = 0; i < TA; i++)
#pragma unroll
    for (int j = 0; j < TB; j++) acc[i][j] = hg_f4{0.f, 0.f, 0.f, 0.f};
  float a0[TA], b0[TB], a1[TA], b1[TB];
  // Lane (kk, c) holds TA CONSECUTIVE floats of row n + kk -- columns TA c .. TA c + TA - 1, one 16-byte load at TA = 4 --
  // and feeds the i-th of them to tile i: tile i then stands for the columns {TA c + i}, a permutation of the output's rows
  // (columns for B) that the reduction below undoes.  Sixteen lanes read one whole 4 TA-float segment of a row per
  // instruction; with tile i = columns 16 i .. 16 i + 15 (round 1) every row was fetched as TA separate 64-byte pieces.
  // Every load is issued unconditionally and unmasked, from a row clamped into the wave's range; only the last, partial step of
  // a range (N not a multiple of four) zeroes the rows past the end, after the loop.  With the loads under `if (row < r1)`
  // branches the compiler could not count them and put s_waitcnt vmcnt(0) in front of every step's MFMAs -- each step then
  // waited for the loads it had just issued, the whole HBM latency per four rows (the kernel ran at half the rate its matrix
  // pipe allows); a select on the loaded value has the same effect (it consumes the value at once).
  auto load = [&](int64_t n, float (&a)[TA], float (&b)[TB]) {
    const int64_t row = min(n + kk, r1 - 1);  // r1 > r0 >= 0 where this is called
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
    auto fetch = [&](const float *p, auto &dst, auto nt) {
      constexpr int T = decltype(nt)::value;
      if constexpr (T % 4 == 0) {
#pragma unroll
        for (int q = 0; q < T / 4; q++) {
          const f4u v = *reinterpret_cast<const f4u *>(p + 4 * q);
          dst[4 * q] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w;
        }
      } else if constexpr (T == 2) {
        const f2u v = *reinterpret_cast<const f2u *>(p);
        dst[0] = v.x; dst[1] = v.y;
      } else {
#pragma unroll
        for (int q = 0; q < T; q++) dst[q] = p[q];
      }
    };
    fetch(A + row * lda + c * TA, a, std::integral_constant<int, TA>{});
    fetch(B + row * ldb + c * TB, b, std::integral_constant<int, TB>{});
  };
  auto step = [&](const float (&a)[TA], const float (&b)[TB]) {
#pragma unroll
    for (int i = 0; i < TA; i++)
#pragma unroll
      for (int j = 0; j < TB; j++)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
  };
  // Three operand buffers in rotation, the loop unrolled by three so that the rotation is a renaming: with register moves
  // (a0 = a1, a1 = a2) the move out of the buffer just loaded waited for that load at the end of every step.
  float a2[TA], b2[TB];
  if (r0 < r1) {
    const int64_t rfull = r0 + ((r1 - r0) & ~(int64_t)3);  // whole steps of four rows
    load(r0, a0, b0);
    load(r0 + 4, a1, b1);
    int64_t n = r0;
    for (; n + 12 <= rfull; n += 12) {  // two steps (eight rows) in flight behind every step's MFMAs
      // (scheduling barriers: left alone the compiler sinks a step's loads behind the wait for the step before)
      load(n + 8, a2, b2);
      __builtin_amdgcn_sched_barrier(0);
      step(a0, b0);
      __builtin_amdgcn_sched_barrier(0);
      load(n + 12, a0, b0);
      __builtin_amdgcn_sched_barrier(0);
      step(a1, b1);
      __builtin_amdgcn_sched_barrier(0);
      load(n + 16, a1, b1);
      __builtin_amdgcn_sched_barrier(0);
      step(a2, b2);
      __builtin_amdgcn_sched_barrier(0);
    }
    // zero to two whole steps and the range's last one to three rows (clamped duplicates beside them: zeroed here)
    auto tail = [&](float (&a)[TA], float (&b)[TB], int64_t at) {
      if (at >= r1) return;
      const bool ok = at + kk < r1;
#pragma unroll
      for (int i = 0; i < TA; i++) a[i] = ok ? a[i] : 0.f;
#pragma unroll
      for (int j = 0; j < TB; j++) b[j] = ok ? b[j] : 0.f;
      step(a, b);
    };
    if (n + 8 <= rfull) {
      load(n + 8, a2, b2);
      step(a0, b0);
      step(a1, b1);
      tail(a2, b2, n + 8);
    } else if (n + 4 <= rfull) {
      step(a0, b0);
      tail(a1, b1, n + 4);
    } else {
      tail(a0, b0, n);
    }
  }
  // D layout: register q of tile (i, j) is tile row 4 (lane >> 4) + q, tile column lane & 15, i.e. (the load's permutation)
  // C[TA (4 (lane >> 4) + q) + i][TB (lane & 15) + j]
  for (int w = 0; w < 4; w++) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < TA; i++)
#pragma unroll
        for (int j = 0; j < TB; j++)
#pragma unroll
          for (int q = 0; q < 4; q++) {
            float *d = red + (TA * (4 * kk + q) + i) * FB + TB * c + j;
            *d = w == 0 ? acc[i][j][q] : *d + acc[i][j][q];
          }
    }
    __syncthreads();
  }
  float *out = partial + ((int64_t)blk * nparts + part) * FA * FB;
  for (int i = threadIdx.x; i < FA * FB; i += 256) out[i] = red[i];
}

// out[c * n + i] = sum over parts p = c, c + nchunks, c + 2 nchunks, ... of partial[p * n + i]
// (blockIdx.y = c).  Run twice -- nparts -> 32 chunks -> 1 -- so that the sum over a thousand
// partial matrices is spread over 512 workgroups instead of sixteen.
// blockIdx.z = block of a blocked product (its partials follow the previous block's; nbb blocks per block row of C).
// fb > 0 (last level): element i of block z goes to out[((z / nbb) * fa + i / fb) * ldc + (z % nbb) * fb + i % fb]; else to the
// block's own run of nchunks * n second-level partials.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *partial, int nparts, int n, float *out, int fa, int fb, int ldc, int nbb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = blockIdx.y, nchunks = gridDim.y, z = blockIdx.z;
  partial += (int64_t)z * nparts * n;
  float s = 0.f;
  for (int p = c; p < nparts; p += nchunks) s += partial[(int64_t)p * n + i];
  if (fb > 0) out[(int64_t)((z / nbb) * fa + i / fb) * ldc + (z % nbb) * fb + (i % fb)] = s;
  else out[((int64_t)z * nchunks + c) * n + i] = s;
}

// Packed form of the fused panel kernel.  The plan hands every panel over as ONE
// contiguous int32 record (hg_fused.cpp, pack_records): a single coalesced copy
// stages it, and hop 1 is a wave-uniform loop over a [step][group] entry stream in
// which the panel's hyperedge slots were packed longest-first over the lane
// groups -- no per-group offsets to look up, no divergent trip counts, the same
// number of row gathers for every group.  Entry word: N (one past the last row of
// X, no flags) = idle, else bits 0..29 =
// row, bit 30 = row of the materialised table, bit 31 = last member of its slot
// (scale, store to the LDS tile, start the next slot).  Members of a slot stay in
// their CSR order, so the arithmetic is still the CPU reference's.
// Waves per SIMD the LIN instances (panel kernel + matrix phase) are compiled for, by lanes per row: the register
// budget that follows (512 / waves) decides how much of hop 2's row registers and the B fragments spill.  Measured
// (tools/linear_probe.py, cora x1024): F = 32 -> 32: 8 waves 0.262 ms, 7 0.258, 6 0.236, 5 0.249; 64 -> 64: 8 waves
// 0.621, 7 0.539, 6 0.507, 5 0.529, 4 0.532; 128 -> 128 (x256): 6 waves 0.739 (spills), 5 0.370, 4 0.388.
constexpr int kLinWaves8 = 8, kLinWaves16 = 6, kLinWaves32 = 5, kLinWavesStaged = 8;
// K = 128 staged-only instances: the register budget of six waves per SIMD, which is what the LDS tile of the epilogue's
// schedule allows anyway (48 slots x 132 floats + record = 26.6 KB: six workgroups per CU); it pays for twelve row
// gathers in flight per lane (kLinU32) -- most panels' hop 1 is then one round trip (both phases merged, below)
constexpr int kLinWavesStaged32 = 6;
constexpr int kLinU32 = 12;  // row gathers in flight per lane, K = 128 staged instances
typedef unsigned hg_u4 __attribute__((ext_vector_type(4)));
typedef int hg_i4 __attribute__((ext_vector_type(4)));

// Floats of the linear epilogue's tile region: cap slot rows of tw floats in hops 1 and 2, then the operand rows of the
// matrix phase (the panel's rows, whole 16-row tiles, stride tw + 4).  A multiple of four floats (16-byte aligned record).
__host__ __device__ inline int lin_tile_floats(int cap, int rows_cap, int tw) {
  const int rows16 = (rows_cap + 15) / 16 * 16;
  const int a = cap * tw, b = rows16 * (tw + 4);
  return a > b ? a : b;
}

// FAST: rows are fetched with buffer_load_dwordx4 (VEC = 1: buffer_load_dword) through a buffer
// descriptor and a 32-bit byte offset formed by one v_mad_u32_u24 (row * row_bytes +
// column bytes) instead of 64-bit pointer arithmetic; needs N < 2^24, F*4 < 2^24 and
// tables below 2 GiB (the launcher checks; otherwise FAST = false runs the same loop
// on global loads).
// MAT / SCALED say whether materialised slots / degE-W scaling can occur at all (the launcher
// knows); false compiles that path out of the unrolled loop, which is issue-bound.
// LIN: the rows a panel produces go through panel_times_wt (Y = rows * Wlin^T, F_out columns)
// instead of straight to Y; needs F == LPR * VEC and at most 4 rows per lane group.
// BS: threads per panel workgroup.  256 everywhere but for a tiny dense hypergraph, whose whole hop-1 stream sits in one
// panel whatever the panel count: 1024 threads then (four times the lane groups, a quarter of the dependent steps).
// For batches, 512- / 1024-thread workgroups with two / four times the tile (the panel shape of F = 32 for rows of 64
// and 128 floats, same waves and LDS per CU) were 3-9 % slower on every wide-row batch (profiles/r03_experiments.md).
// LINW (LIN only): the output may be wider than the input, or a panel hold more row tiles than the staged matrix phase
// takes -- the direct form is compiled in.  LINW = false instances (F_out <= F, the common case) carry the staged form
// only and fit 8 waves per SIMD without spills; the direct form's registers used to set the budget of every LIN
// instance (natural demand 85-92 VGPRs, 5-6 waves).
// SPLIT (LIN, !LINW, K = 128 only): the matrix phase as six bf16 products per fp32 product (mfma_rows_split); a.epi.wsplit.
// T: element type of the rows of X and Y (Rows; bf16 without LIN only).  Tile, materialised rows and partial rows are fp32.
// BLIN (T = bf16, LIN, !LINW, K = 128): the native bf16 epilogue of hg_aggr_linear_res_bf16 -- the combined row is rounded to bf16
// once, the same bits go to T_out and into ONE operand plane, and the matrix phase is one bf16 MFMA per (k-step, row tile,
// column tile) (panel_times_wt_b16); a.Wlin holds the bf16 fragments, a.epi.R / a.epi.T_out / a.Y point at bf16 rows.  Unlike the
// fp32 epilogue it takes panels with pieces of split vertices: a piece's sum goes to its partial row and gets no epilogue.
// TY: element type of the rows of Y where it is not T's (bf16 X, fp32 Y: the aggregated rows on their way to
// linear_rows_bf16_kernel); never with LIN.
template <int LPR, int VEC, int U, bool FAST, bool MAT, bool SCALED, bool LIN = false, int BS = 256, bool LINW = true, bool SPLIT = false,
          typename T = float, bool BLIN = false, typename TY = T>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(LIN ? (!LINW ? (LPR >= 32 ? kLinWavesStaged32 : kLinWavesStaged) : LPR >= 32 ? kLinWaves32 : LPR == 16 ? kLinWaves16 : kLinWaves8) : 1, 8))) void fused_packed_kernel(const FusedArgs a) {
  static_assert(!LIN || BS == 256, "the linear epilogue is written for four waves");
  static_assert(!SPLIT || (LIN && !LINW && LPR == 32 && VEC == 4), "bf16x6 matrix phase: K = 128 staged instances");
  static_assert(!LIN || std::is_same_v<T, float> || BLIN, "the fp32 linear epilogue takes fp32 rows");
  static_assert(!BLIN || (LIN && !LINW && !SPLIT && LPR == 32 && VEC == 4 && std::is_same_v<T, bf16>), "bf16 epilogue: K = 128 staged instances on bf16 rows");
  static_assert(std::is_same_v<TY, T> || (!LIN && std::is_same_v<TY, float>), "rows of Y: T's type, or fp32 without an epilogue");
  constexpr bool XF32 = std::is_same_v<T, float>;
  constexpr bool YF32 = std::is_same_v<TY, float>;
  constexpr int NG = BS / LPR;
  constexpr int TW = LPR * VEC;
  using V = Vec<VEC>;
  using RX = Rows<T, VEC>;
  extern __shared__ int32_t smem[];
  const int64_t F = a.F;
  const int tid = threadIdx.x;
  const int gl = tid & (LPR - 1);
  const int lcol = gl * VEC;
  const int col = blockIdx.y * TW + lcol;
  const bool col_ok = col < a.F;
  int b = blockIdx.x;
  if (a.xcd_remap) {
    // workgroups are dealt round-robin to the 8 XCDs; give each XCD one contiguous run of panels so that neighbouring
    // panels share an L2
    const int x = b & 7;
    int i = b >> 3;
    const int cpx = a.npanels >> 3, rem = a.npanels & 7;
    // After a substantial materialisation pre-pass each XCD walks its run of panels backwards: the pre-pass walked the
    // hyperedges forwards, so the member rows it read last -- still in the L2 / Infinity Cache -- are the ones the
    // panels ask for first (pubmed-shape batches at F = 64 .. 128: -2 .. -3.6 % per step; neutral elsewhere).
    if (MAT && a.reverse_runs) i = cpx + (x < rem ? 1 : 0) - 1 - i;
    b = x * cpx + (x < rem ? x : rem) + i;
  }

  // [cap * TW] slot rows; LIN: the same floats later hold the matrix phase's operand, [rows_cap up to whole 16-row tiles]
  // rows of TW + 4 floats -- the region is the larger of the two (lin_tile_floats: the launcher sizes it the same way)
  float *tile = reinterpret_cast<float *>(smem);
  int32_t *rec = smem + (LIN ? lin_tile_floats(a.cap, a.rows_cap, TW) : a.cap * TW);  // [max_rec_words], 16-byte aligned
  // scale staging exists only for the scales this call has (fused_scale_floats: the launcher sizes LDS the same way)
  float *sA = reinterpret_cast<float *>(rec + a.max_rec_words);  // [cap], if degE
  float *sB = sA + (a.degE ? a.cap : 0);                 // [cap], if W
  float *sdeg = sB + (a.W ? a.cap : 0);                  // [rows_cap], if degV and not kept in registers (below)

  const FRec rt = a.rec_tab[b];
  const int32_t *grec = a.rec + rt.off;
  const int g = tid / LPR;
  // Bound degV, at most four rows per lane group, and the launcher found that the row factors' LDS costs a resident
  // workgroup (a.dv_regs, fused_dv_regs): the lane group's four factors travel in registers from the start instead.  Those
  // 512 bytes decide whether the weighted headline batch fits eight workgroups per CU or seven (20 112 against 20 624
  // bytes per workgroup, 163 840 per CU).  SCALED instances only: the unweighted instance's code is untouched.
  const bool dv_regs = SCALED && a.dv_regs != 0;
  [[maybe_unused]] float dv[4] = {1.f, 1.f, 1.f, 1.f};
  if constexpr (SCALED) {
    if (dv_regs) {
      const int rpg0 = (rt.nrows + NG - 1) / NG;
      const int q0 = min(g * rpg0, rt.nrows), q1 = min(q0 + rpg0, rt.nrows);
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (q0 + i < q1) dv[i] = a.bsD[rt.row_base + q0 + i];
    }
  }

  // Staging of the record and of the call's scales.  Everything a thread stages first -- its 16 bytes of the record (records are
  // padded to whole 16-byte units: one dwordx4 per lane copies 4 KB per pass), its slot's bound degE / W factors, its row's
  // bound degV -- is REQUESTED before anything is written to LDS, from indices clamped into range so that no load sits under a
  // lane-dependent branch: written as one loop after the other, each loop's load was followed by s_waitcnt vmcnt(0) and its LDS
  // write, i.e. up to four dependent round trips to memory (record, degE, W, degV) before a weighted panel's first barrier where
  // one suffices.  The loops below take what is left (records beyond 4 KB, unbound scales: an id first, then the factor).
  // An unweighted call has one thing to stage and keeps its plain loop (the clamped form cost the pubmed-shape F = 128 batch 4 %).
  const int nrec4 = rt.len >> 2;  // >= 1: a record has its header
  const hg_i4 *grec4 = reinterpret_cast<const hg_i4 *>(grec);
  const bool bound_e = SCALED && a.bsA && (a.degE || a.W) && rt.nslots > 0, bound_v = a.degV && !dv_regs && a.bsD && rt.nrows > 0;
  const bool pre = bound_e || bound_v;  // workgroup-uniform
  if (pre) {
    const hg_i4 rv = grec4[min(tid, nrec4 - 1)];
    float va = 1.f, vb = 1.f, vd = 1.f;
    if (bound_e) {
      const int64_t si = rt.slot_base + min(tid, rt.nslots - 1);
      if (a.degE) va = a.bsA[si];
      if (a.W) vb = a.bsB[si];
    }
    if (bound_v) vd = a.bsD[rt.row_base + min(tid, rt.nrows - 1)];
    if (tid < nrec4) reinterpret_cast<hg_i4 *>(rec)[tid] = rv;
    if (bound_e && tid < rt.nslots) {
      if (a.degE) sA[tid] = va;
      if (a.W) sB[tid] = vb;
    }
    if (bound_v && tid < rt.nrows) sdeg[tid] = vd;
  }
  for (int i = pre ? tid + BS : tid; i < nrec4; i += BS)
    reinterpret_cast<hg_i4 *>(rec)[i] = grec4[i];
  if (a.degE || a.W)
    for (int i = bound_e ? tid + BS : tid; i < rt.nslots; i += BS) {
      if (a.bsA) {  // bound: one coalesced read instead of a scattered 4-byte gather per slot
        if (a.degE) sA[i] = a.bsA[rt.slot_base + i];
        if (a.W) sB[i] = a.bsB[rt.slot_base + i];
      } else {
        const int e = a.eid_all[rt.slot_base + i];  // -1: materialised row, already scaled
        if (a.degE) sA[i] = e >= 0 ? a.degE[e] : 1.f;
        if (a.W) sB[i] = e >= 0 ? a.W[e] : 1.f;
      }
    }
  if (a.degV && !dv_regs)
    for (int i = bound_v ? tid + BS : tid; i < rt.nrows; i += BS) {
      if (a.bsD) {
        sdeg[i] = a.bsD[rt.row_base + i];
      } else {
        const int pr = grec[rt.off_prow + i];  // bit 31: a piece of a split vertex, scaled by its fixup
        sdeg[i] = pr < 0 ? 1.f : a.degV[pr];
      }
    }
  __syncthreads();
  const int steps = rec[0], nrows = rec[1];
  const int32_t *gbase = rec + rec[4];
  const int32_t *stream = rec + rec[5];
  const uint16_t *pend = reinterpret_cast<const uint16_t *>(rec + rec[6]);
  const int32_t *prow = rec + rec[7];
  const uint16_t *pvs = reinterpret_cast<const uint16_t *>(rec + rec[9]);

  {  // ---- hop 1
    [[maybe_unused]] int slot = gbase[g];
    float *tp = tile + gbase[g] * TW + lcol;  // where this group's next finished slot goes
    V acc = V::zero();
    // FAST: nothing in the gather is predicated.  An idle entry names row N, one past the
    // table, and a lane whose columns lie beyond F gets bit 31 in its column offset: both
    // byte offsets fall outside the descriptor's range (tables are < 2 GiB here), and an
    // out-of-range buffer load returns zeros without touching memory.
    [[maybe_unused]] const unsigned row_bytes = (unsigned)a.F * 4u;
    [[maybe_unused]] const unsigned col_off = col_ok ? (unsigned)col * 4u : 0x80000000u;
    // bf16 rows of X: the same offsets at the element size (the materialised table stays fp32)
    [[maybe_unused]] const unsigned xrow_bytes = (unsigned)a.F * (unsigned)sizeof(T);
    [[maybe_unused]] const unsigned xcol_off = col_ok ? (unsigned)col * (unsigned)sizeof(T) : 0x80000000u;
    [[maybe_unused]] const T *X = static_cast<const T *>(a.X);
    [[maybe_unused]] __amdgpu_buffer_rsrc_t rx, rm;
    if constexpr (FAST) {
      rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.X), 0, a.x_bytes, 0x00020000);
      rm = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.Xe_mat ? static_cast<const void *>(a.Xe_mat) : a.X), 0,
                                             a.Xe_mat ? a.mat_bytes : 0, 0x00020000);
    }
    // The stream has two phases (pack_stream, hg_fused.cpp): steps [0, steps_x) gather member rows of X,
    // steps [steps_x, steps) rows of the materialised table -- one buffer descriptor per phase, no
    // per-entry test.  FULL: all U steps of the block exist, so the entry reads need no bounds test.
    auto block = [&](const int s0, const int send, auto full, auto matph) {
      constexpr bool FULL = decltype(full)::value;
      constexpr bool MATPH = decltype(matph)::value;
      const int idle = MATPH ? a.nrows_mat : a.nrows_x;
      int ent[U];
#pragma unroll
      for (int j = 0; j < U; j++) ent[j] = (FULL || s0 + j < send) ? stream[(s0 + j) * NG + g] : idle;
      V v[U];
#pragma unroll
      for (int j = 0; j < U; j++) {
        if (!FULL && s0 + j >= send) {  // wave-uniform: no load is issued for a step that is not there
          v[j] = V::zero();
          continue;
        }
        if constexpr (FAST && !XF32 && !MATPH) {
          v[j] = RX::load_buf(rx, __umul24((unsigned)ent[j], xrow_bytes) + xcol_off);
        } else if constexpr (FAST) {
          const unsigned off = __umul24((unsigned)ent[j], row_bytes) + col_off;  // flags sit above bit 23
          v[j] = V::load_buf(MATPH ? rm : rx, off);
        } else if constexpr (!XF32 && !MATPH) {
          const bool on = col_ok && ent[j] != idle;
          const int64_t idx = ent[j] & 0x3fffffff;
          v[j] = on ? RX::load(X + idx * F + col) : V::zero();
        } else {
          const bool on = col_ok && ent[j] != idle;
          const int64_t idx = ent[j] & 0x3fffffff;
          const float *base = MATPH ? a.Xe_mat : static_cast<const float *>(a.X);
          v[j] = on ? V::load(base + idx * F + col) : V::zero();
        }
      }
#pragma unroll
      for (int j = 0; j < U; j++) {
        acc.add(v[j]);      // an idle step contributed zeros
        if (ent[j] < 0) {   // bit 31: last member of this slot
          if constexpr (SCALED) {
            if (a.degE) acc.mul(sA[slot]);
            if (a.W) acc.mul(sB[slot]);
            slot++;
          }
          acc.store(tp);
          tp += TW;
          acc = V::zero();
        }
      }
    };
    const int steps_x = MAT ? rec[8] : steps;
    // Both phases in ONE run of batches, the descriptor picked per step (wave-uniform): a pubmed-shape panel of the
    // epilogue's schedule has ~7 steps of X rows and ~4 of materialised rows -- two dependent round trips as two
    // phases, one as a batch of twelve.  The plain panels with materialised slots run it with batches of eight: a
    // panel's last X batch and its materialised rows share a round trip.  Measured on one box, three rounds each: K = 128
    // staged epilogue instances (twelve gathers in flight at the six-wave budget) -1.2 % on pubmed x64 128 -> 128, -2.2 % on
    // 128 -> 64; plain panels pubmed x256 F = 32 0.512-0.515 -> 0.526-0.529 of the roofline, x64 F = 128 0.502-0.503 ->
    // 0.507-0.510, weighted pubmed 0.494-0.496 -> 0.505-0.510, power-law step 0.917-0.921 -> 0.907-0.912 ms.
    if constexpr (MAT && FAST && ((LIN && !LINW && LPR >= 32) || (!LIN && VEC == 4 && BS == 256))) {
      auto mixed = [&](const int s0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        int ent[U];
#pragma unroll
        for (int j = 0; j < U; j++) ent[j] = (FULL || s0 + j < steps) ? stream[(s0 + j) * NG + g] : 0;
        V v[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
          if (!FULL && s0 + j >= steps) {  // wave-uniform: no load is issued for a step that is not there
            v[j] = V::zero();
            continue;
          }
          const unsigned off = __umul24((unsigned)ent[j], row_bytes) + col_off;  // flags sit above bit 23
          if (s0 + j >= steps_x) v[j] = V::load_buf(rm, off);  // wave-uniform
          else if constexpr (XF32) v[j] = V::load_buf(rx, off);
          else v[j] = RX::load_buf(rx, __umul24((unsigned)ent[j], xrow_bytes) + xcol_off);
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
          acc.add(v[j]);
          if (ent[j] < 0) {
            if constexpr (SCALED) {
              if (a.degE) acc.mul(sA[slot]);
              if (a.W) acc.mul(sB[slot]);
              slot++;
            }
            acc.store(tp);
            tp += TW;
            acc = V::zero();
          }
        }
      };
      int s0 = 0;
      for (; s0 + U <= steps; s0 += U) mixed(s0, std::true_type{});
      if (s0 < steps) mixed(s0, std::false_type{});
    } else {
      int s0 = 0;
      for (; s0 + U <= steps_x; s0 += U) block(s0, steps_x, std::true_type{}, std::false_type{});
      if (s0 < steps_x) block(s0, steps_x, std::false_type{}, std::false_type{});
      if constexpr (MAT) {
        for (s0 = steps_x; s0 + U <= steps; s0 += U) block(s0, steps, std::true_type{}, std::true_type{});
        if (s0 < steps) block(s0, steps, std::false_type{}, std::true_type{});
      }
    }
  }
  __syncthreads();
  if constexpr (BLIN) {  // ---- hop 2 into registers, one rounding to bf16, then rows * Wb^T on the bf16 MFMA
    const uint4 *wb = reinterpret_cast<const uint4 *>(a.Wlin);
    const T *Rb = reinterpret_cast<const T *>(a.epi.R);
    T *Tb = reinterpret_cast<T *>(a.epi.T_out);
    const int NT = a.F_out >> 4;
    const LinSplit sp = lin_split(tid >> 6, NT);
    uint4 bq[kB16Depth];  // the first steps' B fragments: in flight during hop 2
    if (sp.active) {
#pragma unroll
      for (int t = 0; t < kB16Depth; t++) bq[t] = load_b16_step(wb, sp, NT, a.F_out > 64 ? 2 : 1, t, tid & 63);
    }
    const int rpg = (nrows + NG - 1) / NG;  // <= 4 (launcher)
    const int r0 = min(g * rpg, nrows), r1 = min(r0 + rpg, nrows);
    int pr[4];  // vertex id, or bit 31 | partial row; a row past the group's range repeats the panel's last row and is not used
#pragma unroll
    for (int i = 0; i < 4; i++) pr[i] = prow[min(r0 + i, nrows - 1)];
    V rr[4];  // the residual rows, bf16, before hop 2 as in the fp32 epilogue (a piece has none: row 0 is read and not used)
    if (Rb) {
#pragma unroll
      for (int i = 0; i < 4; i++) rr[i] = RX::load(Rb + (int64_t)max(pr[i], 0) * F + col);
    }
    V outr[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      outr[i] = V::zero();
      const int r = r0 + i;
      if (r < r1) {
        const int pb = r ? pend[r - 1] : 0, pe = pend[r];
        for (int p = pb; p < pe; p++) outr[i].add(V::load(tile + (int)pvs[p] * TW + lcol));
        if (a.degV && pe > pb) outr[i].mul(dv_regs ? dv[i] : sdeg[r]);
        if (pr[i] < 0) outr[i].store(a.partial + (int64_t)(pr[i] & 0x7fffffff) * F + col);  // summed and scaled by the fixup pass
      }
    }
    if (Rb || a.epi.ca != 1.f) {  // t' = ca * t + cb * R[v], the fp32 epilogue's operations in its order
      const float cb = a.epi.cb_dev ? *a.epi.cb_dev : a.epi.cb;
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (r0 + i < r1) {
          outr[i].mul(a.epi.ca);
          if (Rb) {
            rr[i].mul(cb);
            outr[i].add(rr[i]);
          }
        }
    }
    uint2 tb[4];  // the ONE rounding: these bits are T_out's and the operand's
#pragma unroll
    for (int i = 0; i < 4; i++) tb[i] = round_bf16x4(outr[i].v);
    if (Tb) {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (r0 + i < r1 && pr[i] >= 0) *reinterpret_cast<uint2 *>(Tb + (int64_t)pr[i] * TW + lcol) = tb[i];
    }
    __syncthreads();  // every slot row has been read: the tile becomes the operand plane
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (r0 + i < r1) *reinterpret_cast<uint2 *>(reinterpret_cast<char *>(tile) + split_off(r0 + i, lcol)) = tb[i];
    __syncthreads();
    if (a.F_out > 64) panel_times_wt_b16<2>(tile, nrows, a.F_out, wb, prow, static_cast<T *>(a.Y), tid, bq, a.epi.relu, a.y_nt);
    else panel_times_wt_b16<1>(tile, nrows, a.F_out, wb, prow, static_cast<T *>(a.Y), tid, bq, a.epi.relu, a.y_nt);
    return;
  } else if constexpr (LIN) {  // ---- hop 2 into registers, then rows * Wlin^T on the matrix cores
    // the B fragments of this wave's first column tile are issued after hop 2 and fly across the two barriers that
    // follow (issued before hop 2 they would hold K/4 more registers through it: 78 instead of 64 VGPRs)
    [[maybe_unused]] float bv[BPre<TW / 4>::N];
    [[maybe_unused]] SplitB bsp[kSplitDepth];
    const LinSplit sp = lin_split(tid >> 6, a.F_out >> 4);
    if constexpr (SPLIT) {  // the first steps' B fragments (three bf16 planes each): in flight during hop 2
      if (sp.active) {
#pragma unroll
        for (int t = 0; t < kSplitDepth; t++)
          bsp[t] = load_bsplit_step(static_cast<const uint4 *>(a.epi.wsplit), sp, a.F_out >> 4, a.F_out > 64 ? 2 : 1, t, tid & 63);
      }
    }
    const int rpg = (nrows + NG - 1) / NG;  // <= 4 (launcher)
    const int r0 = min(g * rpg, nrows), r1 = min(r0 + rpg, nrows);
    // A layer's residual rows (t = ca Aggr(X) + cb R): the lane group's four rows of R in flight together, unconditionally (a row
    // past the group's range reads the panel's last row and is not used), and BEFORE hop 2, which they overlap.  Under
    // `if (r0 + i < r1)` after hop 2 each load was followed by s_waitcnt vmcnt(0) -- four dependent trips to HBM per panel in every
    // UniGCNII / UniGIN layer.
    V rr[4];
    if (a.epi.R) {
#pragma unroll
      for (int i = 0; i < 4; i++) rr[i] = V::load(a.epi.R + (int64_t)prow[min(r0 + i, nrows - 1)] * F + col);
    }
    V outr[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      outr[i] = V::zero();
      const int r = r0 + i;
      if (r < r1) {
        const int pb = r ? pend[r - 1] : 0, pe = pend[r];
        for (int p = pb; p < pe; p++) outr[i].add(V::load(tile + (int)pvs[p] * TW + lcol));
        if (a.degV && pe > pb) outr[i].mul(dv_regs ? dv[i] : sdeg[r]);
      }
    }
    if (a.epi.R || a.epi.ca != 1.f) {  // t' = ca * t + cb * R[v]  (workgroup-uniform)
      const float cb = a.epi.cb_dev ? *a.epi.cb_dev : a.epi.cb;
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (r0 + i < r1) {
          outr[i].mul(a.epi.ca);
          if (a.epi.R) {
            rr[i].mul(cb);
            outr[i].add(rr[i]);
          }
        }
    }
    if constexpr (SPLIT) {
      const int pstride = split_plane_bytes(a.rows_cap);
      if (a.epi.T_out) {  // the combined rows themselves, for the backward pass: straight from the registers
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (r0 + i < r1) outr[i].store(a.epi.T_out + (int64_t)prow[r0 + i] * TW + lcol);
      }
      __syncthreads();  // every slot row has been read: the tile becomes the operand's three bf16 planes
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (r0 + i < r1) split_store_row(reinterpret_cast<char *>(tile), pstride, r0 + i, lcol, outr[i].v);
      __syncthreads();
      if (a.F_out > 64) panel_times_wt_split<2>(tile, pstride, nrows, a.F_out, static_cast<const uint4 *>(a.epi.wsplit), prow, static_cast<float *>(a.Y), tid, bsp, a.epi.relu);
      else panel_times_wt_split<1>(tile, pstride, nrows, a.F_out, static_cast<const uint4 *>(a.epi.wsplit), prow, static_cast<float *>(a.Y), tid, bsp, a.epi.relu);
      return;
    }
    if (sp.active) load_bfrag_pre<TW / 4>(a.Wlin, sp.nt_first, tid & 63, bv);
    __syncthreads();  // every slot row has been read: the tile becomes the [rows][TW + 4] operand
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (r0 + i < r1) outr[i].store(tile + (r0 + i) * (TW + 4) + lcol);
    __syncthreads();
    if (a.epi.T_out) {  // the combined rows themselves, for the backward pass (dWlin needs them)
      constexpr int q = TW >> 2;
      for (int i = tid; i < nrows * q; i += 256) {
        const int r = i / q, c = (i - r * q) * 4;
        *reinterpret_cast<float4 *>(a.epi.T_out + (int64_t)prow[r] * TW + c) =
            *reinterpret_cast<const float4 *>(tile + r * (TW + 4) + c);
      }
    }
    panel_times_wt<TW / 4, LINW>(tile, nrows, a.F_out, a.Wlin, prow, 0, static_cast<float *>(a.Y), tid, bv, a.epi.relu);
    return;
  } else {  // ---- hop 2
    const int rpg = (nrows + NG - 1) / NG;
    const int r0 = min(g * rpg, nrows), r1 = min(r0 + rpg, nrows);
    auto row = [&](const int r, const float dscale) {  // dscale: the row's degV where it came in a register, else read from LDS
      V acc = V::zero();
      const int pb = r ? pend[r - 1] : 0, pe = pend[r];
      for (int p = pb; p < pe; p++) acc.add(V::load(tile + (int)pvs[p] * TW + lcol));
      if (a.degV && pe > pb) acc.mul(dv_regs ? dscale : sdeg[r]);
      if (col_ok) {
        const int pr = prow[r];  // vertex id, or bit 31 | partial row (a piece of a split vertex)
        if constexpr (YF32) {
          float *dst = (pr < 0 ? a.partial + (int64_t)(pr & 0x7fffffff) * F : static_cast<float *>(a.Y) + (int64_t)pr * F) + col;
          if (a.y_nt && pr >= 0) acc.store_n_nt(dst, a.F - col);  // partial rows are read back by the fixup pass: plain
          else acc.store_n(dst, a.F - col);
        } else {  // partial rows stay fp32
          if (pr < 0) {
            acc.store_n(a.partial + (int64_t)(pr & 0x7fffffff) * F + col, a.F - col);
          } else {
            T *y = static_cast<T *>(a.Y) + (int64_t)pr * F + col;
            if (a.y_nt) RX::store_n_nt(acc, y, a.F - col);
            else RX::store_n(acc, y, a.F - col);
          }
        }
      }
    };
    if (SCALED && dv_regs) {  // at most four rows, their factors in dv[0..3] (static indices)
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (r0 + i < r1) row(r0 + i, dv[i]);
    } else {
      for (int r = r0; r < r1; r++) row(r, 1.f);
    }
  }
}


// The hub pass (HubPass, hg_internal.h).  One persistent 1024-thread workgroup per CU: lane group g
// keeps the running sums of its R virtual hub rows in registers for the whole launch and walks the
// workgroup's rounds; per round the hyperedge sums are computed ONCE into the LDS tile (hop 1 as in
// fused_packed_kernel: same entry words, same unpredicated buffer loads) and every lane group adds
// the tile rows its hubs belong to (16-bit lists, cumulative ends per virtual row).  A vertex in
// 10^6 hyperedges costs one LDS row read per incidence instead of one 4F-byte row of a 1 GB table
// from HBM, and the table never exists.  Each workgroup writes one partial row per virtual row;
// fixup_rows_kernel adds them in slot order.
//  * The next round's record travels through registers during hop 1 (two dwordx4 per thread), so
//    its round trip hides behind the row gathers.
//  * HEAVY: the (at most six) heaviest hubs have no virtual rows.  Bits 24..29 of the last entry of a
//    slot name the heavy hubs among the hyperedge's members, and the lane group that finishes the sum
//    adds it to registers of its own: no tile read, no list entry, every lane group equally loaded.
//    The lane groups' registers are added up once, at the end (through the tile, in group order).
//  * Hop 2 is latency-bound (index read -> tile row read -> add, ~2 LDS latencies per pair on one
//    dependent chain): the lane group's R ends are fetched at once, and the rows are walked four
//    registers at a time, all four pairs of a step in flight; a step past a row's end reads the
//    all-zero row `cap` instead of branching.  Registers are ordered by weight (the plan deals the
//    heaviest rows first), so the four rows of a chunk have similar lengths.
// T: element type of the rows of X (Rows); the partial rows it writes are fp32.
template <int LPR, int VEC, int U, bool MAT, bool SCALED, bool HEAVY, typename T = float>
__global__ __launch_bounds__(1024) void hub_pass_kernel(const HubArgs a) {
  constexpr int BS = 1024, NG = BS / LPR, TW = LPR * VEC, R = kHubRows, NH = HEAVY ? kHubHeavy : 1;
  using V = Vec<VEC>;
  using RX = Rows<T, VEC>;
  extern __shared__ int32_t smem[];
  const int tid = threadIdx.x;
  const int gl = tid & (LPR - 1);
  const int lcol = gl * VEC;
  const int col = blockIdx.y * TW + lcol;
  const bool col_ok = col < a.F;
  const int64_t F = a.F;
  const int w = blockIdx.x;
  const int g = tid / LPR;
  float *tile = reinterpret_cast<float *>(smem);                          // [(cap + 1) * TW], row `cap` = zeros
  int32_t *recbuf = smem + (a.cap + 1) * TW;                              // 2 x [max_rec_words]: this round's record, the next one's
  float *sA = reinterpret_cast<float *>(recbuf + 2 * a.max_rec_words);    // [cap]
  float *sB = sA + a.cap;                                                 // [cap]

  V acc[R];
#pragma unroll
  for (int i = 0; i < R; i++) acc[i] = V::zero();
  [[maybe_unused]] V hacc[NH];
#pragma unroll
  for (int h = 0; h < NH; h++) hacc[h] = V::zero();
  if (tid < LPR) V::zero().store(tile + a.cap * TW + lcol);
  const unsigned row_bytes = (unsigned)a.F * 4u;
  const unsigned col_off = col_ok ? (unsigned)col * 4u : 0x80000000u;
  [[maybe_unused]] const unsigned xrow_bytes = (unsigned)a.F * (unsigned)sizeof(T);  // rows of X at their element size
  [[maybe_unused]] const unsigned xcol_off = col_ok ? (unsigned)col * (unsigned)sizeof(T) : 0x80000000u;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.X), 0, a.x_bytes, 0x00020000);
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<void *>(a.Xe_mat ? static_cast<const void *>(a.Xe_mat) : a.X), 0, a.Xe_mat ? a.mat_bytes : 0, 0x00020000);
  const int rd0 = a.wg_first[w], rd1 = a.wg_first[w + 1];
  // A record is at most NPRE * 16 KB: each thread carries NPRE dwordx4 of the NEXT round's record
  // through hop 1, so the copy's round trip hides behind the row gathers.
  constexpr int NPRE = 2;
  hg_i4 pre[NPRE];
  auto fetch = [&](int rd) {
    const HubRec rt = a.rec_tab[rd];
    const hg_i4 *src = reinterpret_cast<const hg_i4 *>(a.rec + rt.off);
#pragma unroll
    for (int k = 0; k < NPRE; k++) {
      const int i = tid + k * BS;
      if (i < (rt.len >> 2)) pre[k] = src[i];
    }
    return rt.len >> 2;
  };
  auto stash = [&](int32_t *dst, int n4) {
#pragma unroll
    for (int k = 0; k < NPRE; k++) {
      const int i = tid + k * BS;
      if (i < n4) reinterpret_cast<hg_i4 *>(dst)[i] = pre[k];
    }
  };
  int cur = 0;
  if (rd0 < rd1) stash(recbuf, fetch(rd0));
  __syncthreads();
  for (int rd = rd0; rd < rd1; rd++) {
    const int32_t *rec = recbuf + cur * a.max_rec_words;
    int n4_next = 0;
    if (rd + 1 < rd1) n4_next = fetch(rd + 1);  // in flight across hop 1
    if constexpr (SCALED) {
      const int nslots = rec[1];
      const int32_t *eid = rec + rec[10];
      for (int i = tid; i < nslots; i += BS) {
        const int e = eid[i];  // -1: materialised row, already scaled
        sA[i] = (a.degE && e >= 0) ? a.degE[e] : 1.f;
        sB[i] = (a.W && e >= 0) ? a.W[e] : 1.f;
      }
      __syncthreads();
    }
    const int steps = rec[0];
    const int32_t *gbase = rec + rec[4];
    const int32_t *stream = rec + rec[5];
    const uint16_t *pend = reinterpret_cast<const uint16_t *>(rec + rec[6]);
    const uint16_t *pvs = reinterpret_cast<const uint16_t *>(rec + rec[9]);
    {  // ---- hop 1: this round's hyperedge sums -> tile (and heavy hubs' registers)
      [[maybe_unused]] int slot = gbase[g];
      float *tp = tile + gbase[g] * TW + lcol;
      V sum = V::zero();
      // two phases, as in fused_packed_kernel: rows of X, then rows of the materialised table
      auto block = [&](const int s0, const int send, auto full, auto matph) {
        constexpr bool FULL = decltype(full)::value;
        constexpr bool MATPH = decltype(matph)::value;
        const int idle = MATPH ? a.nrows_mat : a.nrows_x;
        int ent[U];
#pragma unroll
        for (int j = 0; j < U; j++) ent[j] = (FULL || s0 + j < send) ? stream[(s0 + j) * NG + g] : idle;
        V v[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
          if (!FULL && s0 + j >= send) {
            v[j] = V::zero();
            continue;
          }
          if constexpr (!MATPH && !std::is_same_v<T, float>) {
            v[j] = RX::load_buf(rx, __umul24((unsigned)ent[j], xrow_bytes) + xcol_off);
          } else {
            const unsigned off = __umul24((unsigned)ent[j], row_bytes) + col_off;  // flags sit above bit 23
            v[j] = V::load_buf(MATPH ? rm : rx, off);
          }
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
          sum.add(v[j]);
          if (ent[j] < 0) {  // bit 31: last member of this slot
            if constexpr (SCALED) {
              if (a.degE) sum.mul(sA[slot]);
              if (a.W) sum.mul(sB[slot]);
              slot++;
            }
            sum.store(tp);
            tp += TW;
            if constexpr (HEAVY) {
              const int hm = (ent[j] >> 24) & ((1 << NH) - 1);
              if (hm) {
#pragma unroll
                for (int h = 0; h < NH; h++)
                  if (hm & (1 << h)) hacc[h].add(sum);
              }
            }
            sum = V::zero();
          }
        }
      };
      const int steps_x = MAT ? rec[8] : steps;
      int s0 = 0;
      for (; s0 + U <= steps_x; s0 += U) block(s0, steps_x, std::true_type{}, std::false_type{});
      if (s0 < steps_x) block(s0, steps_x, std::false_type{}, std::false_type{});
      if constexpr (MAT) {
        for (s0 = steps_x; s0 + U <= steps; s0 += U) block(s0, steps, std::true_type{}, std::true_type{});
        if (s0 < steps) block(s0, steps, std::false_type{}, std::true_type{});
      }
    }
    stash(recbuf + (cur ^ 1) * a.max_rec_words, n4_next);  // nobody reads that buffer during this round
    __syncthreads();
    {  // ---- hop 2: every virtual row adds the tile rows of the hyperedges it belongs to
      // the lane group's R cumulative ends: eight aligned dwords of 16-bit pairs (g * R is a multiple of 16)
      const uint32_t *pw = reinterpret_cast<const uint32_t *>(pend) + g * (R / 2);
      uint32_t ew[R / 2];
#pragma unroll
      for (int i = 0; i < R / 2; i++) ew[i] = pw[i];
      const int first = g ? (int)(pw[-1] >> 16) : 0;
      auto end_of = [&](int i) { return (int)((ew[i >> 1] >> ((i & 1) * 16)) & 0xffffu); };  // i static
      constexpr int C = kHubChunk;  // rows walked together: four (index, tile row) pairs in flight per lane group
#pragma unroll
      for (int c = 0; c < R; c += C) {
        int b_[C], n_[C], len = 0;
#pragma unroll
        for (int i = 0; i < C; i++) {
          b_[i] = c + i ? end_of(c + i - 1) : first;
          n_[i] = end_of(c + i) - b_[i];
          len = max(len, n_[i]);
        }
        for (int k = 0; __builtin_amdgcn_ballot_w64(k < len) != 0; k++) {  // wave-uniform trip count
          int sidx[C];
#pragma unroll
          for (int i = 0; i < C; i++) sidx[i] = k < n_[i] ? (int)pvs[b_[i] + k] : a.cap;
          V t[C];
#pragma unroll
          for (int i = 0; i < C; i++) t[i] = V::load(tile + sidx[i] * TW + lcol);
#pragma unroll
          for (int i = 0; i < C; i++) acc[c + i].add(t[i]);
        }
      }
    }
    __syncthreads();  // the tile is rewritten by the next round, this record by the one after
    cur ^= 1;
  }
  int vs0[R];  // the lane group's R partial slots: requested together (read one by one next to their stores they were R dependent
               // round trips at the end of every workgroup)
#pragma unroll
  for (int i = 0; i < R; i++) vs0[i] = a.vslot0[g * R + i];
#pragma unroll
  for (int i = 0; i < R; i++)
    if (vs0[i] >= 0 && col_ok) acc[i].store(a.partial + (int64_t)(vs0[i] + w) * F + col);
  if constexpr (HEAVY) {  // the lane groups' shares of each heavy hub, added in group order
    for (int h = 0; h < a.n_heavy; h++) {
      V mine = V::zero();
#pragma unroll
      for (int q = 0; q < NH; q++)
        if (q == h) mine = hacc[q];
      mine.store(tile + g * TW + lcol);
      __syncthreads();
      if (g == 0) {
        V tot = V::zero();
#pragma unroll 8  // left alone the compiler unrolls all NG (128 at F = 32) tile reads at once: 44-84 bytes of scratch per lane
        for (int q = 0; q < NG; q++) tot.add(V::load(tile + q * TW + lcol));
        if (col_ok) tot.store(a.partial + (int64_t)(a.hslot0[h] + w) * F + col);
      }
      __syncthreads();
    }
  }
}

// Streaming row gather (RowStream, hg_internal.h): dst[r] = scaleB * (scaleA * sum of the src rows of CSR
// row r), scheduled like a panel's hop 1 -- the workgroup's rows spread over the lane groups longest first,
// eight unpredicated buffer loads in flight per lane -- and finished in registers: the lane group that
// reaches a row's last entry scales the sum and stores the row (or a chunk's partial row).  No tile, no
// second hop, one barrier.  The materialisation pre-pass of the fused variant runs on it.
// TS / TD: element types of src / dst rows (Rows); partial rows are fp32.
template <int LPR, int VEC, int U, typename TS = float, typename TD = float>
__global__ __launch_bounds__(256) void stream_rows_kernel(const StreamArgs a) {
  constexpr int BS = 256, NG = BS / LPR, TW = LPR * VEC;
  using V = Vec<VEC>;
  using RS = Rows<TS, VEC>;
  using RD = Rows<TD, VEC>;
  extern __shared__ int32_t smem[];
  const int tid = threadIdx.x;
  const int gl = tid & (LPR - 1);
  const int col = blockIdx.y * TW + gl * VEC;
  const bool col_ok = col < a.F;
  const int64_t F = a.F;
  int b = blockIdx.x;
  if (a.xcd_remap) {
    const int x = b & 7, i = b >> 3;
    const int cpx = a.nrec >> 3, rem = a.nrec & 7;
    b = x * cpx + (x < rem ? x : rem) + i;
  }
  const SRec rt = a.rec_tab[b];
  const int32_t *grec = a.rec + rt.off;
  int32_t *rec = smem;                                           // [max_rec_words]
  float *sA = reinterpret_cast<float *>(rec + a.max_rec_words);  // [cap]
  float *sB = sA + a.cap;                                        // [cap]
  // A scaled call stages the record, then per slot an id and the factors it names: written as loops one after the other that was
  // four dependent round trips (record, id, scaleA, scaleB) before the barrier.  A thread's piece of the record and its slot's id
  // are requested together (clamped indices, no lane-dependent branch around a load), then both factors together.
  const int nrec4 = rt.len >> 2;
  const bool scaled = (a.scaleA || a.scaleB) && rt.nslots > 0;  // workgroup-uniform
  if (scaled) {
    const hg_i4 rv = reinterpret_cast<const hg_i4 *>(grec)[min(tid, nrec4 - 1)];
    const int si = grec[rt.off_sidx + min(tid, rt.nslots - 1)];  // -1: a chunk (scaled by its fixup) or an empty row (stays exactly 0)
    const int sc = max(si, 0);
    float fa = 1.f, fb = 1.f;
    if (a.scaleA) fa = a.scaleA[sc];
    if (a.scaleB) fb = a.scaleB[sc];
    if (tid < nrec4) reinterpret_cast<hg_i4 *>(rec)[tid] = rv;
    if (tid < rt.nslots) {
      sA[tid] = si >= 0 ? fa : 1.f;
      sB[tid] = si >= 0 ? fb : 1.f;
    }
  }
  for (int i = scaled ? tid + BS : tid; i < nrec4; i += BS)
    reinterpret_cast<hg_i4 *>(rec)[i] = reinterpret_cast<const hg_i4 *>(grec)[i];
  if (a.scaleA || a.scaleB)
    for (int i = tid + BS; i < rt.nslots; i += BS) {
      const int si = grec[rt.off_sidx + i];
      sA[i] = (a.scaleA && si >= 0) ? a.scaleA[si] : 1.f;
      sB[i] = (a.scaleB && si >= 0) ? a.scaleB[si] : 1.f;
    }
  __syncthreads();
  const int steps = rec[0];
  const int32_t *stream = rec + rec[5];
  const int32_t *dstl = rec + rec[6];
  const int g = tid / LPR;
  int slot = rec[rec[4] + g];
  const unsigned row_bytes = (unsigned)a.F * (unsigned)sizeof(TS);
  const unsigned col_off = col_ok ? (unsigned)col * (unsigned)sizeof(TS) : 0x80000000u;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.src), 0, a.src_bytes, 0x00020000);
  TD *dst = static_cast<TD *>(a.dst);
  const int idle = a.nrows_src;
  V acc = V::zero();
  auto block = [&](const int s0, auto full) {
    constexpr bool FULL = decltype(full)::value;
    int ent[U];
#pragma unroll
    for (int j = 0; j < U; j++) ent[j] = (FULL || s0 + j < steps) ? stream[(s0 + j) * NG + g] : idle;
    V v[U];
#pragma unroll
    for (int j = 0; j < U; j++) {
      if (!FULL && s0 + j >= steps) {
        v[j] = V::zero();
        continue;
      }
      v[j] = RS::load_buf(rx, __umul24((unsigned)ent[j], row_bytes) + col_off);  // flags sit above bit 23
    }
#pragma unroll
    for (int j = 0; j < U; j++) {
      acc.add(v[j]);
      if (ent[j] < 0) {  // bit 31: last entry of this row (or chunk)
        if (a.scaleA) acc.mul(sA[slot]);
        if (a.scaleB) acc.mul(sB[slot]);
        const int d = dstl[slot];
        slot++;
        if (col_ok) {
          if constexpr (std::is_same_v<TD, float>) {
            if (a.nt_dst && d >= 0) acc.store_n_nt(dst + (int64_t)d * F + col, a.F - col);
            else acc.store_n((d < 0 ? a.partial + (int64_t)(d & 0x7fffffff) * F : dst + (int64_t)d * F) + col, a.F - col);
          } else if (d < 0) {  // partial rows stay fp32
            acc.store_n(a.partial + (int64_t)(d & 0x7fffffff) * F + col, a.F - col);
          } else if (a.nt_dst) {
            RD::store_n_nt(acc, dst + (int64_t)d * F + col, a.F - col);
          } else {
            RD::store_n(acc, dst + (int64_t)d * F + col, a.F - col);
          }
        }
        acc = V::zero();
      }
    }
  };
  int s0 = 0;
  for (; s0 + U <= steps; s0 += U) block(s0, std::true_type{});
  if (s0 < steps) block(s0, std::false_type{});
}

// Push form (the scheme the reference's group_* tensors describe, HyperGsys/balancer.py:15-33): a task sums the
// member rows of one partition of a hyperedge and adds the scaled sum into the rows of Y that another partition
// names, with memory-side fp32 atomics.  Lane layout: one feature column per lane, LPR = next_pow2(F) lanes per
// task (64 / LPR tasks per wave) -- the shape the atomic units want: an atomic wave-instruction then covers whole
// contiguous row segments (two 128-byte rows at F = 32), which is what runs at the chip's full atomic rate
// (MI355X_MICROARCH.md, global float atomics); 16-byte lanes gather faster but scatter every fourth float per
// instruction and lost 1.3-2x on the dataset shapes (profiles/r03_experiments.md).  The source rows go eight at a
// time into flight.  Kept as the drop-in for callers that bring the reference's schedule (any ngs, the w^2 task
// grid included) and as the CLI's comparator; AUTO never picks it -- atomics run at about 1.3 TB/s of added bytes.
template <int LPR>
__global__ __launch_bounds__(256) void push_tasks_kernel(const PushArgs a) {
  constexpr int TPB = 256 / LPR, U = 8;
  const int64_t task = (int64_t)blockIdx.x * TPB + threadIdx.x / LPR;
  const int col = blockIdx.y * LPR + (threadIdx.x & (LPR - 1));
  if (task >= a.n_group || col >= a.F) return;
  const int64_t F = a.F;
  // source partition, destination partition and hyperedge of this task: from the caller's schedule, or one task
  // per hyperedge covering all its members
  int e, src_lo, src_hi, dst_lo, dst_hi;
  if (a.group_key) {
    e = a.group_row[task];
    const int ps = a.group_st[task], pd = a.group_ed[task];
    src_lo = a.group_key[ps];
    src_hi = a.group_key[ps + 1];
    dst_lo = a.group_key[pd];
    dst_hi = a.group_key[pd + 1];
  } else {
    e = (int)task;
    src_lo = dst_lo = a.csrptr_t[e];
    src_hi = dst_hi = a.csrptr_t[e + 1];
  }
  const float *xcol = a.X + col;
  float sum = 0.f;
  for (int p = src_lo; p < src_hi; p += U) {  // members in order: the sum is the reference kernel's, bit for bit
    float v[U];
#pragma unroll
    for (int j = 0; j < U; j++) v[j] = xcol[(int64_t)a.colind_t[min(p + j, src_hi - 1)] * F];
#pragma unroll
    for (int j = 0; j < U; j++)
      if (p + j < src_hi) sum += v[j];
  }
  float es = a.degE ? a.degE[e] : 1.f;  // degE * W first, then the sum times that product (hgnnaggr_cuda.cu:38)
  es *= a.W ? a.W[e] : 1.f;
  sum *= es;
  float *ycol = a.Y + col;
  for (int p = dst_lo; p < dst_hi; p++) {
    const int64_t v = a.colind_t[p];
    atomicAdd(ycol + v * F, a.degV ? sum * a.degV[v] : sum);
  }
}

static inline int next_pow2(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

// The lane rule: a row of F floats lies on a power of two of lanes, 64 at the most (wider rows take more column tiles), of
// four floats each (vec4: 16-byte lanes) or one.  lanes_per_row is for rows of whole lanes (vec4: F % 4 == 0);
// lanes_per_row_up covers rows of any width with 16-byte lanes (loadu / store_n) and so counts the last, partial lane.
static inline int lanes_pow2(int lanes) { return std::min(64, next_pow2(std::max(lanes, 1))); }
static inline int lanes_per_row(int F, bool vec4) { return lanes_pow2(vec4 ? F / 4 : F); }
static inline int lanes_per_row_up(int F, bool vec4) { return lanes_pow2(vec4 ? (F + 3) / 4 : F); }

// Runtime launch arguments to template arguments.  dispatch_lpr calls fn with the lanes per row (a power of two from MIN to
// 64; anything else is an invalid value) as a std::integral_constant, dispatch_vec with the floats per lane, and both
// return what fn returns.  The constants convert to int where fn names a kernel: fn<L, V>.
template <int N> using Int = std::integral_constant<int, N>;
template <int L, int MIN, typename Fn> static hipError_t call_lpr(Fn &fn) {
  if constexpr (L >= MIN) return fn(Int<L>{});
  else return hipErrorInvalidValue;
}
template <int MIN = 1, typename Fn> static hipError_t dispatch_lpr(int lpr, Fn fn) {
  switch (lpr) {
    case 1: return call_lpr<1, MIN>(fn);
    case 2: return call_lpr<2, MIN>(fn);
    case 4: return call_lpr<4, MIN>(fn);
    case 8: return call_lpr<8, MIN>(fn);
    case 16: return call_lpr<16, MIN>(fn);
    case 32: return call_lpr<32, MIN>(fn);
    case 64: return call_lpr<64, MIN>(fn);
  }
  return hipErrorInvalidValue;
}
template <typename Fn> static hipError_t dispatch_vec(bool vec4, Fn fn) { return vec4 ? fn(Int<4>{}) : fn(Int<1>{}); }
template <typename Fn> static hipError_t dispatch_flag(bool flag, Fn fn) { return flag ? fn(std::true_type{}) : fn(std::false_type{}); }
// the MAT and SCALED of the fused panels and the hub pass: a materialised table is read; hyperedge scales (degE, W) are applied
template <typename Args, typename Fn> static hipError_t dispatch_mat_scaled(const Args &a, Fn fn) {
  return dispatch_flag(a.Xe_mat != nullptr, [&](auto M) { return dispatch_flag(a.degE || a.W, [&](auto S) { return fn(M, S); }); });
}

// The element types of two row tables, fn(TA{}, TB{}) with each of float and bf16.  bf16 rows exist on 16-byte lanes only:
// at VEC = 1 no bf16 pair is formed (so no such kernel is instantiated) and a bf16 flag is an invalid value.
template <int VEC, typename Fn> static hipError_t dispatch_rows(bool a_bf16, bool b_bf16, Fn fn) {
  if constexpr (VEC == 4) {
    if (a_bf16 && b_bf16) return fn(bf16{}, bf16{});
    if (a_bf16) return fn(bf16{}, float{});
    if (b_bf16) return fn(float{}, bf16{});
  } else if (a_bf16 || b_bf16) {
    return hipErrorInvalidValue;
  }
  return fn(float{}, float{});
}

// Dynamic LDS above the 64 KiB default is an opt-in per kernel; gfx950 has 160 KiB per CU.
constexpr size_t kLdsMax = 160 * 1024;
template <auto Kern, int BLOCK = 256, typename Args>
static hipError_t launch_lds(dim3 grid, size_t lds, hipStream_t stream, const Args &a) {
  static std::atomic<size_t> granted{64 * 1024};
  if (lds > kLdsMax) return hipErrorInvalidValue;
  if (lds > granted.load(std::memory_order_relaxed)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
    if (e != hipSuccess) return e;
    granted.store(kLdsMax, std::memory_order_relaxed);
  }
  hipLaunchKernelGGL(Kern, grid, dim3(BLOCK), lds, stream, a);
  return hipGetLastError();
}

// The dynamic LDS of a panel gather, the carve-up of gather_rows_kernel and gather_rows_reduce_kernel: sptr
// [panel_rows + 1], three more words per row, then entry_words per index entry -- 1: sind alone; 2: a float (a position)
// beside it, the weighted (reduce) instances -- and last the attention instances' row_extras scalars per row.
static size_t panel_lds_bytes(int32_t panel_rows, int32_t panel_nnz, int entry_words, size_t row_extras = 0) {
  return ((size_t)4 * panel_rows + 1 + (size_t)entry_words * panel_nnz + row_extras * panel_rows) * sizeof(int32_t);
}

// The two-level fixup sums, lane groups of LPR lanes: the first level's fixups [0, nfix_l1) (rows cut into very many
// tasks), then the rest in a launch of their own.  Kern: fixup_rows_kernel or fixup_rows_reduce_kernel.
template <auto Kern, int LPR, typename Args>
static hipError_t launch_fixup_levels(const Args &a, int col_tiles, int nfix, int nfix_l1, const Fixup *fixups, hipStream_t stream) {
  const int per_block = 256 / LPR;
  if (nfix_l1 > 0)
    hipLaunchKernelGGL(Kern, dim3((nfix_l1 + per_block - 1) / per_block, col_tiles), dim3(256), 0, stream, a, fixups, nfix_l1);
  if (nfix > nfix_l1)
    hipLaunchKernelGGL(Kern, dim3((nfix - nfix_l1 + per_block - 1) / per_block, col_tiles), dim3(256), 0, stream, a,
                       fixups + nfix_l1, nfix - nfix_l1);
  return hipGetLastError();
}

template <int LPR, int VEC, typename TD = float>
static hipError_t launch_fixups_t(const GatherArgs &a, int nfix, int nfix_l1, const Fixup *fixups, hipStream_t stream) {
  const int col_tiles = (a.F + LPR * VEC - 1) / (LPR * VEC);
  return launch_fixup_levels<fixup_rows_kernel<LPR, VEC, TD>, LPR>(a, col_tiles, nfix, nfix_l1, fixups, stream);
}

// WM: 0 no weights, 1 a weight per entry (the WT instances), 2 a weight per entry and head (the WH instances), 3 the
// attention coefficient formed in the lane (the WA instances)
template <int LPR, int VEC, typename TS = float, typename TD = float, int WM = 0>
static hipError_t launch_gather_t(const GatherArgsOf<WM == 1, WM == 2, WM == 3> &a, int nfix, int nfix_l1, const Fixup *fixups,
                                  hipStream_t stream) {
  const int col_tiles = (a.F + LPR * VEC - 1) / (LPR * VEC);
  const int nblocks = a.n_task_blocks + a.npanels;
  if (nblocks > 0) {
    // the weighted instances stage one float (heads: one position) per index entry beside sind; the attention instances
    // stage nothing per entry: the unweighted layout, then the rows' scalars
    size_t lds = panel_lds_bytes(a.panel_rows, a.panel_nnz, WM == 1 || WM == 2 ? 2 : 1);
    if constexpr (WM == 3) lds = attn_gather_lds_bytes(a.panel_rows, a.panel_nnz, a.heads, a.stat_row != 0);
    const dim3 grid(nblocks, col_tiles);
    const hipError_t e = launch_lds<gather_rows_kernel<LPR, VEC, TS, TD, WM == 1, WM == 2, WM == 3>>(grid, lds, stream, a);
    if (e != hipSuccess) return e;
  }
  return launch_fixups_t<LPR, VEC, TD>(a, nfix, nfix_l1, fixups, stream);
}

// gather_rows_kernel's WM = 0 .. 2 instances on lpr lanes of VEC = (lane4 ? 4 : 1) floats and, on 16-byte lanes, every form
// of (src_bf16, dst_bf16); a bf16 form on 4-byte lanes is an invalid value
template <int WM>
static hipError_t launch_gather_rows(const GatherArgsOf<WM == 1, WM == 2, false> &a, int nfix, int nfix_l1, const Fixup *fixups,
                                     int lpr, bool lane4, hipStream_t stream, bool src_bf16, bool dst_bf16) {
  return dispatch_lpr(lpr, [&](auto L) {
    return dispatch_vec(lane4, [&](auto V) {
      return dispatch_rows<V>(src_bf16, dst_bf16, [&](auto ts, auto td) {
        return launch_gather_t<L, V, decltype(ts), decltype(td), WM>(a, nfix, nfix_l1, fixups, stream);
      });
    });
  });
}

hipError_t launch_gather(const GatherArgs &a, int nfix, int nfix_l1, const Fixup *fixups, bool vec4,
                         hipStream_t stream, bool src_bf16, bool dst_bf16) {
  if ((src_bf16 || dst_bf16) && !vec4) return hipErrorInvalidValue;
  return launch_gather_rows<0>(a, nfix, nfix_l1, fixups, lanes_per_row(a.F, vec4), vec4, stream, src_bf16, dst_bf16);
}

hipError_t launch_gather_weighted(const WeightedGatherArgs &a, int nfix, int nfix_l1, const Fixup *fixups, bool vec4,
                                  hipStream_t stream, bool src_bf16, bool dst_bf16) {
  if (!a.w || ((src_bf16 || dst_bf16) && !vec4)) return hipErrorInvalidValue;
  return launch_gather_rows<1>(a, nfix, nfix_l1, fixups, lanes_per_row(a.F, vec4), vec4, stream, src_bf16, dst_bf16);
}

// lane4: 16-byte lanes are legal (C % 4 == 0, rows and partial rows 16-byte aligned).  lpr: the lanes per row of the
// single-head call of the same F -- the heads instances keep it on 4-byte lanes too and run more column tiles instead, so
// that a wave task's entries are dealt to the same 64 / lpr row groups and every column is summed in the single-head order.
hipError_t launch_gather_heads(const HeadsGatherArgs &a, int nfix, int nfix_l1, const Fixup *fixups, bool vec4, bool lane4,
                               hipStream_t stream, bool src_bf16, bool dst_bf16) {
  if (!a.w || a.heads < 1 || a.C < 1 || (int64_t)a.heads * a.C != a.F || (lane4 && (!vec4 || a.C % 4))) return hipErrorInvalidValue;
  if ((src_bf16 || dst_bf16) && !lane4) return hipErrorInvalidValue;
  return launch_gather_rows<2>(a, nfix, nfix_l1, fixups, lanes_per_row(a.F, vec4), lane4, stream, src_bf16, dst_bf16);
}

size_t attn_gather_lds_bytes(int32_t panel_rows, int32_t panel_nnz, int32_t heads, bool stat_row) {
  return panel_lds_bytes(panel_rows, panel_nnz, 1, (size_t)(stat_row ? 3 : 1) * heads);
}

// launch_gather_heads' lane rule (lane4, lpr), so that every column is summed in the order of the WH instance on alpha
hipError_t launch_gather_attention(const AttnGatherArgs &a, int nfix, int nfix_l1, const Fixup *fixups, bool vec4, bool lane4,
                                   hipStream_t stream) {
  if (!a.seg_max || !a.seg_inv || a.heads < 1 || a.C < 1 || (int64_t)a.heads * a.C != a.F || (lane4 && (!vec4 || a.C % 4)))
    return hipErrorInvalidValue;
  return dispatch_lpr(lanes_per_row(a.F, vec4), [&](auto L) {
    return dispatch_vec(lane4, [&](auto V) { return launch_gather_t<L, V, float, float, 3>(a, nfix, nfix_l1, fixups, stream); });
  });
}

template <int LPR, int VEC, int RMODE>
static hipError_t launch_gather_reduce_t(const ReduceGatherArgs &a, int nfix, int nfix_l1, const Fixup *fixups, hipStream_t stream) {
  const int col_tiles = (a.F + LPR * VEC - 1) / (LPR * VEC);
  const int nblocks = a.n_task_blocks + a.npanels;
  if (nblocks > 0) {
    const size_t lds = panel_lds_bytes(a.panel_rows, a.panel_nnz, 2);  // a position beside every index entry
    const hipError_t e = launch_lds<gather_rows_reduce_kernel<LPR, VEC, RMODE>>(dim3(nblocks, col_tiles), lds, stream, a);
    if (e != hipSuccess) return e;
  }
  if constexpr (RMODE == 3)
    return launch_fixups_t<LPR, VEC>(a, nfix, nfix_l1, fixups, stream);  // float partial rows, summed in slot order
  else
    return launch_fixup_levels<fixup_rows_reduce_kernel<LPR, VEC, RMODE == 1>, LPR>(a, col_tiles, nfix, nfix_l1, fixups, stream);
}

hipError_t launch_gather_reduce(const ReduceGatherArgs &a, int rmode, int nfix, int nfix_l1, const Fixup *fixups, bool vec4,
                                hipStream_t stream) {
  if (rmode < 1 || rmode > 3 || (rmode == 3 ? !a.arg_in : (!a.arg_out || (nfix > 0 && !a.ipartial)))) return hipErrorInvalidValue;
  return dispatch_lpr(lanes_per_row(a.F, vec4), [&](auto L) {
    return dispatch_vec(vec4, [&](auto V) {
      return rmode == 1   ? launch_gather_reduce_t<L, V, 1>(a, nfix, nfix_l1, fixups, stream)
             : rmode == 2 ? launch_gather_reduce_t<L, V, 2>(a, nfix, nfix_l1, fixups, stream)
                          : launch_gather_reduce_t<L, V, 3>(a, nfix, nfix_l1, fixups, stream);
    });
  });
}

// a_bf16 / b_bf16: rows of A / B are bf16 (16-byte lanes only: the caller has checked widths and alignment)
hipError_t launch_incidence_dot_heads(int32_t M, int64_t nnz, int32_t H, int32_t C, const int32_t *ptr, const int32_t *ind,
                                      const void *A, const void *B, float *out, bool lane4, hipStream_t stream, bool a_bf16,
                                      bool b_bf16) {
  if (nnz == 0) return hipSuccess;
  if (M <= 0 || H <= 0 || C <= 0 || (lane4 && C % 4) || ((a_bf16 || b_bf16) && !lane4)) return hipErrorInvalidValue;
  const int lph = lanes_per_row(C, lane4);
  const int64_t items = (nnz + kDotRun - 1) / kDotRun * H;
  const int64_t per_block = 256 / lph;
  const int64_t nblocks = (items + per_block - 1) / per_block;
  if (nblocks > 0x7fffffff) return hipErrorInvalidValue;
  return dispatch_lpr(lph, [&](auto L) {
    return dispatch_vec(lane4, [&](auto V) {
      return dispatch_rows<V>(a_bf16, b_bf16, [&](auto ta, auto tb) {
        hipLaunchKernelGGL((incidence_dot_heads_kernel<L, V, decltype(ta), decltype(tb)>), dim3((unsigned)nblocks), dim3(256), 0,
                           stream, ptr, ind, M, nnz, H, C, static_cast<const decltype(ta) *>(A),
                           static_cast<const decltype(tb) *>(B), out);
        return hipGetLastError();
      });
    });
  });
}

hipError_t launch_incidence_dot(int32_t M, int64_t nnz, int32_t F, const int32_t *ptr, const int32_t *ind, const void *A,
                                const void *B, float *out, bool vec4, hipStream_t stream, bool a_bf16, bool b_bf16) {
  if (nnz == 0) return hipSuccess;
  if (M <= 0 || F <= 0 || (vec4 && F % 4) || ((a_bf16 || b_bf16) && !vec4)) return hipErrorInvalidValue;
  const int lpr = lanes_per_row(F, vec4);
  const int64_t per_block = (int64_t)(256 / lpr) * kDotRun;
  const int64_t nblocks = (nnz + per_block - 1) / per_block;
  if (nblocks > 0x7fffffff) return hipErrorInvalidValue;
  return dispatch_lpr(lpr, [&](auto L) {
    return dispatch_vec(vec4, [&](auto V) {
      return dispatch_rows<V>(a_bf16, b_bf16, [&](auto ta, auto tb) {
        hipLaunchKernelGGL((incidence_dot_kernel<L, V, decltype(ta), decltype(tb)>), dim3((unsigned)nblocks), dim3(256), 0, stream,
                           ptr, ind, M, nnz, F, static_cast<const decltype(ta) *>(A), static_cast<const decltype(tb) *>(B), out);
        return hipGetLastError();
      });
    });
  });
}

// ---- the product of two hyperedge sums (hg_hyperedge_dot_heads_f32): the gradient of a per-hyperedge scale ---------------
// out[e] = sum_c SA[e, c] * SB[e, c] with SA[e, :] = sum_{p=(e,u)} wa[p, c / C] * A[u, :] and SB likewise from (B, wb).
// Both sums run over the same H_T row, so a lane group gathers the two member rows of an entry together and keeps both
// sums in registers: neither [M, F] table exists in memory, one float per hyperedge leaves.
//
// Work split.  A row of F floats lies on LPR lanes of VEC floats, as in gather_rows_kernel (launch_gather's rule), and a
// lane group owns one hyperedge, 256 / LPR hyperedges per workgroup, U = 4 member-row pairs in flight.  Rows wider than
// the group's tile (LPR * VEC columns: more than 256 at 16-byte lanes) are walked once per column chunk; a lane adds the
// chunk's products to its partial dot before the next chunk.  The lanes' partial dots meet in incidence_dot_kernel's
// butterfly.  Hyperedges of more than kSegLong members are skipped here and taken by hyperedge_dot_long_kernel, one
// workgroup each from the plan's side-0 long-row list: group g takes members g, g + NG, ...; the groups' sums of both
// tables are added through LDS in group order 0 .. NG - 1 by group 0, which then forms the chunk's products.
// No atomics; a lane adds its members in ascending order: the order depends on the row's length, F and heads only.
// A unit weight is the factor 1.0f of the same fma (fma(x, 1, s) = s + x exactly): one instance for all four forms.
template <int VEC>
__device__ __forceinline__ void edge_dot_walk(const EdgeDotArgs &a, int64_t beg, int64_t end, int step, int col, bool col_ok,
                                              int hd, Vec<VEC> &sa, Vec<VEC> &sb) {
  constexpr int U = 4;  // member-row pairs in flight per lane
  using V = Vec<VEC>;
  const int64_t F = a.F;
  for (int64_t p = beg; p < end; p += (int64_t)step * U) {
    V va[U], vb[U];
    float fa[U], fb[U];
#pragma unroll
    for (int k = 0; k < U; k++) {
      const int64_t q = p + (int64_t)k * step;
      const bool ok = col_ok && q < end;
      const int64_t row = ok ? (int64_t)a.ind[q] * F + col : 0;
      fa[k] = (ok && a.wa) ? a.wa[q * a.heads + hd] : 1.f;
      fb[k] = (ok && a.wb) ? a.wb[q * a.heads + hd] : 1.f;
      va[k] = ok ? V::load(a.A + row) : V::zero();
      vb[k] = ok ? V::load(a.B + row) : V::zero();
    }
#pragma unroll
    for (int k = 0; k < U; k++) {
      if (p + (int64_t)k * step < end) {
        sa.fma(va[k], fa[k]);
        sb.fma(vb[k], fb[k]);
      }
    }
  }
}

template <int VEC>
__device__ __forceinline__ float edge_dot_add(const Vec<VEC> &x, const Vec<VEC> &y, float dot) {
  if constexpr (VEC == 4) {
    dot = __builtin_fmaf(x.v.x, y.v.x, dot);
    dot = __builtin_fmaf(x.v.y, y.v.y, dot);
    dot = __builtin_fmaf(x.v.z, y.v.z, dot);
    return __builtin_fmaf(x.v.w, y.v.w, dot);
  } else {
    return __builtin_fmaf(x.x, y.x, dot);
  }
}

template <int LPR, int VEC>
__global__ __launch_bounds__(256) void hyperedge_dot_kernel(const EdgeDotArgs a) {
  using V = Vec<VEC>;
  constexpr int NG = 256 / LPR;
  const int tid = threadIdx.x, gl = tid & (LPR - 1);
  const int64_t e = (int64_t)blockIdx.x * NG + tid / LPR;
  bool valid = e < a.M;
  int32_t beg = 0, end = 0;
  if (valid) {
    beg = a.ptr[e];
    end = a.ptr[e + 1];
    if (end - beg > kSegLong) {  // a workgroup of its own has it
      beg = end = 0;
      valid = false;
    }
  }
  float dot = 0.f;
  for (int c0 = 0; c0 < a.F; c0 += LPR * VEC) {
    const int col = c0 + gl * VEC;
    const bool col_ok = col < a.F;
    V sa = V::zero(), sb = V::zero();
    edge_dot_walk<VEC>(a, beg, end, 1, col, col_ok, col_ok ? col / a.C : 0, sa, sb);
    dot = edge_dot_add<VEC>(sa, sb, dot);
  }
#pragma unroll
  for (int off = 1; off < LPR; off <<= 1) dot += __shfl_xor(dot, off, 64);
  if (gl == 0 && valid) a.out[e] = dot;  // an empty hyperedge: no member, no product: +0.0f
}

template <int LPR, int VEC>
__global__ __launch_bounds__(256) void hyperedge_dot_long_kernel(const EdgeDotArgs a) {
  using V = Vec<VEC>;
  constexpr int NG = 256 / LPR;
  __shared__ __attribute__((aligned(16))) float lds[2 * 256 * VEC];  // [table][group][lane][VEC]
  const int tid = threadIdx.x, gl = tid & (LPR - 1), g = tid / LPR;
  const int32_t e = a.long_seg[blockIdx.x];
  const int32_t beg = a.ptr[e], end = a.ptr[e + 1];
  float dot = 0.f;
  for (int c0 = 0; c0 < a.F; c0 += LPR * VEC) {
    const int col = c0 + gl * VEC;
    const bool col_ok = col < a.F;
    V sa = V::zero(), sb = V::zero();
    edge_dot_walk<VEC>(a, (int64_t)beg + g, end, NG, col, col_ok, col_ok ? col / a.C : 0, sa, sb);
    sa.store(lds + tid * VEC);
    sb.store(lds + (256 + tid) * VEC);
    __syncthreads();
    if (g == 0) {
      V ta = V::zero(), tb = V::zero();
      for (int k = 0; k < NG; k++) {
        ta.add(V::load(lds + (k * LPR + gl) * VEC));
        tb.add(V::load(lds + (256 + k * LPR + gl) * VEC));
      }
      dot = edge_dot_add<VEC>(ta, tb, dot);
    }
    __syncthreads();  // the sums have been read before the next chunk's are written
  }
#pragma unroll
  for (int off = 1; off < LPR; off <<= 1) dot += __shfl_xor(dot, off, 64);
  if (tid == 0) a.out[e] = dot;
}

hipError_t launch_hyperedge_dot(const EdgeDotArgs &a, bool lane4, hipStream_t stream) {
  if (a.M <= 0) return hipSuccess;
  if (a.F <= 0 || a.heads < 1 || a.C < 1 || (int64_t)a.heads * a.C != a.F || (lane4 && (a.F % 4 || a.C % 4)) || !a.ptr ||
      !a.A || !a.B || !a.out || a.nlong < 0 || (a.nlong > 0 && !a.long_seg))
    return hipErrorInvalidValue;
  const int lpr = lanes_per_row(a.F, lane4);
  const unsigned nblocks = (unsigned)(((int64_t)a.M + 256 / lpr - 1) / (256 / lpr));
  return dispatch_lpr(lpr, [&](auto L) {
    return dispatch_vec(lane4, [&](auto V) {
      hipLaunchKernelGGL((hyperedge_dot_kernel<L, V>), dim3(nblocks), dim3(256), 0, stream, a);
      if (a.nlong > 0) hipLaunchKernelGGL((hyperedge_dot_long_kernel<L, V>), dim3(a.nlong), dim3(256), 0, stream, a);
      return hipGetLastError();
    });
  });
}

// out[r] = <A[r, :], B[r, :]>: one lane group per row, a lane's fma chain over its columns (ascending), then the same
// butterfly.  The last step of the degV gradient, <dY[v], Z[v]>.
template <int LPR, int VEC>
__global__ __launch_bounds__(256) void rows_dot_kernel(int64_t nrows, int32_t F, const float *A, const float *B, float *out) {
  using V = Vec<VEC>;
  constexpr int NG = 256 / LPR;
  const int tid = threadIdx.x, gl = tid & (LPR - 1);
  const int64_t r = (int64_t)blockIdx.x * NG + tid / LPR;
  const bool valid = r < nrows;
  float dot = 0.f;
  if (valid) {
    const float *pa = A + r * F, *pb = B + r * F;
    for (int c = gl * VEC; c < F; c += LPR * VEC) dot = edge_dot_add<VEC>(V::load(pa + c), V::load(pb + c), dot);
  }
#pragma unroll
  for (int off = 1; off < LPR; off <<= 1) dot += __shfl_xor(dot, off, 64);
  if (gl == 0 && valid) out[r] = dot;
}

hipError_t launch_rows_dot(int64_t nrows, int32_t F, const float *A, const float *B, float *out, bool vec4,
                           hipStream_t stream) {
  if (nrows <= 0) return hipSuccess;
  if (F <= 0 || (vec4 && F % 4) || !A || !B || !out) return hipErrorInvalidValue;
  const int lpr = lanes_per_row(F, vec4);
  const int64_t nblocks = (nrows + 256 / lpr - 1) / (256 / lpr);
  if (nblocks > 0x7fffffff) return hipErrorInvalidValue;
  return dispatch_lpr(lpr, [&](auto L) {
    return dispatch_vec(vec4, [&](auto V) {
      hipLaunchKernelGGL((rows_dot_kernel<L, V>), dim3((unsigned)nblocks), dim3(256), 0, stream, nrows, F, A, B, out);
      return hipGetLastError();
    });
  });
}

hipError_t launch_fixups(const Fixup *fixups, int nfix, int nfix_l1, int32_t F, float *partial, void *Y,
                         const float *scaleA, const float *scaleB, const int32_t *scale_map, bool vec4,
                         hipStream_t stream, bool nt_dst, bool Y_bf16) {
  if (nfix == 0) return hipSuccess;
  if (Y_bf16 && (!vec4 || (F & 3))) return hipErrorInvalidValue;
  GatherArgs a{};
  a.nt_dst = nt_dst ? 1 : 0;
  a.F = F;
  a.partial = partial;
  a.dst = Y;
  a.scaleA = scaleA;
  a.scaleB = scaleB;
  a.scale_map = scale_map;
  // vec4 here: 16-byte lanes over rows of any width (loadu / store_n)
  return dispatch_lpr(lanes_per_row_up(F, vec4), [&](auto L) {
    if (Y_bf16) return launch_fixups_t<L, 4, bf16>(a, nfix, nfix_l1, fixups, stream);
    return dispatch_vec(vec4, [&](auto V) { return launch_fixups_t<L, V>(a, nfix, nfix_l1, fixups, stream); });
  });
}

bool stream_rows_ok(const StreamArgs &a, bool vec4) {
  return vec4 && a.nrec > 0 && a.src_bytes > 0 && a.nrows_src < (1 << 24) && a.F < (1 << 22) &&
         a.ng == 256 / lanes_per_row_up(a.F, true) && (size_t)a.max_rec_words * 4 + (size_t)2 * a.cap * 4 <= kLdsMax;
}

template <int LPR>
static hipError_t launch_stream_t(const StreamArgs &a, hipStream_t stream, bool src_bf16, bool dst_bf16) {
  constexpr int TW = LPR * 4;
  const dim3 grid(a.nrec, (a.F + TW - 1) / TW);
  const size_t lds = (size_t)a.max_rec_words * 4 + (size_t)2 * a.cap * 4;
  return dispatch_rows<4>(src_bf16, dst_bf16, [&](auto ts, auto td) {
    using TS = decltype(ts);
    using TD = decltype(td);
    if constexpr (std::is_same_v<TS, bf16> && std::is_same_v<TD, bf16>) return hipErrorInvalidValue;  // no such instance
    else return launch_lds<stream_rows_kernel<LPR, 4, 8, TS, TD>>(grid, lds, stream, a);
  });
}

hipError_t launch_stream_rows(const StreamArgs &a, hipStream_t stream, bool src_bf16, bool dst_bf16) {
  if (a.nrec == 0) return hipSuccess;
  if ((src_bf16 && dst_bf16) || ((src_bf16 || dst_bf16) && (a.F & 3))) return hipErrorInvalidValue;
  return dispatch_lpr(lanes_per_row_up(a.F, true), [&](auto L) { return launch_stream_t<L>(a, stream, src_bf16, dst_bf16); });
}

size_t hub_pass_lds_bytes(int32_t cap, int32_t row_floats, int32_t max_rec_words) {
  return (size_t)(cap + 1) * row_floats * 4 + (size_t)2 * max_rec_words * 4 + (size_t)2 * cap * 4 + 16;
}

template <int LPR, typename T>
static hipError_t launch_hub_t(const HubArgs &a, hipStream_t stream) {
  constexpr int TW = LPR * 4;
  if (a.ng != 1024 / LPR) return hipErrorInvalidValue;  // records were packed for another lane layout
  const bool fast = a.x_bytes > 0 && a.nrows_x < (1 << 24) && a.F < (1 << 22) &&
                    (!a.Xe_mat || (a.mat_bytes > 0 && a.nrows_mat < (1 << 24)));
  if (!fast) return hipErrorInvalidValue;  // the plan builds a hub pass only for buffer-addressable tables
  const dim3 grid(a.nwg, (a.F + TW - 1) / TW);
  const size_t lds = hub_pass_lds_bytes(a.cap, TW, a.max_rec_words);
  if (a.cap < 1024 / LPR) return hipErrorInvalidValue;  // the end-of-launch reduction parks one row per lane group in the tile
  return dispatch_mat_scaled(a, [&](auto M, auto S) {
    return dispatch_flag(a.n_heavy > 0, [&](auto H) {  // HEAVY: hubs fed by stream flags
      return launch_lds<hub_pass_kernel<LPR, 4, 4, M, S, H, T>, 1024>(grid, lds, stream, a);
    });
  });
}

hipError_t launch_hub_pass(const HubArgs &a, bool vec4, hipStream_t stream, bool x_bf16) {
  if (a.nwg == 0) return hipSuccess;
  if (!vec4) return hipErrorInvalidValue;
  if (x_bf16 && (a.F & 3)) return hipErrorInvalidValue;
  return dispatch_lpr<4>(lanes_per_row_up(a.F, true), [&](auto L) {  // no instances of 1 and 2 lanes
    return x_bf16 ? launch_hub_t<L, bf16>(a, stream) : launch_hub_t<L, float>(a, stream);
  });
}

// floats of LDS the panel kernel stages scales in (its sA / sB / sdeg carve-up): degE and W per slot where present, degV per
// row unless it travels in registers (a.dv_regs)
static size_t fused_scale_floats(const FusedArgs &a) {
  return (size_t)(a.degE ? a.cap : 0) + (size_t)(a.W ? a.cap : 0) + (size_t)((a.degV && !a.dv_regs) ? a.rows_cap : 0);
}
// Bound degV in registers (fused_packed_kernel) where it can be (SCALED instance, at most four rows per lane group) AND its
// LDS would cost a resident workgroup: measured on one box, weighted batches at F = 32: cora x1024 0.597-0.600 -> 0.611-0.614
// of the roofline, citeseer 0.680 -> 0.690, pubmed x256 0.459 -> 0.497 (seven -> eight workgroups per CU); at F = 128, where
// eight fit either way, the register form costs 4.5 % (cora x256 0.589 -> 0.562) and is not used.
static int fused_dv_regs(const FusedArgs &a, int ng, size_t lds_without_scales, int max_wgs) {
  if (!((a.degE || a.W) && a.degV && a.bsD && a.rows_cap <= 4 * ng)) return 0;
  const size_t common = lds_without_scales + ((size_t)(a.degE ? a.cap : 0) + (size_t)(a.W ? a.cap : 0)) * 4;
  const size_t with = common + (size_t)a.rows_cap * 4;
  const int fit_with = (int)std::min<size_t>((size_t)max_wgs, kLdsMax / with);
  const int fit_without = (int)std::min<size_t>((size_t)max_wgs, kLdsMax / common);
  return fit_without > fit_with ? 1 : 0;
}

// T: element type of the rows of X and Y.  bf16 (VEC = 4 only) takes the fp32 instances' decisions.  TY: rows of Y where they
// are not T's (bf16 X, fp32 Y; no epilogue).
template <int LPR, int VEC, typename T = float, typename TY = T>
static hipError_t launch_fused_t(const FusedArgs &a, hipStream_t stream) {
  if (a.npanels == 0) return hipSuccess;
  constexpr int TW = LPR * VEC;
  constexpr bool XF32 = std::is_same_v<T, float>;
  if constexpr (VEC == 4 && (LPR == 8 || LPR == 16)) {
    // a tiny dense hypergraph as one or a few 1024-thread panels (hg_api.hip, get_fused): nothing materialised there
    if (a.ng == 1024 / LPR) {
      const bool fast = a.x_bytes > 0 && a.nrows_x < (1 << 24) && a.F < (1 << 22) && (a.F & 3) == 0;
      if (!fast || a.Wlin || a.Xe_mat) return hipErrorInvalidValue;
      const dim3 grid(a.npanels, (a.F + TW - 1) / TW);
      const size_t lds = (size_t)a.cap * TW * 4 + (size_t)a.max_rec_words * 4 + fused_scale_floats(a) * 4 + 16;  // dv_regs = 0
      if (a.degE || a.W) return launch_lds<fused_packed_kernel<LPR, VEC, 8, true, false, true, false, 1024, true, false, T, false, TY>, 1024>(grid, lds, stream, a);
      return launch_lds<fused_packed_kernel<LPR, VEC, 8, true, false, false, false, 1024, true, false, T, false, TY>, 1024>(grid, lds, stream, a);
    }
  }
  if (a.ng != 256 / LPR) return hipErrorInvalidValue;  // records were packed for another lane layout
  const int col_tiles = (a.F + TW - 1) / TW;
  FusedArgs ad = a;
  const dim3 grid(a.npanels, col_tiles);
  // tile | record | scale staging (only what this call's scales need: without them the F = 32
  // bench shape fits 8 workgroups per CU instead of 7)
  // (the linear epilogue's instances stage degV in LDS: their tile already decides the residency)
  ad.dv_regs = a.Wlin ? 0 : fused_dv_regs(a, 256 / LPR, (size_t)a.cap * TW * 4 + (size_t)a.max_rec_words * 4 + 16, 8);
  const size_t lds_p = (size_t)a.cap * TW * 4 + (size_t)a.max_rec_words * 4 + fused_scale_floats(ad) * 4 + 16;
  if constexpr (VEC == 4) {
    const bool fast = a.x_bytes > 0 && a.nrows_x < (1 << 24) && a.F < (1 << 22) &&
                      (!a.Xe_mat || (a.mat_bytes > 0 && a.nrows_mat < (1 << 24)));
    if (a.Wlin) {  // linear epilogue: eligibility was checked by fused_linear_ok
      if constexpr (XF32 && (TW == 32 || TW == 64 || TW == 128)) {
        if (!fast || a.F != TW || a.rows_cap > 4 * (256 / LPR) || (a.F_out & 15)) return hipErrorInvalidValue;
        const size_t lds_l = lds_p - (size_t)a.cap * TW * 4 + (size_t)lin_tile_floats(a.cap, a.rows_cap, TW) * 4;  // slot tile / padded operand rows
        // the staged matrix phase alone serves this call (as panel_times_wt decides per panel, for the fullest panel)
        const int nt_all = a.F_out >> 4, nwr = nt_all >= 3 ? 1 : 4 / nt_all;
        const bool staged = a.F_out <= TW && (((a.rows_cap + 15) >> 4) + nwr - 1) / nwr <= (a.F_out > 64 ? 2 : 4);
        // K = 128, staged: the LDS tile already holds occupancy to five workgroups per CU, so the registers for twelve row
        // gathers in flight per lane cost nothing there (a panel's hop 1 is then two dependent batches instead of three)
        constexpr int UL = LPR >= 32 ? kLinU32 : 8;
        // bf16x6 matrix phase (a.epi.wsplit): K = 128, staged, at most 32 rows, and the three operand planes fit the tile region
        bool split = false;
        if constexpr (TW == 128) {
          const int ps = split_plane_bytes(a.rows_cap), tile_b = lin_tile_floats(a.cap, a.rows_cap, TW) * 4;
          split = a.epi.wsplit && staged && a.rows_cap > 0 && a.rows_cap <= 32 && 3 * ps <= tile_b && 2 * ps + 32 * 256 <= (int)lds_l;
        }
        if (!split) ad.epi.wsplit = nullptr;
        return dispatch_mat_scaled(a, [&](auto M, auto S) {
          if constexpr (TW == 128)
            if (split) return launch_lds<fused_packed_kernel<LPR, VEC, UL, true, M, S, true, 256, false, true>>(grid, lds_l, stream, ad);
          return staged ? launch_lds<fused_packed_kernel<LPR, VEC, UL, true, M, S, true, 256, false>>(grid, lds_l, stream, ad)
                        : launch_lds<fused_packed_kernel<LPR, VEC, 8, true, M, S, true, 256, true>>(grid, lds_l, stream, ad);
        });
      } else if constexpr (!XF32 && std::is_same_v<TY, T> && TW == 128) {
        // the native bf16 epilogue (fused_linear_b16_ok): K = 128 staged, at most 32 rows -- the one operand plane (32 rows of
        // 256 bytes, read whole) and the [rows][132] fp32 results both fit the tile region, which holds at least 16 x 132 floats
        if (!fast || !fused_linear_b16_ok(a)) return hipErrorInvalidValue;
        const size_t lds_l = lds_p - (size_t)a.cap * TW * 4 + (size_t)lin_tile_floats(a.cap, a.rows_cap, TW) * 4;
        if ((size_t)lin_tile_floats(a.cap, a.rows_cap, TW) * 4 < 32 * 256) return hipErrorInvalidValue;
        return dispatch_mat_scaled(a, [&](auto M, auto S) {
          return launch_lds<fused_packed_kernel<LPR, VEC, kB16U, true, M, S, true, 256, false, false, T, true>>(grid, lds_l, stream, ad);
        });
      } else {
        return hipErrorInvalidValue;
      }
    }
    if (fast) {
      // A grid that does not even fill the chip once is latency-bound, not occupancy-bound:
      // put every row gather of a group in flight at once (U = 16) instead of two batches.
      const bool u16 = a.npanels <= 512;
      return dispatch_mat_scaled(a, [&](auto M, auto S) {
        return u16 ? launch_lds<fused_packed_kernel<LPR, VEC, 16, true, M, S, false, 256, true, false, T, false, TY>>(grid, lds_p, stream, ad)
                   : launch_lds<fused_packed_kernel<LPR, VEC, 8, true, M, S, false, 256, true, false, T, false, TY>>(grid, lds_p, stream, ad);
      });
    }
    if (a.F & 3) return hipErrorInvalidValue;  // other widths ride on the range-checked buffer loads only (hg_api: wide_rows_ok)
  }
  if (a.Wlin) return hipErrorInvalidValue;
  if constexpr (XF32 && VEC == 1 && LPR >= 8) {  // F >= 5, not a multiple of 4 (class-count widths): the same buffer-load
                                          // loop, one dword per lane (+7-20 % at F = 7, 33; narrower rows: no gain)
    const bool fast = a.x_bytes > 0 && a.nrows_x < (1 << 24) && a.F < (1 << 22) &&
                      (!a.Xe_mat || (a.mat_bytes > 0 && a.nrows_mat < (1 << 24)));
    if (fast) {
      if (!a.Xe_mat && !a.degE && !a.W)
        return launch_lds<fused_packed_kernel<LPR, VEC, 8, true, false, false>>(grid, lds_p, stream, ad);
      return launch_lds<fused_packed_kernel<LPR, VEC, 8, true, true, true>>(grid, lds_p, stream, ad);
    }
  }
  return launch_lds<fused_packed_kernel<LPR, VEC, 8, false, true, true, false, 256, true, false, T, false, TY>>(grid, lds_p, stream, ad);
}

bool fused_linear_b16_ok(const FusedArgs &a) {
  return fused_linear_ok(a) && a.F == 128 && a.F_out <= 128 && a.rows_cap > 0 && a.rows_cap <= 32;
}

hipError_t launch_linear_pack_bf16(int32_t F_out, int32_t F_in, const uint16_t *Wlin, void *wfrag, hipStream_t stream) {
  if (F_out <= 0 || (F_out & 15) || (F_in != 32 && F_in != 64 && F_in != 128)) return hipErrorInvalidValue;
  const int64_t n = (int64_t)(F_out >> 4) * (F_in >> 5) * 64;
  hipLaunchKernelGGL(linear_pack_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, F_out, F_in, Wlin,
                     static_cast<uint4 *>(wfrag));
  return hipGetLastError();
}

hipError_t launch_linear_bf16(const LinearB16Args &a, bool t_f32, hipStream_t stream) {
  if (a.nrows == 0) return hipSuccess;
  if ((a.F_out & 15) || a.F_out <= 0) return hipErrorInvalidValue;
  const int64_t nb = (a.nrows + 63) / 64;  // four waves of 16 rows
  if (nb > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)nb), block(256);
#define HG_LRB(KS_)                                                                                   \
  if (t_f32) hipLaunchKernelGGL((linear_rows_bf16_kernel<KS_, true>), grid, block, 0, stream, a);     \
  else hipLaunchKernelGGL((linear_rows_bf16_kernel<KS_, false>), grid, block, 0, stream, a);          \
  break
  switch (a.F_in) {
    case 32: HG_LRB(1);
    case 64: HG_LRB(2);
    case 128: HG_LRB(4);
    default: return hipErrorInvalidValue;
  }
#undef HG_LRB
  return hipGetLastError();
}

hipError_t launch_linear_pack_split(int32_t F_out, int32_t F_in, const float *Wlin, void *wsplit, hipStream_t stream) {
  if (F_out <= 0 || F_in != 128 || (F_out & 15)) return hipErrorInvalidValue;
  const int64_t n = (int64_t)(F_out >> 4) * (F_in >> 5) * 64;
  hipLaunchKernelGGL(linear_pack_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, F_out, F_in, Wlin,
                     static_cast<uint4 *>(wsplit));
  return hipGetLastError();
}

hipError_t launch_linear_pack(int32_t F_out, int32_t F_in, const float *Wlin, float *wfrag, hipStream_t stream) {
  if (F_out <= 0 || F_in <= 0 || (F_out & 15) || (F_in & 15)) return hipErrorInvalidValue;
  const int64_t n = (int64_t)F_out * F_in;
  hipLaunchKernelGGL(linear_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, F_out, F_in,
                     Wlin, wfrag);
  return hipGetLastError();
}

// One resident round of workgroups: the accumulators (4 registers per output tile) decide how
// many fit a CU -- 64 x 64: three, 32 x 32: eight.
// Products beyond sixteen 16 x 16 tiles (the accumulators of one wave) run as independent 64 x 64 blocks of the output over the
// same rows (blockIdx.y; both widths multiples of 64): 128 x 128 = four blocks, every operand row read twice.  rocBLAS takes
// 1.11 ms for [128 x 693 k] . [693 k x 128] (35.8 % of a 4-layer nhid = 128 HGNN epoch under rocprofv3).
bool wgrad_blocked(int32_t Fa, int32_t Fb) { return (Fa / 16) * (Fb / 16) > 16; }
bool wgrad_shape_ok(int32_t Fa, int32_t Fb) {
  if (Fa <= 0 || Fb <= 0 || (Fa & 15) || (Fb & 15)) return false;
  if (!wgrad_blocked(Fa, Fb)) return true;
  return (Fa % 64) == 0 && (Fb % 64) == 0 && Fa <= 512 && Fb <= 512;
}
int wgrad_parts(int64_t nrows, int32_t Fa, int32_t Fb) {
  const bool blocked = wgrad_blocked(Fa, Fb);
  if (blocked) Fa = Fb = 64;
  const int tiles = (Fa / 16) * (Fb / 16);
  const int64_t cap = tiles <= 4 ? 2048 : (tiles <= 8 ? 1024 : 768);
  const int n = (int)std::max<int64_t>(1, std::min<int64_t>(cap, (nrows + 63) / 64));
  return blocked ? (n + 7) / 8 * 8 : n;  // blocked: whole groups of eight parts (one per XCD; a part past the rows adds zeros)
}

hipError_t launch_wgrad(int64_t nrows, int32_t Fa, int32_t Fb, const float *A, const float *B, float *C,
                        float *partial, hipStream_t stream) {
  if (!wgrad_shape_ok(Fa, Fb)) return hipErrorInvalidValue;
  const bool blocked = wgrad_blocked(Fa, Fb);
  const int32_t Ba = blocked ? 64 : Fa, Bb = blocked ? 64 : Fb;  // block of the output one workgroup's accumulators hold
  const int nba = Fa / Ba, nbb = Fb / Bb, nblocks = nba * nbb;
  const int nparts = wgrad_parts(nrows, Fa, Fb);  // blocked: a multiple of 8
  int64_t rows_per_wg = (nrows + nparts - 1) / nparts;
  rows_per_wg = (rows_per_wg + 15) & ~(int64_t)15;
#define HG_WG(TA_, TB_)                                                                                          \
  if (Ba == 16 * TA_ && Bb == 16 * TB_) {                                                                        \
    hipLaunchKernelGGL((wgrad_kernel<TA_, TB_>), dim3(nparts * nblocks), dim3(256), 0, stream, A, B, partial, nrows, rows_per_wg, Fa, Fb, nbb, nblocks, nparts); \
  } else
  HG_WG(1, 1) HG_WG(1, 2) HG_WG(2, 1) HG_WG(2, 2) HG_WG(1, 4) HG_WG(4, 1) HG_WG(2, 4) HG_WG(4, 2) HG_WG(4, 4)
  HG_WG(1, 8) HG_WG(8, 1) HG_WG(2, 8) HG_WG(8, 2) HG_WG(1, 3) HG_WG(3, 1) HG_WG(3, 3) HG_WG(3, 4) HG_WG(4, 3)
  HG_WG(2, 3) HG_WG(3, 2) { return hipErrorInvalidValue; }
#undef HG_WG
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int n = Ba * Bb;
  const int mid = nparts > 64 ? 32 : 1;  // second-level partials live behind the first-level ones
  float *p2 = partial + (int64_t)nblocks * nparts * n;
  // every block in the same two launches (blockIdx.z); per element the additions keep their fixed order: deterministic
  if (mid > 1) {
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((n + 255) / 256, mid, nblocks), dim3(256), 0, stream, partial, nparts, n, p2, 0, 0, 0, nbb);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((n + 255) / 256, 1, nblocks), dim3(256), 0, stream, p2, mid, n, C, Ba, Bb, Fb, nbb);
  } else {
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((n + 255) / 256, 1, nblocks), dim3(256), 0, stream, partial, nparts, n, C, Ba, Bb, Fb, nbb);
  }
  return hipGetLastError();
}

bool fused_linear_ok(const FusedArgs &a) {
  const int lpr = a.F / 4;
  return (a.F == 32 || a.F == 64 || a.F == 128) && a.F_out > 0 && (a.F_out & 15) == 0 && a.x_bytes > 0 && a.nrows_x < (1 << 24) &&
         (!a.Xe_mat || (a.mat_bytes > 0 && a.nrows_mat < (1 << 24))) &&
         a.ng == 256 / lpr && a.rows_cap <= 4 * (256 / lpr) && a.rows_cap <= a.cap;
}

hipError_t launch_linear(const LinearArgs &a, hipStream_t stream) {
  if (a.nrows == 0) return hipSuccess;
  if ((a.F_out & 15) || a.F_out <= 0) return hipErrorInvalidValue;
  const int R = a.F_in >= 128 ? 32 : 64;
  const int64_t nb = (a.nrows + R - 1) / R;
  if (nb > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)nb), block(256);
  switch (a.F_in) {
    case 32: hipLaunchKernelGGL((linear_rows_kernel<8>), grid, block, 0, stream, a); break;
    case 64: hipLaunchKernelGGL((linear_rows_kernel<16>), grid, block, 0, stream, a); break;
    case 128: hipLaunchKernelGGL((linear_rows_kernel<32>), grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_fused(const FusedArgs &a, bool vec4, hipStream_t stream, bool xy_bf16, bool y_f32) {
  if (xy_bf16 && (!vec4 || (a.Wlin && (y_f32 || a.F != 128)) || (a.F & 3))) return hipErrorInvalidValue;
  if (y_f32) {  // bf16 X, fp32 Y: the widths of the bf16 linear layer only
    if (!xy_bf16) return hipErrorInvalidValue;
    switch (a.F) {
      case 32: return launch_fused_t<8, 4, bf16, float>(a, stream);
      case 64: return launch_fused_t<16, 4, bf16, float>(a, stream);
      case 128: return launch_fused_t<32, 4, bf16, float>(a, stream);
      default: return hipErrorInvalidValue;
    }
  }
  return dispatch_lpr(lanes_per_row_up(a.F, vec4), [&](auto L) {
    if (xy_bf16) return launch_fused_t<L, 4, bf16>(a, stream);
    return dispatch_vec(vec4, [&](auto V) { return launch_fused_t<L, V>(a, stream); });
  });
}

// floats per LDS tile row for feature width F (what launch_fused will use): the whole row up to 64 lanes.  Cutting wide
// rows into 128-byte column tiles (the F = 32 panel shape for every width) lost 7 % at F >= 64.
int fused_tile_row_floats(int F, bool vec4) { return lanes_per_row_up(F, vec4) * (vec4 ? 4 : 1); }

hipError_t launch_push(const PushArgs &a, hipStream_t stream) {
  const int lpr = lanes_per_row(a.F, false);  // a 4-byte lane per column
  const int per_block = 256 / lpr;
  const int col_tiles = (a.F + lpr - 1) / lpr;
  const int64_t nblocks = (a.n_group + per_block - 1) / per_block;
  if (nblocks == 0) return hipSuccess;
  if (nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
  return dispatch_lpr(lpr, [&](auto L) {
    hipLaunchKernelGGL((push_tasks_kernel<L>), dim3((unsigned)nblocks, col_tiles), dim3(256), 0, stream, a);
    return hipGetLastError();
  });
}

// first_aggr = max (HGNNAggr_f1max_forward_kernel, hgnnaggr_cuda.cu:144-177): per
// hyperedge and feature column the running maximum starts at -1e5, a member
// replaces it on strict >, the winning vertex id goes to record[e, k] (0 when no
// member beats -1e5), then Xe = max * (degE * W).  One lane per (hyperedge,
// column); the second hop is the ordinary row gather over H.
__global__ __launch_bounds__(256) void gather_max_kernel(int32_t M, int32_t F, const int32_t *ptr,
                                                         const int32_t *ind, const float *X,
                                                         const float *degE, const float *W, float *Xe,
                                                         int32_t *record) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)M * F) return;
  const int32_t e = (int32_t)(t / F), k = (int32_t)(t % F);
  float best = -1e5f;
  int32_t who = 0;
  for (int32_t p = ptr[e]; p < ptr[e + 1]; p++) {
    const int32_t u = ind[p];
    const float x = X[(int64_t)u * F + k];
    if (x > best) {
      best = x;
      who = u;
    }
  }
  const float degE_val = degE ? degE[e] : 1.f, W_val = W ? W[e] : 1.f;
  best *= degE_val * W_val;
  Xe[t] = best;
  record[t] = who;
}

// Backward of first_aggr = max (HGNNAggr_f1max_backward_kernel, hgnnaggr_cuda.cu:179-208):
// Y[record[e,k], k] += T[e,k] * degV[record[e,k]], T = the scaled hyperedge sums of grad.
__global__ __launch_bounds__(256) void scatter_record_kernel(int32_t M, int32_t F, const float *T,
                                                             const int32_t *record, const float *degV,
                                                             float *Y) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)M * F) return;
  const int32_t k = (int32_t)(t % F);
  const int64_t v = record[t];
  atomicAdd(Y + v * F + k, T[t] * (degV ? degV[v] : 1.f));
}

// hg_plan_bind_scales: degE[e], W[e] per slot and degV[v] per panel row, in record order.
__global__ __launch_bounds__(256) void bind_scales_kernel(int64_t nslots, const int32_t *eid_all,
                                                          const float *degE, const float *W, float *bsA,
                                                          float *bsB, int64_t nrows, const int32_t *prow,
                                                          const float *degV, float *bsD) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < nslots) {
    const int e = eid_all[t];  // -1: materialised row, already scaled
    bsA[t] = (degE && e >= 0) ? degE[e] : 1.f;
    bsB[t] = (W && e >= 0) ? W[e] : 1.f;
  }
  if (t < nrows) bsD[t] = (degV && prow[t] >= 0) ? degV[prow[t]] : 1.f;  // pieces of split vertices: scaled by their fixup
}

hipError_t launch_bind_scales(int64_t nslots, const int32_t *eid_all, const float *degE, const float *W,
                              float *bsA, float *bsB, int64_t nrows, const int32_t *prow, const float *degV,
                              float *bsD, hipStream_t stream) {
  const int64_t n = std::max(nslots, nrows);
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(bind_scales_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, nslots,
                     eid_all, degE, W, bsA, bsB, nrows, prow, degV, bsD);
  return hipGetLastError();
}

// The reference's models pass W = ones (model/ugsys/hgnn.py:12).  Multiplying by exactly 1.0f changes no bit,
// so a bound all-ones W is dropped from the kernels' argument lists (hg_plan_bind_scales).
__global__ __launch_bounds__(256) void all_ones_kernel(int64_t n, const float *W, int32_t *flag) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool ok = true;
  for (; i < n; i += (int64_t)gridDim.x * 256) ok = ok && W[i] == 1.0f;
  if (__builtin_amdgcn_ballot_w64(!ok) != 0 && (threadIdx.x & 63) == 0) *flag = 0;
}

hipError_t launch_all_ones(int64_t n, const float *W, int32_t *flag, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<int64_t>(1024, (n + 255) / 256);
  hipLaunchKernelGGL(all_ones_kernel, dim3(blocks), dim3(256), 0, stream, n, W, flag);
  return hipGetLastError();
}

hipError_t launch_gather_max(int32_t M, int32_t F, const int32_t *ptr, const int32_t *ind, const float *X,
                             const float *degE, const float *W, float *Xe, int32_t *record,
                             hipStream_t stream) {
  const int64_t n = (int64_t)M * F;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(gather_max_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, M, F, ptr, ind,
                     X, degE, W, Xe, record);
  return hipGetLastError();
}

hipError_t launch_scatter_record(int32_t M, int32_t F, const float *T, const int32_t *record,
                                 const float *degV, float *Y, hipStream_t stream) {
  const int64_t n = (int64_t)M * F;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(scatter_record_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, M, F, T,
                     record, degV, Y);
  return hipGetLastError();
}

}  // namespace hg
