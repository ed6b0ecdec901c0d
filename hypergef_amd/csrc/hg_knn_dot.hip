// k nearest neighbours with a dot-form prefilter on the f32 MFMA and an exact rerank (include/hg_aggr.h, hg_knn_dot_f32).
// The result is hg_knn_f32's, bit for bit: the dot form |q|^2 + |x|^2 - 2 q.x only shortlists, the difference form of
// hg_knn.hip ranks the shortlist, a proven error bound certifies every row, and a row it cannot certify is searched
// exhaustively in the difference form by the same launch (DESIGN.md 3.20 has the derivation).
//
//   knn_dot_norm_kernel      n2[j] = sum_c X[j, c]^2, one fma per column in column order; one maximum per 64 rows
//   knn_dot_max_kernel       the maximum candidate norm, from the block maxima
//   knn_dot_prefilter_kernel s~ = q.x on v_mfma_f32_32x32x2_f32 (columns ascending: an fma chain, the same bits in every
//                            tiling), d~ = (n2q + n2x) - 2 s~, and per query row the kp smallest (d~, j) of its slice
//   knn_dot_rerank_kernel    one wave per query row: merges the slices' shortlists, computes the shortlist's d2 with
//                            knn_kernel's arithmetic (q - x, then one fma into one accumulator, c = 0 .. F - 1), selects
//                            the k smallest under (d2, j), certifies, and otherwise scans all n candidates
// The prefilter keeps a row's shortlist in the 32 lanes of the half wave that holds the row's accumulators (list_offer<KS,
// 32>, as knn_kernel keeps its list), the rerank its best-k list in the 64 lanes of the row's wave (list_offer<1, 64>); the
// slices' shortlists are merged by merged_rank, as knn_merge_kernel merges.  All three are hg_knn_list.h's.
// No atomics; every sum has a fixed order, so two calls give the same bits.
//
// bfloat16 rows (hg_knn_dot_bf16): the same launches with the row type R as a parameter.  The norms and the
// rerank widen every element at the load and are otherwise the kernels above; the prefilter's sums run on
// v_mfma_f32_32x32x16_bf16 (bf_tile), whose C/D layout is the f32 instruction's, so the shortlists are kept the same way
// (offer_tile, write_lists); the certificate uses the bound E1b (dot_e1b).  The float32 instances are instruction for
// instruction what they were before R existed -- which is why knn_dot_prefilter_kernel keeps its body inline: calling
// offer_tile / write_lists from it changed its register allocation.  knn_dot_estimates_bf16_kernel is the diagnostic entry's.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>

#include "hg_aggr.h"
#include "hg_internal.h"
#include "hg_knn.h"
#include "hg_knn_list.h"

namespace hg {

KnnDotLayout knn_dot_layout(int64_t nq, int64_t n, int k, int slices) {
  KnnDotLayout L;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const int64_t cap = 32 * (int64_t)knn_dot_slots(k);
  L.kp = (int)(n < cap ? n : cap);
  const size_t lists = (size_t)slices * (size_t)nq * (size_t)L.kp * 4;
  L.n2x = 0;
  L.n2q = L.n2x + up((size_t)n * 4);
  L.bmax = L.n2q + up((size_t)nq * 4);
  L.n2max = L.bmax + up((size_t)((n + kDotNormRows - 1) / kDotNormRows) * 4);
  L.idx = L.n2max + 256;
  L.est = L.idx + up(lists);
  L.mean = L.est + up(lists);
  L.total = L.mean + up((size_t)slices * (size_t)nq * 4);
  return L;
}

int knn_dot_slices(int64_t nq, int64_t n, int cand_slices) {
  const int64_t groups = (nq + kDotTQ - 1) / kDotTQ, tiles = (n + kDotTC - 1) / kDotTC;
  int64_t s = cand_slices ? cand_slices : 512 / groups;
  if (s > kKnnMaxSlices) s = kKnnMaxSlices;
  if (s > tiles) s = tiles;
  return s < 1 ? 1 : (int)s;
}

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// R: the rows' type in memory, float or uint16_t (bfloat16 bits); every kernel computes on the float32 value of an element
template <typename R>
struct DotArgsT {
  const R *Q, *X;
  int32_t nq, n, F, k, kp, slices, self_first, same;
  const float *n2q, *n2x, *n2max;
  int32_t *l_idx;  // the slices' shortlists [slices, nq, kp], each sorted under (d~, j)
  float *l_est;
  float *l_mean;  // [slices, nq] partial sums of sqrt(max(d~, 0)), or null
  int32_t *idx;
  float *dist, *mean;
  int32_t *fallback;
};
typedef DotArgsT<float> DotArgs;
typedef DotArgsT<uint16_t> DotArgsBf16;

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }  // exact

// bfloat16 rows: the two-sided bound on |d~ - D| of a row with sum = fl(n2q + n2max),
//   E1b = C_b u (n2q + n2max) + (65 G + 1) 2^-126,  G = ceil(F / 16),  C_b = (F + 34 G + 4) (1 + 1/64) rounded up
__device__ __forceinline__ float dot_e1b(int F, float sum) {
  const float u = 5.9604644775390625e-8f;  // 2^-24
  const int G = (F + 15) >> 4, c2 = F + 34 * G + 4;
  const float C = (float)(c2 + (c2 >> 6) + 1) * u;
  return C * sum + (float)(65 * G + 1) * 1.1754943508222875e-38f;  // 2^-126
}

// bfloat16 rows (R = uint16_t): where the base and the rows are 16-byte aligned a thread reads eight elements at once
template <typename R>
__global__ __launch_bounds__(256) void knn_dot_norm_kernel(const R *__restrict__ X, int n, int F, float *__restrict__ n2,
                                                           float *__restrict__ bmax) {
  __shared__ float tile[kDotNormRows][kDotNormRows + 1];
  const int t = threadIdx.x, r0 = blockIdx.x * kDotNormRows;
  float acc = 0.f;
  bool vec = false;
  if constexpr (sizeof(R) == 2) vec = ((uintptr_t)X | (uintptr_t)(2 * (size_t)F)) % 16 == 0;
  for (int f0 = 0; f0 < F; f0 += kDotNormRows) {
    __syncthreads();
    if (vec) {
      for (int e = t; e < kDotNormRows * kDotNormRows / 8; e += 256) {
        const int r = e >> 3, c = (e & 7) * 8, j = r0 + r;
        uint4 v = make_uint4(0, 0, 0, 0);  // F is a multiple of 8 here: the eight columns are inside the row or past it
        if (j < n && f0 + c < F) v = *reinterpret_cast<const uint4 *>(X + (size_t)j * F + f0 + c);
        const uint32_t p[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          tile[r][c + 2 * i] = __uint_as_float(p[i] << 16);
          tile[r][c + 2 * i + 1] = __uint_as_float(p[i] & 0xffff0000u);
        }
      }
    } else {
      for (int e = t; e < kDotNormRows * kDotNormRows; e += 256) {
        const int r = e >> 6, c = e & 63, j = r0 + r;
        tile[r][c] = (j < n && f0 + c < F) ? widen(X[(size_t)j * F + f0 + c]) : 0.f;
      }
    }
    __syncthreads();
    if (t < kDotNormRows)
#pragma unroll 8
      for (int c = 0; c < kDotNormRows; ++c) acc = fmaf(tile[t][c], tile[t][c], acc);  // a column past F adds +0
  }
  if (t < kDotNormRows) {  // wave 0
    const bool live = r0 + t < n;
    if (live) n2[r0 + t] = acc;
    float m = live ? acc : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (t == 0 && bmax) bmax[blockIdx.x] = m;
  }
}

__global__ __launch_bounds__(256) void knn_dot_max_kernel(const float *__restrict__ bmax, int nb, float *__restrict__ out) {
  __shared__ float red[4];
  const int t = threadIdx.x;
  float m = 0.f;
  for (int i = t; i < nb; i += 256) m = fmaxf(m, bmax[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((t & 63) == 0) red[t >> 6] = m;
  __syncthreads();
  if (t == 0) out[0] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// KS: shortlist slots per lane (kp <= 32 KS); MEAN: also sum sqrt(max(d~, 0)) over every candidate of the row
template <int KS, bool MEAN>
__global__ __launch_bounds__(kDotBlock) void knn_dot_prefilter_kernel(DotArgs a) {
  __shared__ float Qs[kDotTQ][kDotLd];
  __shared__ float Xs[kDotTC][kDotLd];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, tx = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * kDotTQ, slice = blockIdx.y;
  const int F = a.F, kp = a.kp, n = a.n;
  const int tiles = (n + kDotTC - 1) / kDotTC;
  const int t_begin = (int)((int64_t)tiles * slice / a.slices), t_end = (int)((int64_t)tiles * (slice + 1) / a.slices);

  // register r of an accumulator is query row (r & 3) + 8 (r >> 2) + 4 h of the wave's 32, candidate tx of the block
  const int row0 = q0 + w * 32 + 4 * h;
  float ld[16][KS];  // the sorted shortlist of row r: slot tx + 32 m
  int lj[16][KS];
  float thr[16];  // the estimate in slot kp - 1, in every lane
  float nq[16], msum[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int m = 0; m < KS; ++m) {
      ld[r][m] = INFINITY;
      lj[r][m] = INT_MAX;
    }
    thr[r] = INFINITY;
    msum[r] = 0.f;
    const int row = row0 + (r & 3) + 8 * (r >> 2);
    nq[r] = row < a.nq ? a.n2q[row] : 0.f;
  }

  // staging: a chunk is 128 query rows and 128 candidate rows of kDotFC columns.  Thirty-two lanes read one row's 128
  // bytes, so a wave's load touches two rows; thread t holds column t & 31 of rows (t >> 5) + 8 i, i < 16 of each.  Rows past
  // the end and columns past F are zeros.  The next chunk is read into registers while the MFMAs of this one run.
  float pre[32];
  const int sc = t & 31, sr = t >> 5;
  auto fetch = [&](int tile, int f0) {
    const bool col = f0 + sc < F;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int g = q0 + sr + 8 * i;
      pre[i] = (col && g < a.nq) ? a.Q[(size_t)g * F + f0 + sc] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int g = tile * kDotTC + sr + 8 * i;
      pre[16 + i] = (col && g < n) ? a.X[(size_t)g * F + f0 + sc] : 0.f;
    }
  };
  if (t_begin < t_end) fetch(t_begin, 0);

  for (int tile = t_begin; tile < t_end; ++tile) {
    const int cb = tile * kDotTC;
    f32x16 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

    for (int f0 = 0; f0 < F; f0 += kDotFC) {
      __syncthreads();  // the readers of the chunk before
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        Qs[sr + 8 * i][sc] = pre[i];
        Xs[sr + 8 * i][sc] = pre[16 + i];
      }
      __syncthreads();
      if (f0 + kDotFC < F) fetch(tile, f0 + kDotFC);
      else if (tile + 1 < t_end) fetch(tile + 1, 0);
#pragma unroll 4
      for (int kk = 0; kk < kDotFC / 2; ++kk) {  // columns f0 + 2 kk (lanes 0 .. 31) and f0 + 2 kk + 1 (lanes 32 .. 63)
        const float av = Qs[w * 32 + tx][2 * kk + h];
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Xs[b * 32 + tx][2 * kk + h], acc[b], 0, 0, 0);
      }
    }

    // offer the tile's estimates to the shortlists
    float nx[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = cb + b * 32 + tx;
      nx[b] = j < n ? a.n2x[j] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + (r & 3) + 8 * (r >> 2);
      float dm[4];
      bool any = false;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int j = cb + b * 32 + tx;
        const bool valid = j < n;
        const float d = (nq[r] + nx[b]) - 2.f * acc[b][r];
        // the row's own pair counts as exactly 0; v_sqrt_f32 as in knn_kernel
        if (MEAN) msum[r] += __builtin_amdgcn_sqrtf((valid && !(a.same && j == row)) ? fmaxf(d, 0.f) : 0.f);
        float v = valid ? d : NAN;  // a NaN fails every compare below
        if (a.self_first && j == row) v = -INFINITY;  // always shortlisted, whatever its estimate
        dm[b] = v;
        any |= v <= thr[r];
      }
      if (__ballot(any)) {
        float td = thr[r];
        int tj = list_slot<KS, 32>(lj[r], kp - 1);
#pragma unroll
        for (int b = 0; b < 4; ++b) list_offer<KS, 32>(ld[r], lj[r], dm[b], cb + b * 32 + tx, kp, td, tj);
        thr[r] = td;
      }
      __builtin_amdgcn_sched_barrier(0);  // one row at a time, as in knn_kernel
    }
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = row0 + (r & 3) + 8 * (r >> 2);
    if (row >= a.nq) continue;
    const size_t at = ((size_t)slice * a.nq + row) * kp;
#pragma unroll
    for (int m = 0; m < KS; ++m) {
      const int s = tx + 32 * m;
      if (s < kp) {
        a.l_idx[at + s] = lj[r][m];
        a.l_est[at + s] = ld[r][m];
      }
    }
    if (MEAN) {
      float v = msum[r];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
      if (tx == 0) a.l_mean[(size_t)slice * a.nq + row] = v;
    }
  }
}

// ---- bfloat16 rows: the sums on v_mfma_f32_32x32x16_bf16 --------------------------------------------------

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// A chunk is 128 query rows and 128 candidate rows of kDotBfFC = 64 columns, 128 bytes a row.  Eight lanes read one row's 128
// bytes, sixteen bytes each; thread t holds columns 8 (t & 7) .. + 7 of rows (t >> 3) + 32 i, i < 4, of each.
struct BfStage {
  uint4 q[4], x[4];
};

// Columns c .. c + 7 of a row, zeros past F and for a row that does not exist.  vec (the same in every thread): the base and
// every row are 16-byte aligned and F is a multiple of 8, so the eight are one load, inside the row or past it; otherwise
// they are read one by one (a base that is only 2-byte aligned, any F).
__device__ __forceinline__ uint4 bf_load8(const uint16_t *base, int g, bool live, int c, int F, bool vec) {
  uint32_t p[4] = {0, 0, 0, 0};
  if (live && c < F) {
    const uint16_t *row = base + (size_t)g * F;
    if (vec) {
      const uint4 v = *reinterpret_cast<const uint4 *>(row + c);
      return v;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (c + i < F) p[i >> 1] |= (uint32_t)row[c + i] << (16 * (i & 1));
  }
  return make_uint4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ void bf_fetch(const DotArgsBf16 &a, bool vec, int q0, int tile, int f0, BfStage &pre) {
  const int t = threadIdx.x, c = f0 + 8 * (t & 7), sr = t >> 3;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int g = q0 + sr + 32 * i;
    pre.q[i] = bf_load8(a.Q, g, g < a.nq, c, a.F, vec);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int g = tile * kDotTC + sr + 32 * i;
    pre.x[i] = bf_load8(a.X, g, g < a.n, c, a.F, vec);
  }
}

// s~ of the workgroup's 128 query rows (from q0) against candidate tile `tile`, in acc: the one piece of code that forms a
// pair's sum, for the prefilter and for the diagnostic entry.  A pair's sum is ceil(F / 16) instructions, columns 16 g ..
// 16 g + 15 in instruction g, ascending, zeros past F -- whatever the tile, the slice or the position in the tile.  `pre`
// holds the tile's first chunk on entry; the next chunk, or the first of tile + 1 (below t_end), is read into it while the
// MFMAs of this one run.  The LDS image is row-major with a pitch of kDotBfLd = 72 elements, 144 bytes: nine 16-byte slots,
// an odd number, so the sixteen lanes of a ds_read_b128 group -- sixteen rows, distinct mod 16 -- cover all sixteen slots
// of the 256-byte bank row.
__device__ __forceinline__ void bf_tile(const DotArgsBf16 &a, bool vec, int q0, int tile, int t_end, BfStage &pre,
                                        f32x16 (&acc)[4], uint16_t (*Qs)[kDotBfLd], uint16_t (*Xs)[kDotBfLd]) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, tx = lane & 31, h = lane >> 5;
  const int sc = 8 * (t & 7), sr = t >> 3, F = a.F;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
  for (int f0 = 0; f0 < F; f0 += kDotBfFC) {
    __syncthreads();  // the readers of the chunk before
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<uint4 *>(&Qs[sr + 32 * i][sc]) = pre.q[i];
      *reinterpret_cast<uint4 *>(&Xs[sr + 32 * i][sc]) = pre.x[i];
    }
    __syncthreads();
    int nt = tile, nf = f0 + kDotBfFC;
    if (nf >= F) {
      nt = tile + 1;
      nf = 0;
    }
    if (nt < t_end) bf_fetch(a, vec, q0, nt, nf, pre);
    const int left = (F - f0 + 15) >> 4, steps = left < kDotBfFC / 16 ? left : kDotBfFC / 16;
    for (int kk = 0; kk < steps; ++kk) {  // columns f0 + 16 kk + 8 h .. + 7 in this lane's fragment
      const bf16x8 av = *reinterpret_cast<const bf16x8 *>(&Qs[w * 32 + tx][16 * kk + 8 * h]);
#pragma unroll
      for (int b = 0; b < 4; ++b)
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, *reinterpret_cast<const bf16x8 *>(&Xs[b * 32 + tx][16 * kk + 8 * h]),
                                                         acc[b], 0, 0, 0);
    }
  }
}

__device__ __forceinline__ bool bf_vec(const DotArgsBf16 &a) {
  return ((uintptr_t)a.Q | (uintptr_t)a.X | (uintptr_t)(2 * (size_t)a.F)) % 16 == 0;
}

// What a prefilter kernel does with a finished tile of sums: register r of an accumulator is query row
// row0 + (r & 3) + 8 (r >> 2) and candidate cb + 32 b + tx; ld / lj are the rows' sorted shortlists (slot tx + 32 m), thr
// the estimate in slot kp - 1 in every lane, nq the query norms and msum the mean's partial sums.
template <int KS, bool MEAN, typename R>
__device__ __forceinline__ void offer_tile(const DotArgsT<R> &a, int cb, int row0, const f32x16 (&acc)[4], float (&ld)[16][KS],
                                           int (&lj)[16][KS], float (&thr)[16], const float (&nq)[16], float (&msum)[16]) {
  const int tx = threadIdx.x & 31, n = a.n, kp = a.kp;
  float nx[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int j = cb + b * 32 + tx;
    nx[b] = j < n ? a.n2x[j] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = row0 + (r & 3) + 8 * (r >> 2);
    float dm[4];
    bool any = false;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = cb + b * 32 + tx;
      const bool valid = j < n;
      const float d = (nq[r] + nx[b]) - 2.f * acc[b][r];
      // the row's own pair counts as exactly 0; v_sqrt_f32 as in knn_kernel
      if (MEAN) msum[r] += __builtin_amdgcn_sqrtf((valid && !(a.same && j == row)) ? fmaxf(d, 0.f) : 0.f);
      float v = valid ? d : NAN;  // a NaN fails every compare below
      if (a.self_first && j == row) v = -INFINITY;  // always shortlisted, whatever its estimate
      dm[b] = v;
      any |= v <= thr[r];
    }
    if (__ballot(any)) {
      float td = thr[r];
      int tj = list_slot<KS, 32>(lj[r], kp - 1);
#pragma unroll
      for (int b = 0; b < 4; ++b) list_offer<KS, 32>(ld[r], lj[r], dm[b], cb + b * 32 + tx, kp, td, tj);
      thr[r] = td;
    }
    __builtin_amdgcn_sched_barrier(0);  // one row at a time, as in knn_kernel
  }
}

// ... and with the finished shortlists: slice `slice` of [slices, nq, kp], and the partial means [slices, nq]
template <int KS, bool MEAN, typename R>
__device__ __forceinline__ void write_lists(const DotArgsT<R> &a, int slice, int row0, const float (&ld)[16][KS],
                                            const int (&lj)[16][KS], const float (&msum)[16]) {
  const int tx = threadIdx.x & 31, kp = a.kp;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = row0 + (r & 3) + 8 * (r >> 2);
    if (row >= a.nq) continue;
    const size_t at = ((size_t)slice * a.nq + row) * kp;
#pragma unroll
    for (int m = 0; m < KS; ++m) {
      const int s = tx + 32 * m;
      if (s < kp) {
        a.l_idx[at + s] = lj[r][m];
        a.l_est[at + s] = ld[r][m];
      }
    }
    if (MEAN) {
      float v = msum[r];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
      if (tx == 0) a.l_mean[(size_t)slice * a.nq + row] = v;
    }
  }
}

// knn_dot_prefilter_kernel for bfloat16 rows: the same workgroup, tiles, slices, shortlists and mean
template <int KS, bool MEAN>
__global__ __launch_bounds__(kDotBlock) void knn_dot_prefilter_bf16_kernel(DotArgsBf16 a) {
  __shared__ __attribute__((aligned(16))) uint16_t Qs[kDotTQ][kDotBfLd];
  __shared__ __attribute__((aligned(16))) uint16_t Xs[kDotTC][kDotBfLd];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, h = lane >> 5;
  const int q0 = blockIdx.x * kDotTQ, slice = blockIdx.y;
  const int tiles = (a.n + kDotTC - 1) / kDotTC;
  const int t_begin = (int)((int64_t)tiles * slice / a.slices), t_end = (int)((int64_t)tiles * (slice + 1) / a.slices);
  const bool vec = bf_vec(a);

  const int row0 = q0 + w * 32 + 4 * h;
  float ld[16][KS];
  int lj[16][KS];
  float thr[16];
  float nq[16], msum[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int m = 0; m < KS; ++m) {
      ld[r][m] = INFINITY;
      lj[r][m] = INT_MAX;
    }
    thr[r] = INFINITY;
    msum[r] = 0.f;
    const int row = row0 + (r & 3) + 8 * (r >> 2);
    nq[r] = row < a.nq ? a.n2q[row] : 0.f;
  }

  BfStage pre;
  if (t_begin < t_end) bf_fetch(a, vec, q0, t_begin, 0, pre);
  for (int tile = t_begin; tile < t_end; ++tile) {
    f32x16 acc[4];
    bf_tile(a, vec, q0, tile, t_end, pre, acc, Qs, Xs);
    offer_tile<KS, MEAN>(a, tile * kDotTC, row0, acc, ld, lj, thr, nq, msum);
  }
  write_lists<KS, MEAN>(a, slice, row0, ld, lj, msum);
}

// The diagnostic entry's kernel: every pair's raw estimate d~ from bf_tile's sums, workgroup (x, y) the 128 query rows x and
// the candidate tile y, and the rows' E1b.
__global__ __launch_bounds__(kDotBlock) void knn_dot_estimates_bf16_kernel(DotArgsBf16 a, float *__restrict__ est,
                                                                           float *__restrict__ e1) {
  __shared__ __attribute__((aligned(16))) uint16_t Qs[kDotTQ][kDotBfLd];
  __shared__ __attribute__((aligned(16))) uint16_t Xs[kDotTC][kDotBfLd];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, tx = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * kDotTQ, tile = blockIdx.y, cb = tile * kDotTC;
  const int row0 = q0 + w * 32 + 4 * h;
  const bool vec = bf_vec(a);
  BfStage pre;
  bf_fetch(a, vec, q0, tile, 0, pre);
  f32x16 acc[4];
  bf_tile(a, vec, q0, tile, tile + 1, pre, acc, Qs, Xs);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = row0 + (r & 3) + 8 * (r >> 2);
    if (row >= a.nq) continue;
    const float nq = a.n2q[row];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = cb + b * 32 + tx;
      if (j < a.n) est[(size_t)row * a.n + j] = (nq + a.n2x[j]) - 2.f * acc[b][r];
    }
    if (tile == 0 && tx == 0) e1[row] = dot_e1b(a.F, nq + a.n2max[0]);
  }
}

// d2(row, j) of this lane's candidate j (j < 0: none) in knn_kernel's arithmetic.  The 64 candidate rows are staged through
// LDS 64 columns at a time with coalesced reads, then every lane walks its own row in column order.
template <typename R>
__device__ __forceinline__ float exact_batch(const DotArgsT<R> &a, int row, int j, float (*tile)[kDotRerankRows + 1], float *qs) {
  const int lane = threadIdx.x, F = a.F;
  float acc = 0.f;
  for (int f0 = 0; f0 < F; f0 += kDotRerankRows) {
    __syncthreads();
    const bool col = f0 + lane < F;
    qs[lane] = col ? widen(a.Q[(size_t)row * F + f0 + lane]) : 0.f;
    for (int r = 0; r < kDotRerankRows; ++r) {
      const int jr = __shfl(j, r);
      if (jr >= 0) tile[r][lane] = col ? widen(a.X[(size_t)jr * F + f0 + lane]) : 0.f;
    }
    __syncthreads();
    if (j >= 0)
#pragma unroll 8
      for (int c = 0; c < kDotRerankRows; ++c) {  // a column past F is 0 - 0: adds +0
        const float d = qs[c] - tile[lane][c];
        acc = fmaf(d, d, acc);
      }
  }
  return acc;
}

// This lane's candidate j (ok: it has one) goes to the wave's best-k list under (d2, j), slot s in lane s, at its exact
// distance; the row's own pair goes before every distance and is written out as 0.
template <typename R>
__device__ __forceinline__ void rerank_offer(const DotArgsT<R> &a, int row, bool ok, int j, float (&bd)[1], int (&bj)[1],
                                             float (*tile)[kDotRerankRows + 1], float *qs) {
  const float d2 = exact_batch(a, row, ok ? j : -1, tile, qs);
  float td = list_slot<1, 64>(bd, a.k - 1);
  int tj = list_slot<1, 64>(bj, a.k - 1);
  list_offer<1, 64>(bd, bj, !ok ? NAN : (a.self_first && j == row) ? -1.f : d2, j, a.k, td, tj);
}

template <typename R>
__global__ __launch_bounds__(kDotRerankRows) void knn_dot_rerank_kernel(DotArgsT<R> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dot_smem[];
  float(*tile)[kDotRerankRows + 1] = reinterpret_cast<float(*)[kDotRerankRows + 1]>(dot_smem);
  float *qs = reinterpret_cast<float *>(dot_smem) + kDotRerankRows * (kDotRerankRows + 1);
  float *cd = qs + kDotRerankRows;                  // the merged shortlist [kp <= 96]
  int *cj = reinterpret_cast<int *>(cd + 96);
  float *sd = reinterpret_cast<float *>(cj + 96);  // the slices' lists [slices, kp]
  const int lane = threadIdx.x, row = blockIdx.x;
  const int k = a.k, kp = a.kp, n = a.n, L = a.slices * kp;
  int *sj = reinterpret_cast<int *>(sd + L);

  for (int e = lane; e < L; e += 64) {
    const int s = e / kp, p = e - s * kp;
    const size_t at = ((size_t)s * a.nq + row) * kp + p;
    sd[e] = a.l_est[at];
    sj[e] = a.l_idx[at];
  }
  __syncthreads();
  // every entry goes to its place in the merge under (d~, j)
  for (int e = lane; e < L; e += 64) {
    const int s = e / kp, p = e - s * kp;
    const int rank = merged_rank(sd, sj, a.slices, kp, s, p);
    if (rank < kp) {
      cd[rank] = sd[e];
      cj[rank] = sj[e];
    }
  }
  __syncthreads();

  // rank the shortlist by the exact distances
  float bd[1] = {INFINITY};
  int bj[1] = {INT_MAX};
  bool bad = false;  // a slot that holds no candidate: an estimate was not a number
  for (int base = 0; base < kp; base += 64) {
    const int e = base + lane;
    const int j = e < kp ? cj[e] : -1;
    const bool ok = j >= 0 && j < n;
    bad |= e < kp && !ok;
    rerank_offer(a, row, ok, j, bd, bj, tile, qs);
  }

  // Every candidate outside the shortlist has d~ >= T, so d2 >= (T - E1) (1 - (F + 2) u) >= T - Ei:
  //   E1 = C u (n2q + n2max) + (F + 2) 2^-146,  C = (2 F + 4) (1 + 1/64) rounded up,  u = 2^-24;  bfloat16 rows: dot_e1b
  //   Ei = E1 + (F + 4) u max(T, 0)
  bool certified = !__any(bad);
  if (certified && n > kp) {
    const float u = 5.9604644775390625e-8f;  // 2^-24
    const float T = cd[kp - 1];
    const float kth = list_slot<1, 64>(bd, k - 1);
    const float sum = a.n2q[row] + a.n2max[0];
    float E1;
    if constexpr (sizeof(R) == 4) {
      const int c2 = 2 * a.F + 4;
      const float C = (float)(c2 + (c2 >> 6) + 1) * u;
      E1 = C * sum + (float)(a.F + 2) * 1.1210387714598537e-44f;  // 2^-146
    } else {
      E1 = dot_e1b(a.F, sum);
    }
    const float Ei = E1 + ((float)(a.F + 4) * u) * fmaxf(T, 0.f);
    certified = sum < 1e37f && kth < T - Ei;  // strictly; an infinite or NaN bound fails both
  }
  if (!certified) {
    bd[0] = INFINITY;
    bj[0] = INT_MAX;
    for (int base = 0; base < n; base += 64) {
      const int j = base + lane;
      rerank_offer(a, row, j < n, j, bd, bj, tile, qs);
    }
  }
  if (lane < k) {
    a.idx[(size_t)row * k + lane] = bj[0];
    a.dist[(size_t)row * k + lane] = bd[0] < 0.f ? 0.f : bd[0];
  }
  if (lane == 0) {
    if (a.fallback) a.fallback[row] = certified ? 0 : 1;
    if (a.mean) {
      float v = a.l_mean[row];
      for (int s = 1; s < a.slices; ++s) v += a.l_mean[(size_t)s * a.nq + row];
      a.mean[row] = v / (float)n;
    }
  }
}

// the row type's prefilter kernel
template <int KS, typename R>
void launch_prefilter(const DotArgsT<R> &a, dim3 grid, bool mean, hipStream_t s) {
  void (*kernel)(DotArgsT<R>);
  if constexpr (sizeof(R) == 4) kernel = mean ? knn_dot_prefilter_kernel<KS, true> : knn_dot_prefilter_kernel<KS, false>;
  else kernel = mean ? knn_dot_prefilter_bf16_kernel<KS, true> : knn_dot_prefilter_bf16_kernel<KS, false>;
  hipLaunchKernelGGL(kernel, grid, dim3(kDotBlock), 0, s, a);
}

// The norms of the candidates, their maximum and (Q != X) the norms of the query rows, into a's n2x / n2max / n2q; bmax is
// scratch of ceil(n / 64) floats.
template <typename R>
void launch_norms(const DotArgsT<R> &a, float *bmax, hipStream_t s) {
  const int nb = (a.n + kDotNormRows - 1) / kDotNormRows;
  hipLaunchKernelGGL(knn_dot_norm_kernel<R>, dim3((unsigned)nb), dim3(256), 0, s, a.X, a.n, a.F, const_cast<float *>(a.n2x), bmax);
  hipLaunchKernelGGL(knn_dot_max_kernel, dim3(1), dim3(256), 0, s, (const float *)bmax, nb, const_cast<float *>(a.n2max));
  if (!a.same)
    hipLaunchKernelGGL(knn_dot_norm_kernel<R>, dim3((unsigned)((a.nq + kDotNormRows - 1) / kDotNormRows)), dim3(256), 0, s, a.Q,
                       a.nq, a.F, const_cast<float *>(a.n2q), (float *)nullptr);
}

// hg_knn_dot_f32 and hg_knn_dot_bf16: the refusals, the workspace and the launches, once for both row types
template <typename R>
int knn_dot_run(const char *entry, const char *ws_entry, const R *Q, int32_t nq, const R *X, int32_t n, int32_t F, int32_t k,
                int32_t self_first, int32_t cand_slices, int32_t *idx, float *dist, float *mean_dist, int32_t *fallback,
                void *workspace, size_t workspace_bytes, hg_stream_t stream) {
  if (const int st = knn_refusal({entry, Q, X, idx, dist, nq, n, F, k, self_first, cand_slices}, kDotMaxF, nullptr, 0)) return st;
  const bool same = Q == X && nq == n;
  if (sizeof(R) == 2 && ((uintptr_t)Q % 2 || (uintptr_t)X % 2)) return fail(entry, HG_ERR_UNSUPPORTED, "Q and X must be 2-byte aligned");
  for (const void *p : {sizeof(R) == 4 ? (const void *)Q : nullptr, sizeof(R) == 4 ? (const void *)X : nullptr, (const void *)idx,
                        (const void *)dist, (const void *)mean_dist, (const void *)fallback, (const void *)workspace})
    if ((uintptr_t)p % 4)
      return fail(entry, HG_ERR_UNSUPPORTED,
                  std::string(sizeof(R) == 4 ? "Q, X, " : "") + "idx, dist, mean_dist, fallback and the workspace must be 4-byte aligned");
  const int slices = knn_dot_slices(nq, n, cand_slices);
  const KnnDotLayout L = knn_dot_layout(nq, n, k, slices);
  if (!workspace || workspace_bytes < L.total)
    return fail(entry, HG_ERR_WORKSPACE, "workspace of " + std::to_string(workspace_bytes) + " bytes, " + ws_entry + " asks for " +
                                             std::to_string(L.total));

  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  float *n2x = reinterpret_cast<float *>(ws + L.n2x), *n2q = reinterpret_cast<float *>(ws + L.n2q);
  DotArgsT<R> a{};
  a.Q = Q;
  a.X = X;
  a.nq = nq;
  a.n = n;
  a.F = F;
  a.k = k;
  a.kp = L.kp;
  a.slices = slices;
  a.self_first = self_first ? 1 : 0;
  a.same = same ? 1 : 0;
  a.n2x = n2x;
  a.n2q = same ? n2x : n2q;
  a.n2max = reinterpret_cast<float *>(ws + L.n2max);
  a.l_idx = reinterpret_cast<int32_t *>(ws + L.idx);
  a.l_est = reinterpret_cast<float *>(ws + L.est);
  a.l_mean = mean_dist ? reinterpret_cast<float *>(ws + L.mean) : nullptr;
  a.idx = idx;
  a.dist = dist;
  a.mean = mean_dist;
  a.fallback = fallback;

  launch_norms(a, reinterpret_cast<float *>(ws + L.bmax), s);
  const dim3 grid((unsigned)((nq + kDotTQ - 1) / kDotTQ), (unsigned)slices);
  const bool mean = mean_dist != nullptr;
  const int ks = (L.kp + 31) / 32;
  if (ks == 1) launch_prefilter<1>(a, grid, mean, s);
  else if (ks == 2) launch_prefilter<2>(a, grid, mean, s);
  else launch_prefilter<3>(a, grid, mean, s);
  const size_t lds = (size_t)(kDotRerankRows * (kDotRerankRows + 1) + kDotRerankRows + 2 * 96) * 4 + (size_t)slices * L.kp * 8;
  hipLaunchKernelGGL(knn_dot_rerank_kernel<R>, dim3((unsigned)nq), dim3(kDotRerankRows), lds, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(entry, HG_ERR_HIP, std::string("launch: ") + hipGetErrorString(e));
  return HG_OK;
}

}  // namespace
}  // namespace hg

extern "C" {

size_t hg_knn_dot_workspace_bytes(int32_t nq, int32_t n, int32_t F, int32_t k, int32_t cand_slices) {
  if (!hg::knn_sizes_ok(nq, n, F, k, cand_slices, hg::kDotMaxF)) return 0;
  return hg::knn_dot_layout(nq, n, k, hg::knn_dot_slices(nq, n, cand_slices)).total;
}

size_t hg_knn_dot_bf16_workspace_bytes(int32_t nq, int32_t n, int32_t F, int32_t k, int32_t cand_slices) {
  return hg_knn_dot_workspace_bytes(nq, n, F, k, cand_slices);  // the same pieces: norms, shortlists and partial means
}

int hg_knn_dot_f32(const float *Q, int32_t nq, const float *X, int32_t n, int32_t F, int32_t k, int32_t self_first,
                   int32_t cand_slices, int32_t *idx, float *dist, float *mean_dist, int32_t *fallback, void *workspace,
                   size_t workspace_bytes, hg_stream_t stream) {
  return hg::knn_dot_run("hg_knn_dot_f32", "hg_knn_dot_workspace_bytes", Q, nq, X, n, F, k, self_first, cand_slices, idx, dist,
                         mean_dist, fallback, workspace, workspace_bytes, stream);
}

int hg_knn_dot_bf16(const uint16_t *Q, int32_t nq, const uint16_t *X, int32_t n, int32_t F, int32_t k, int32_t self_first,
                    int32_t cand_slices, int32_t *idx, float *dist, float *mean_dist, int32_t *fallback, void *workspace,
                    size_t workspace_bytes, hg_stream_t stream) {
  return hg::knn_dot_run("hg_knn_dot_bf16", "hg_knn_dot_bf16_workspace_bytes", Q, nq, X, n, F, k, self_first, cand_slices, idx,
                         dist, mean_dist, fallback, workspace, workspace_bytes, stream);
}

int hg_knn_dot_estimates_bf16(const uint16_t *Q, int32_t nq, const uint16_t *X, int32_t n, int32_t F, float *est, float *e1,
                              hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_knn_dot_estimates_bf16";
  if (!Q || !X || !est || !e1) return fail(entry, HG_ERR_INVALID, "null Q, X, est or e1");
  if (nq < 1 || n < 1 || F < 1) return fail(entry, HG_ERR_INVALID, "nq, n and F must be at least 1");
  if (F > kDotMaxF)
    return fail(entry, HG_ERR_INVALID, "F = " + std::to_string(F) + " is above " + std::to_string(kDotMaxF) + ", the width the error bound is derived for");
  if ((int64_t)nq * n > kDotEstimatesMax)
    return fail(entry, HG_ERR_UNSUPPORTED, "a diagnostic: nq * n must be at most " + std::to_string(kDotEstimatesMax));
  if ((uintptr_t)Q % 2 || (uintptr_t)X % 2 || (uintptr_t)est % 4 || (uintptr_t)e1 % 4)
    return fail(entry, HG_ERR_UNSUPPORTED, "Q and X must be 2-byte aligned, est and e1 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const KnnDotLayout L = knn_dot_layout(nq, n, 1, 1);  // for the norms' places; the lists are not used
  unsigned char *ws = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&ws), L.idx);
  if (e != hipSuccess) return fail(entry, HG_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
  DotArgsBf16 a{};
  a.Q = Q;
  a.X = X;
  a.nq = nq;
  a.n = n;
  a.F = F;
  a.same = Q == X && nq == n;
  a.n2x = reinterpret_cast<float *>(ws + L.n2x);
  a.n2q = a.same ? a.n2x : reinterpret_cast<float *>(ws + L.n2q);
  a.n2max = reinterpret_cast<float *>(ws + L.n2max);
  launch_norms(a, reinterpret_cast<float *>(ws + L.bmax), s);
  const dim3 grid((unsigned)((nq + kDotTQ - 1) / kDotTQ), (unsigned)((n + kDotTC - 1) / kDotTC));
  hipLaunchKernelGGL(knn_dot_estimates_bf16_kernel, grid, dim3(kDotBlock), 0, s, a, est, e1);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // the norms' memory goes back below
  (void)hipFree(ws);
  if (e != hipSuccess) return fail(entry, HG_ERR_HIP, std::string("launch: ") + hipGetErrorString(e));
  return HG_OK;
}

}  // extern "C"
