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

struct DotArgs {
  const float *Q, *X;
  int32_t nq, n, F, k, kp, slices, self_first, same;
  const float *n2q, *n2x, *n2max;
  int32_t *l_idx;  // the slices' shortlists [slices, nq, kp], each sorted under (d~, j)
  float *l_est;
  float *l_mean;  // [slices, nq] partial sums of sqrt(max(d~, 0)), or null
  int32_t *idx;
  float *dist, *mean;
  int32_t *fallback;
};

__global__ __launch_bounds__(256) void knn_dot_norm_kernel(const float *__restrict__ X, int n, int F, float *__restrict__ n2,
                                                           float *__restrict__ bmax) {
  __shared__ float tile[kDotNormRows][kDotNormRows + 1];
  const int t = threadIdx.x, r0 = blockIdx.x * kDotNormRows;
  float acc = 0.f;
  for (int f0 = 0; f0 < F; f0 += kDotNormRows) {
    __syncthreads();
    for (int e = t; e < kDotNormRows * kDotNormRows; e += 256) {
      const int r = e >> 6, c = e & 63, j = r0 + r;
      tile[r][c] = (j < n && f0 + c < F) ? X[(size_t)j * F + f0 + c] : 0.f;
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

// d2(row, j) of this lane's candidate j (j < 0: none) in knn_kernel's arithmetic.  The 64 candidate rows are staged through
// LDS 64 columns at a time with coalesced reads, then every lane walks its own row in column order.
__device__ __forceinline__ float exact_batch(const DotArgs &a, int row, int j, float (*tile)[kDotRerankRows + 1], float *qs) {
  const int lane = threadIdx.x, F = a.F;
  float acc = 0.f;
  for (int f0 = 0; f0 < F; f0 += kDotRerankRows) {
    __syncthreads();
    const bool col = f0 + lane < F;
    qs[lane] = col ? a.Q[(size_t)row * F + f0 + lane] : 0.f;
    for (int r = 0; r < kDotRerankRows; ++r) {
      const int jr = __shfl(j, r);
      if (jr >= 0) tile[r][lane] = col ? a.X[(size_t)jr * F + f0 + lane] : 0.f;
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
__device__ __forceinline__ void rerank_offer(const DotArgs &a, int row, bool ok, int j, float (&bd)[1], int (&bj)[1],
                                             float (*tile)[kDotRerankRows + 1], float *qs) {
  const float d2 = exact_batch(a, row, ok ? j : -1, tile, qs);
  float td = list_slot<1, 64>(bd, a.k - 1);
  int tj = list_slot<1, 64>(bj, a.k - 1);
  list_offer<1, 64>(bd, bj, !ok ? NAN : (a.self_first && j == row) ? -1.f : d2, j, a.k, td, tj);
}

__global__ __launch_bounds__(kDotRerankRows) void knn_dot_rerank_kernel(DotArgs a) {
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
  //   E1 = C u (n2q + n2max) + (F + 2) 2^-146,  C = (2 F + 4) (1 + 1/64) rounded up,  u = 2^-24
  //   Ei = E1 + (F + 4) u max(T, 0)
  bool certified = !__any(bad);
  if (certified && n > kp) {
    const float u = 5.9604644775390625e-8f;  // 2^-24
    const float T = cd[kp - 1];
    const float kth = list_slot<1, 64>(bd, k - 1);
    const float sum = a.n2q[row] + a.n2max[0];
    const int c2 = 2 * a.F + 4;
    const float C = (float)(c2 + (c2 >> 6) + 1) * u;
    const float E1 = C * sum + (float)(a.F + 2) * 1.1210387714598537e-44f;  // 2^-146
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

template <int KS>
void launch_prefilter(const DotArgs &a, dim3 grid, bool mean, hipStream_t s) {
  if (mean) hipLaunchKernelGGL((knn_dot_prefilter_kernel<KS, true>), grid, dim3(kDotBlock), 0, s, a);
  else hipLaunchKernelGGL((knn_dot_prefilter_kernel<KS, false>), grid, dim3(kDotBlock), 0, s, a);
}

}  // namespace
}  // namespace hg

extern "C" {

size_t hg_knn_dot_workspace_bytes(int32_t nq, int32_t n, int32_t F, int32_t k, int32_t cand_slices) {
  if (!hg::knn_sizes_ok(nq, n, F, k, cand_slices, hg::kDotMaxF)) return 0;
  return hg::knn_dot_layout(nq, n, k, hg::knn_dot_slices(nq, n, cand_slices)).total;
}

int hg_knn_dot_f32(const float *Q, int32_t nq, const float *X, int32_t n, int32_t F, int32_t k, int32_t self_first,
                   int32_t cand_slices, int32_t *idx, float *dist, float *mean_dist, int32_t *fallback, void *workspace,
                   size_t workspace_bytes, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_knn_dot_f32";
  if (const int st = knn_refusal({entry, Q, X, idx, dist, nq, n, F, k, self_first, cand_slices}, kDotMaxF, nullptr, 0)) return st;
  const bool same = Q == X && nq == n;
  for (const void *p : {(const void *)Q, (const void *)X, (const void *)idx, (const void *)dist, (const void *)mean_dist,
                        (const void *)fallback, (const void *)workspace})
    if ((uintptr_t)p % 4)
      return fail(entry, HG_ERR_UNSUPPORTED, "Q, X, idx, dist, mean_dist, fallback and the workspace must be 4-byte aligned");
  const int slices = knn_dot_slices(nq, n, cand_slices);
  const KnnDotLayout L = knn_dot_layout(nq, n, k, slices);
  if (!workspace || workspace_bytes < L.total)
    return fail(entry, HG_ERR_WORKSPACE, "workspace of " + std::to_string(workspace_bytes) +
                                             " bytes, hg_knn_dot_workspace_bytes asks for " + std::to_string(L.total));

  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  float *n2x = reinterpret_cast<float *>(ws + L.n2x), *n2q = reinterpret_cast<float *>(ws + L.n2q);
  float *bmax = reinterpret_cast<float *>(ws + L.bmax), *n2max = reinterpret_cast<float *>(ws + L.n2max);
  DotArgs a{};
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
  a.n2max = n2max;
  a.l_idx = reinterpret_cast<int32_t *>(ws + L.idx);
  a.l_est = reinterpret_cast<float *>(ws + L.est);
  a.l_mean = mean_dist ? reinterpret_cast<float *>(ws + L.mean) : nullptr;
  a.idx = idx;
  a.dist = dist;
  a.mean = mean_dist;
  a.fallback = fallback;

  const int nb = (n + kDotNormRows - 1) / kDotNormRows;
  hipLaunchKernelGGL(knn_dot_norm_kernel, dim3((unsigned)nb), dim3(256), 0, s, X, n, F, n2x, bmax);
  hipLaunchKernelGGL(knn_dot_max_kernel, dim3(1), dim3(256), 0, s, (const float *)bmax, nb, n2max);
  if (!same)
    hipLaunchKernelGGL(knn_dot_norm_kernel, dim3((unsigned)((nq + kDotNormRows - 1) / kDotNormRows)), dim3(256), 0, s, Q, nq, F,
                       n2q, (float *)nullptr);
  const dim3 grid((unsigned)((nq + kDotTQ - 1) / kDotTQ), (unsigned)slices);
  const bool mean = mean_dist != nullptr;
  const int ks = (L.kp + 31) / 32;
  if (ks == 1) launch_prefilter<1>(a, grid, mean, s);
  else if (ks == 2) launch_prefilter<2>(a, grid, mean, s);
  else launch_prefilter<3>(a, grid, mean, s);
  const size_t lds = (size_t)(kDotRerankRows * (kDotRerankRows + 1) + kDotRerankRows + 2 * 96) * 4 + (size_t)slices * L.kp * 8;
  hipLaunchKernelGGL(knn_dot_rerank_kernel, dim3((unsigned)nq), dim3(kDotRerankRows), lds, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(entry, HG_ERR_HIP, std::string("launch: ") + hipGetErrorString(e));
  return HG_OK;
}

}  // extern "C"
