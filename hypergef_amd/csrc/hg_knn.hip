// k nearest neighbours of every query row among the candidate rows, without the distance matrix (include/hg_aggr.h,
// hg_knn_f32).  d2(i, j) = sum_c (Q[i, c] - X[j, c])^2 in float32, in the difference form, summed over c = 0, 1, .. F - 1
// in that order into one accumulator with an explicit fma (the library is built without contraction): the bits of
// d2(i, j) depend on the two rows and on F alone, not on the tile the pair lands in nor on the split of the candidates.
// Selection is under the total order (d2, j), so the result is one bit pattern however the work is cut.  No atomics.
//
// knn_kernel: a workgroup owns kKnnTQ = 64 query rows and one slice of its candidate tiles (kKnnTC = 256 rows each).
// Query and candidate rows are staged in LDS kKnnFC = 32 columns at a time, column-major, so that a lane reads its 8
// query values (a broadcast) and its 2 x 4 candidate values with four 16-byte reads per column and feeds 64
// subtract / fma pairs with them, two pairs per packed instruction.  Lane (ty, tx) holds query rows 8 ty .. 8 ty + 7 and
// candidates 4 tx .. 4 tx + 3 and 128 + 4 tx .. 128 + 4 tx + 3 of the tile: the 256 candidates of a query row sit in the
// 32 lanes of one half wave.  Those 32 lanes also hold the row's best-k list, sorted, slot s in lane s % 32: an offer
// is one compare against the row's k-th distance (kept in every lane); the rare survivor is inserted by the half wave
// with one shift by a lane (list_offer<KS, 32>).  The other slices' lists go to the workspace and knn_merge_kernel ranks
// every entry of a row's lists against the others under the same order (merged_rank).  The list and the rank are
// hg_knn_list.h's, shared with hg_knn_dot.hip.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>

#include "hg_aggr.h"
#include "hg_internal.h"
#include "hg_knn.h"
#include "hg_knn_list.h"

namespace hg {

KnnLayout knn_layout(int64_t nq, int64_t n, int k, int slices) {
  KnnLayout L;
  const size_t seg_bytes = nq == n ? (((size_t)n + 1) * 4 + 255) / 256 * 256 : 0;  // segments need Q == X
  const size_t extra = slices > 1 ? (size_t)(slices - 1) : 0;
  L.seg = 0;
  L.idx = seg_bytes;
  L.dist = L.idx + extra * (size_t)nq * (size_t)k * 4;
  L.mean = L.dist + extra * (size_t)nq * (size_t)k * 4;
  L.total = L.mean + extra * (size_t)nq * 4;
  return L;
}

int knn_auto_slices(int64_t nq, int64_t n) {
  const int64_t groups = (nq + kKnnTQ - 1) / kKnnTQ, tiles = (n + kKnnTC - 1) / kKnnTC;
  return groups <= 128 && tiles >= 2 ? 2 : 1;
}

bool knn_sizes_ok(int32_t nq, int32_t n, int32_t F, int32_t k, int32_t cand_slices, int32_t max_F) {
  return nq >= 1 && n >= 1 && F >= 1 && (!max_F || F <= max_F) && k >= 1 && k <= kKnnMaxK && k <= n && cand_slices >= 0 &&
         cand_slices <= kKnnMaxSlices;
}

int knn_refusal(const KnnCall &c, int32_t max_F, const int32_t *seg, int32_t B) {
  const int32_t n = c.n, k = c.k;
  if (!c.Q || !c.X || !c.idx || !c.dist) return fail(c.entry, HG_ERR_INVALID, "null Q, X, idx or dist");
  if (c.nq < 1 || n < 1 || c.F < 1) return fail(c.entry, HG_ERR_INVALID, "nq, n and F must be at least 1");
  if (max_F && c.F > max_F)
    return fail(c.entry, HG_ERR_INVALID, "F = " + std::to_string(c.F) + " is above " + std::to_string(max_F) + ", the width the error bound is derived for");
  if (k < 1 || k > kKnnMaxK) return fail(c.entry, HG_ERR_INVALID, "k must be in 1 .. 64, got " + std::to_string(k));
  if (k > n) return fail(c.entry, HG_ERR_INVALID, "k = " + std::to_string(k) + " exceeds the n = " + std::to_string(n) + " candidates");
  if (c.cand_slices < 0) return fail(c.entry, HG_ERR_INVALID, "cand_slices must be 0 (auto) or positive");
  const bool same = c.Q == c.X && c.nq == n;
  if (c.self_first && !same) return fail(c.entry, HG_ERR_INVALID, "self_first needs Q == X (the same pointer, nq == n)");
  if (seg) {
    if (!same) return fail(c.entry, HG_ERR_INVALID, "seg needs Q == X (the same pointer, nq == n)");
    if (B < 1 || seg[0] != 0 || seg[B] != n) return fail(c.entry, HG_ERR_INVALID, "seg must have B >= 1, seg[0] = 0 and seg[B] = n");
    for (int32_t b = 0; b < B; ++b)
      if (seg[b + 1] < seg[b]) return fail(c.entry, HG_ERR_INVALID, "seg must ascend (seg[" + std::to_string(b + 1) + "] < seg[" + std::to_string(b) + "])");
    for (int32_t b = 0; b < B; ++b)
      if (seg[b + 1] - seg[b] < k)
        return fail(c.entry, HG_ERR_INVALID, "segment " + std::to_string(b) + " has " + std::to_string(seg[b + 1] - seg[b]) +
                                                 " rows, fewer than k = " + std::to_string(k));
  }
  if (c.cand_slices > kKnnMaxSlices)
    return fail(c.entry, HG_ERR_UNSUPPORTED, "cand_slices above " + std::to_string(kKnnMaxSlices) + " is not implemented");
  return HG_OK;
}

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));

struct KnnArgs {
  const float *Q, *X;
  const int32_t *seg;  // device copy of the offsets [B + 1], or null: every row competes with all n
  int32_t nq, n, F, k, B, slices, self_first;
  // slice 0's list and partial mean, and the final result (no __restrict__: the merge reads and writes them)
  int32_t *idx;
  float *dist, *mean;
  int32_t *ws_idx;  // slices 1 .. : [slices - 1, nq, k]
  float *ws_dist;
  float *ws_mean;  // [slices - 1, nq]
};

// the candidates [lo, hi) of row i: its segment, or all n
__device__ __forceinline__ void row_range(const int32_t *seg, int B, int n, int i, int &lo, int &hi) {
  if (!seg) {
    lo = 0;
    hi = n;
    return;
  }
  int a = 0, b = B;  // seg[a] <= i < seg[b]
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (seg[m] <= i) a = m;
    else b = m;
  }
  lo = seg[a];
  hi = seg[b];
}

// KS: list slots per lane (k <= 32 KS); MEAN: also sum sqrt(d2) over every candidate of the row
template <int KS, bool MEAN>
__global__ __launch_bounds__(kKnnBlock) void knn_kernel(KnnArgs a) {
  __shared__ __attribute__((aligned(16))) float Qs[kKnnFC][kKnnTQ];
  __shared__ __attribute__((aligned(16))) float Xs[kKnnFC][kKnnTC];
  __shared__ int s_lo[kKnnTQ], s_hi[kKnnTQ];
  const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
  const int q0 = blockIdx.x * kKnnTQ;
  const int slice = blockIdx.y;
  const int F = a.F, k = a.k;

  if (t < kKnnTQ) {
    int lo, hi;
    row_range(a.seg, a.B, a.n, min(q0 + t, a.nq - 1), lo, hi);
    s_lo[t] = lo;
    s_hi[t] = hi;
  }
  __syncthreads();
  // segments ascend with the rows: the tile's candidates are one range, cut into tiles from its own start
  const int c_lo = s_lo[0], c_hi = s_hi[kKnnTQ - 1];
  const int tiles = (c_hi - c_lo + kKnnTC - 1) / kKnnTC;
  const int t_begin = (int)((int64_t)tiles * slice / a.slices), t_end = (int)((int64_t)tiles * (slice + 1) / a.slices);

  float ld[8][KS];  // the sorted list of query row 8 ty + qi: slot tx + 32 m
  int lj[8][KS];
  float thr[8];  // the distance in slot k - 1, in every lane
  float msum[8];
#pragma unroll
  for (int qi = 0; qi < 8; ++qi) {
#pragma unroll
    for (int m = 0; m < KS; ++m) {
      ld[qi][m] = INFINITY;
      lj[qi][m] = INT_MAX;
    }
    thr[qi] = INFINITY;
    msum[qi] = 0.f;
  }

  for (int tile = t_begin; tile < t_end; ++tile) {
    const int cb = c_lo + tile * kKnnTC;
    v2f acc[8][4];
#pragma unroll
    for (int qi = 0; qi < 8; ++qi)
#pragma unroll
      for (int p = 0; p < 4; ++p) acc[qi][p] = v2f{0.f, 0.f};

    for (int f0 = 0; f0 < F; f0 += kKnnFC) {
      __syncthreads();  // the readers of the chunk before
      {  // candidate row cb + t, 32 columns; rows past the range and columns past F are zeros
        const int j = cb + t;
        const bool ok = j < c_hi;
        const float *src = a.X + (size_t)(ok ? j : 0) * F + f0;
#pragma unroll
        for (int c = 0; c < kKnnFC; ++c) Xs[c][t] = (ok && f0 + c < F) ? src[c] : 0.f;
      }
      {  // query row q0 + (t & 63), 8 columns
        const int r = t & 63, cg = (t >> 6) * 8, i = q0 + r;
        const bool ok = i < a.nq;
        const float *src = a.Q + (size_t)(ok ? i : 0) * F + f0 + cg;
#pragma unroll
        for (int c = 0; c < 8; ++c) Qs[cg + c][r] = (ok && f0 + cg + c < F) ? src[c] : 0.f;
      }
      __syncthreads();
#pragma unroll 2
      for (int c = 0; c < kKnnFC; ++c) {
        const float4 qa = *reinterpret_cast<const float4 *>(&Qs[c][ty * 8]);
        const float4 qb = *reinterpret_cast<const float4 *>(&Qs[c][ty * 8 + 4]);
        const float4 xa = *reinterpret_cast<const float4 *>(&Xs[c][tx * 4]);
        const float4 xb = *reinterpret_cast<const float4 *>(&Xs[c][128 + tx * 4]);
        const float q[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
        v2f x[4];
        x[0] = v2f{xa.x, xa.y};
        x[1] = v2f{xa.z, xa.w};
        x[2] = v2f{xb.x, xb.y};
        x[3] = v2f{xb.z, xb.w};
#pragma unroll
        for (int qi = 0; qi < 8; ++qi)
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const v2f d = v2f{q[qi], q[qi]} - x[p];
            acc[qi][p] = __builtin_elementwise_fma(d, d, acc[qi][p]);
          }
      }
    }

    // offer the tile's distances to the lists
#pragma unroll
    for (int qi = 0; qi < 8; ++qi) {
      const int row = q0 + ty * 8 + qi;
      const int lo = s_lo[ty * 8 + qi], hi = s_hi[ty * 8 + qi];
      float dm[8];
      bool any = false;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int j = cb + (jj < 4 ? tx * 4 + jj : 128 + tx * 4 + (jj - 4));
        const bool valid = j >= lo && j < hi;
        const float d = (jj & 1) ? acc[qi][jj >> 1].y : acc[qi][jj >> 1].x;
        // v_sqrt_f32: 1 ulp, a d2 below the smallest normal counts as 0.  sqrtf's correctly rounded expansion, 64 times a
        // tile, takes the kernel to 256 registers
        if (MEAN) msum[qi] += __builtin_amdgcn_sqrtf(valid ? d : 0.f);
        float v = valid ? d : NAN;  // a NaN fails every compare below
        if (a.self_first && j == row) v = -1.f;  // before every distance; written out as 0
        dm[jj] = v;
        any |= v <= thr[qi];
      }
      if (__ballot(any)) {
        float td = thr[qi];
        int tj = list_slot<KS, 32>(lj[qi], k - 1);
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          const int j = cb + (jj < 4 ? tx * 4 + jj : 128 + tx * 4 + (jj - 4));
          list_offer<KS, 32>(ld[qi], lj[qi], dm[jj], j, k, td, tj);
        }
        thr[qi] = td;
      }
      __builtin_amdgcn_sched_barrier(0);  // one row at a time: the rows' work interleaved costs a hundred registers
    }
  }

  const bool final_pass = a.slices == 1;
#pragma unroll
  for (int qi = 0; qi < 8; ++qi) {
    const int row = q0 + ty * 8 + qi;
    if (row >= a.nq) continue;
    int32_t *oi = slice == 0 ? a.idx : a.ws_idx + (size_t)(slice - 1) * a.nq * k;
    float *od = slice == 0 ? a.dist : a.ws_dist + (size_t)(slice - 1) * a.nq * k;
#pragma unroll
    for (int m = 0; m < KS; ++m) {
      const int s = tx + 32 * m;
      if (s < k) {
        const float d = ld[qi][m];
        oi[(size_t)row * k + s] = lj[qi][m];
        od[(size_t)row * k + s] = (final_pass && d < 0.f) ? 0.f : d;
      }
    }
    if (MEAN) {
      float v = msum[qi];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
      if (tx == 0) {
        if (final_pass) a.mean[row] = v / (float)(s_hi[ty * 8 + qi] - s_lo[ty * 8 + qi]);
        else if (slice == 0) a.mean[row] = v;
        else a.ws_mean[(size_t)(slice - 1) * a.nq + row] = v;
      }
    }
  }
}

// One wave per query row: the row's `slices` sorted lists are read into LDS, every entry counts the entries before it under
// (d2, j) -- equal keys, which only the unused slots of a short slice have, by slice -- and the first k go out in place.
__global__ __launch_bounds__(64 * kKnnMergeRows) void knn_merge_kernel(KnnArgs a, int with_mean) {
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_smem[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * kKnnMergeRows + w;
  const int k = a.k, L = a.slices * k;
  float *sd = reinterpret_cast<float *>(knn_smem) + (size_t)w * L;
  int *sj = reinterpret_cast<int *>(reinterpret_cast<float *>(knn_smem) + (size_t)kKnnMergeRows * L) + (size_t)w * L;
  const bool live = row < a.nq;
  if (live)
    for (int e = lane; e < L; e += 64) {
      const int s = e / k, p = e - s * k;
      const size_t at = s == 0 ? (size_t)row * k + p : ((size_t)(s - 1) * a.nq + row) * k + p;
      sd[e] = s == 0 ? a.dist[at] : a.ws_dist[at];
      sj[e] = s == 0 ? a.idx[at] : a.ws_idx[at];
    }
  __syncthreads();
  if (!live) return;
  for (int e = lane; e < L; e += 64) {
    const int s = e / k, p = e - s * k;
    const float d = sd[e];
    const int j = sj[e];
    const int rank = merged_rank(sd, sj, a.slices, k, s, p);
    if (rank < k) {
      a.idx[(size_t)row * k + rank] = j;
      a.dist[(size_t)row * k + rank] = d < 0.f ? 0.f : d;
    }
  }
  if (with_mean && lane == 0) {
    float v = a.mean[row];
    for (int s = 1; s < a.slices; ++s) v += a.ws_mean[(size_t)(s - 1) * a.nq + row];
    int lo, hi;
    row_range(a.seg, a.B, a.n, row, lo, hi);
    a.mean[row] = v / (float)(hi - lo);
  }
}

}  // namespace
}  // namespace hg

extern "C" {

size_t hg_knn_workspace_bytes(int32_t nq, int32_t n, int32_t F, int32_t k, int32_t cand_slices) {
  if (!hg::knn_sizes_ok(nq, n, F, k, cand_slices, 0)) return 0;
  const int slices = cand_slices ? cand_slices : hg::knn_auto_slices(nq, n);
  return hg::knn_layout(nq, n, k, slices).total;
}

int hg_knn_f32(const float *Q, int32_t nq, const float *X, int32_t n, int32_t F, int32_t k, const int32_t *seg, int32_t B,
               int32_t self_first, int32_t cand_slices, int32_t *idx, float *dist, float *mean_dist, void *workspace,
               size_t workspace_bytes, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_knn_f32";
  if (const int st = knn_refusal({entry, Q, X, idx, dist, nq, n, F, k, self_first, cand_slices}, 0, seg, B)) return st;
  for (const void *p : {(const void *)Q, (const void *)X, (const void *)idx, (const void *)dist, (const void *)mean_dist,
                        (const void *)workspace})
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, "Q, X, idx, dist, mean_dist and the workspace must be 4-byte aligned");
  const int slices = cand_slices ? cand_slices : knn_auto_slices(nq, n);
  const KnnLayout L = knn_layout(nq, n, k, slices);
  const bool need_ws = seg || slices > 1;
  if (need_ws && (!workspace || workspace_bytes < L.total))
    return fail(entry, HG_ERR_WORKSPACE, "workspace of " + std::to_string(workspace_bytes) + " bytes, hg_knn_workspace_bytes asks for " +
                                             std::to_string(L.total));

  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  KnnArgs a{};
  a.Q = Q;
  a.X = X;
  a.nq = nq;
  a.n = n;
  a.F = F;
  a.k = k;
  a.B = B;
  a.slices = slices;
  a.self_first = self_first ? 1 : 0;
  a.idx = idx;
  a.dist = dist;
  a.mean = mean_dist;
  if (seg) {
    // the offsets are the caller's host memory: the copy has left it when this returns
    hipError_t e = hipMemcpyAsync(ws + L.seg, seg, ((size_t)B + 1) * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(entry, HG_ERR_HIP, std::string("copy of seg: ") + hipGetErrorString(e));
    a.seg = reinterpret_cast<const int32_t *>(ws + L.seg);
  }
  if (slices > 1) {
    a.ws_idx = reinterpret_cast<int32_t *>(ws + L.idx);
    a.ws_dist = reinterpret_cast<float *>(ws + L.dist);
    a.ws_mean = reinterpret_cast<float *>(ws + L.mean);
  }
  const dim3 grid((unsigned)((nq + kKnnTQ - 1) / kKnnTQ), (unsigned)slices);
  const bool wide = k > 32, mean = mean_dist != nullptr;
  if (wide && mean) hipLaunchKernelGGL((knn_kernel<2, true>), grid, dim3(kKnnBlock), 0, s, a);
  else if (wide) hipLaunchKernelGGL((knn_kernel<2, false>), grid, dim3(kKnnBlock), 0, s, a);
  else if (mean) hipLaunchKernelGGL((knn_kernel<1, true>), grid, dim3(kKnnBlock), 0, s, a);
  else hipLaunchKernelGGL((knn_kernel<1, false>), grid, dim3(kKnnBlock), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && slices > 1) {
    const size_t lds = (size_t)kKnnMergeRows * slices * k * 8;  // at most 4 x 32 x 64 x 8 = 64 KiB
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((nq + kKnnMergeRows - 1) / kKnnMergeRows)), dim3(64 * kKnnMergeRows),
                       lds, s, a, mean ? 1 : 0);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return fail(entry, HG_ERR_HIP, std::string("launch: ") + hipGetErrorString(e));
  return HG_OK;
}

}  // extern "C"
