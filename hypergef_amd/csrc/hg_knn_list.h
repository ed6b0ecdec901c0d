// The two pieces the kNN kernels share (hg_knn.hip, hg_knn_dot.hip), each once: the sorted best-`len` list that W lanes of
// a wave keep in registers, and the rank of an entry in the merge of the slices' sorted lists.  Both order entries by the
// total order (d, j) -- the smaller distance first, the smaller index among equal distances -- and every result is
// compared bit for bit against the CPU reference.
//
// The list: slot s is in lane s % W of its W lanes (W = 32: a half wave, W = 64: the wave), in ld / lj[s / W]; unused
// slots hold (INFINITY, INT_MAX).  The block is one-dimensional, so a wave's lanes are threadIdx.x & 63.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace hg {

__device__ __forceinline__ bool key_less(float ad, int aj, float bd, int bj) { return ad < bd || (ad == bd && aj < bj); }

// slot s of the list, in every lane
template <int KS, int W, typename T>
__device__ __forceinline__ T list_slot(const T (&l)[KS], int s) {
  const unsigned u = (unsigned)s;
  T sel = l[0];
#pragma unroll
  for (int m = 1; m < KS; ++m) sel = u / W == (unsigned)m ? l[m] : sel;
  return __shfl(sel, (int)(u % W), W);
}

// Every lane offers (d, j) to its list of `len` entries; a NaN d is no offer.  (td, tj) is the list's last entry, slot
// len - 1, in every lane: the threshold, read by the caller before the first offer and kept up to date here.  An offer
// is one compare against it; the survivors go in smallest first, each with one shift by a lane -- slot s keeps its entry
// if that is smaller than the new one, else takes the larger of slot s - 1's and the new -- and the threshold is read
// again after every insert, so a survivor that no longer beats it drops out.
template <int KS, int W>
__device__ __forceinline__ void list_offer(float (&ld)[KS], int (&lj)[KS], float d, int j, int len, float &td, int &tj) {
  static_assert(W == 32 || W == 64, "a list is a half wave's or a wave's");
  const int lane = threadIdx.x & 63, tx = lane & (W - 1);
  bool pass = key_less(d, j, td, tj);
  unsigned long long wm = __ballot(pass);
  while (wm) {
    // the first of this list's offers; with W = 32 the wave's other list may be the only one that has any left
    bool act = true;
    int src;
    if constexpr (W == 32) {
      const unsigned hm = (unsigned)(wm >> (lane & 32));
      act = hm != 0;
      src = act ? __ffs(hm) - 1 : 0;
    } else {
      src = __ffsll((long long)wm) - 1;
    }
    const float nd = __shfl(d, src, W);
    const int nj = __shfl(j, src, W);
    float pd[KS];  // slot s - 1's entry: the lane before, and lane W - 1's slot of the row before for lane 0
    int pj[KS];
#pragma unroll
    for (int m = 0; m < KS; ++m) {
      pd[m] = __shfl_up(ld[m], 1, W);
      pj[m] = __shfl_up(lj[m], 1, W);
    }
#pragma unroll
    for (int m = KS - 1; m > 0; --m) {
      const float wd = __shfl(ld[m - 1], W - 1, W);
      const int wj = __shfl(lj[m - 1], W - 1, W);
      if (tx == 0) {
        pd[m] = wd;
        pj[m] = wj;
      }
    }
    if (tx == 0) {
      pd[0] = -INFINITY;
      pj[0] = -1;
    }
#pragma unroll
    for (int m = 0; m < KS; ++m) {
      const bool keep = !act || key_less(ld[m], lj[m], nd, nj);
      const bool take_new = key_less(pd[m], pj[m], nd, nj);
      ld[m] = keep ? ld[m] : (take_new ? nd : pd[m]);
      lj[m] = keep ? lj[m] : (take_new ? nj : pj[m]);
    }
    td = list_slot<KS, W>(ld, len - 1);
    tj = list_slot<KS, W>(lj, len - 1);
    pass = pass && !(act && tx == src) && key_less(d, j, td, tj);
    wm = __ballot(pass);
  }
}

// The place of entry p of slice s in the merge of `slices` sorted lists of `len` entries each, back to back in sd / sj
// (LDS): p, plus for every other slice the entries before this one, found by bisection.  Equal keys, which only the unused
// slots of a short slice have, go by slice.
__device__ __forceinline__ int merged_rank(const float *sd, const int *sj, int slices, int len, int s, int p) {
  const float d = sd[s * len + p];
  const int j = sj[s * len + p];
  int rank = p;
  for (int o = 0; o < slices; ++o) {
    if (o == s) continue;
    const float *od = sd + o * len;
    const int *oj = sj + o * len;
    int lo = 0, hi = len;  // entries [0, lo) are before this one, [hi, len) are not
    while (lo < hi) {
      const int m = (lo + hi) >> 1;
      const bool before = o < s ? !key_less(d, j, od[m], oj[m]) : key_less(od[m], oj[m], d, j);
      if (before) lo = m + 1;
      else hi = m;
    }
    rank += lo;
  }
  return rank;
}

}  // namespace hg
