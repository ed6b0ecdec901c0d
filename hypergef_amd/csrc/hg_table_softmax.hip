// Attention softmax over a dense neighbour table idx [rows, k] (include/hg_aggr.h, hg_table_softmax_f32 /
// hg_table_softmax_bwd_f32 / hg_table_sum_f32): the coefficients of a kNN hypergraph on the device, with no plan, no host
// list of long segments and no workspace.  One kernel template over (side, body), six instances.
//
// A segment is one group of table positions.  Side 0 ("hyperedge"): row i of the table, the positions i k .. i k + k - 1.
// Side 1 ("vertex"): pos_v[ptr_v[v] .. ptr_v[v + 1]) of hg_table_transpose, any length.  An entry of a segment is a
// candidate where it is in range (side 0: idx[p] in 0 .. n - 1; side 1: pos_v[q] in 0 .. rows k - 1).
//
// Lanes: a lane group of L lanes owns a segment, 64 / L segments a wave, kTableWaves waves a workgroup.  Side 0:
// L = the power of two at or above k, one entry per lane.  Side 1: L = max(kSoftMinL, that power of two) -- a function of k
// alone -- and lane l takes the entries q = l, l + L, l + 2 L .. of a segment of at most HG_TABLE_SEQ_MAX entries, at most
// kSoftKeep = HG_TABLE_SEQ_MAX / kSoftMinL of them, all kept in registers across the passes: every score is gathered once.
// A reduction is the lane's own ascending chain and then the xor butterfly t[l] = t[l] (+) t[l xor o], o = L / 2 .. 1, every
// lane at once: no LDS, no barrier.
//
// A side-1 segment of more entries is taken by the whole workgroup that owns it, in the same launch, after the short
// ones (the wave ballots of hg_table_gather_t_f32): thread t takes q = t, t + 256 .., gathers its logits again in every
// pass (no staging in LDS), and a reduction is the thread's chain, the wave's butterfly o = 32 .. 1, one LDS slot per wave
// and the join ((w0 (+) w1) (+) w2) (+) w3 by every thread: one barrier per reduction, the slots alternating between two
// buffers so that the barrier of reduction t + 1 is what frees the buffer of reduction t.
//
// Side 1 reaches only the positions some vertex owns, so its softmax and backward bodies sweep idx once more -- every
// workgroup a contiguous slice of the positions -- and write the +0.0 of the positions whose idx is out of range.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <string>

#include "hg_aggr.h"
#include "hg_attention.h"
#include "hg_internal.h"
#include "hg_table.h"

namespace hg {
namespace {

constexpr int kSoftBlock = 64 * kTableWaves;
constexpr int kSoftMinL = 8;                          // side 1: the narrowest lane group
constexpr int kSoftKeep = kTableSeqMax / kSoftMinL;   // side 1: entries a lane keeps in registers
static_assert(kSoftKeep * kSoftMinL == kTableSeqMax, "a short segment must fit its lane group's registers");

enum { kBodySoftmax = 0, kBodySoftmaxBwd = 1, kBodySum = 2 };

struct TableSoftmaxArgs {
  const int32_t *idx, *ptr_v, *pos_v;
  const float *node, *edge, *entry;  // the scores [n], [rows], [rows k]; each may be null
  const float *val, *dval;           // backward: alpha and dalpha; sum: the summed values; [rows k]
  float *out_entry;                  // softmax: alpha; backward: ds; [rows k]
  float *out_seg;                    // backward: the segments' own sums of ds, or null; sum: out; [segments]
  float slope;
  int32_t rows, k, n, entries, nseg;
  int32_t L, R;                      // lanes per segment, segments per wave
};

template <int SIDE>
__device__ __forceinline__ void seg_range(const TableSoftmaxArgs &a, int seg, int &beg, int &end) {
  if (SIDE) {
    beg = max(a.ptr_v[seg], 0);
    end = min(a.ptr_v[seg + 1], a.entries);
  } else {
    beg = seg * a.k;
    end = beg + a.k;
  }
}

// Entry q of a segment: its table position p and the other end j (side 0: the vertex idx[p]; side 1: the hyperedge p / k),
// both 0 where the entry is no candidate; returns whether it is one.  `on`: q is an entry at all.
template <int SIDE>
__device__ __forceinline__ bool seg_entry(const TableSoftmaxArgs &a, int q, bool on, int &p, int &j) {
  if (SIDE) {
    p = a.pos_v[on ? q : 0];
    on = on && (unsigned)p < (unsigned)a.entries;
    p = on ? p : 0;
    j = p / a.k;
  } else {
    p = on ? q : 0;
    j = a.idx[p];
    on = on && (unsigned)j < (unsigned)a.n;
    j = on ? j : 0;
  }
  return on;
}

// raw = (own + other) + entry, the segment's own score first; an absent score is no addition
template <int SIDE>
__device__ __forceinline__ float seg_raw(const TableSoftmaxArgs &a, float own, int p, int j) {
  const float *other = SIDE ? a.edge : a.node;
  bool have = (SIDE ? a.node : a.edge) != nullptr;
  float raw = have ? own : 0.f;
  if (other) {
    const float o = other[j];
    raw = have ? raw + o : o;
    have = true;
  }
  if (a.entry) {
    const float e = a.entry[p];
    raw = have ? raw + e : e;
  }
  return raw;
}

template <bool MAX>
__device__ __forceinline__ float join(float x, float y) {
  return MAX ? fmaxf(x, y) : x + y;
}

// the butterfly of one lane group: every lane of the wave takes part, and every lane of a group ends with the same bits
template <bool MAX>
__device__ __forceinline__ float group_join(float v, int L) {
  for (int o = L >> 1; o >= 1; o >>= 1) v = join<MAX>(v, __shfl_xor(v, o, 64));
  return v;
}

// the whole workgroup: the wave's butterfly, one slot per wave, the slots joined in ascending wave order by every thread
template <bool MAX>
__device__ __forceinline__ float block_join(float v, float (*slot)[kTableWaves], int &buf, int w, int lane) {
  v = group_join<MAX>(v, 64);
  if (lane == 0) slot[buf][w] = v;
  __syncthreads();
  float r = slot[buf][0];
#pragma unroll
  for (int o = 1; o < kTableWaves; ++o) r = join<MAX>(r, slot[buf][o]);
  buf ^= 1;
  return r;
}

// The segments a lane group owns whole: entries [beg, end) (none where the group is off), lane cl of L takes beg + cl + u L.
// Every lane of the wave runs this, for the shuffles; NS: the entries a lane can hold.
template <int SIDE, int BODY, int NS>
__device__ __forceinline__ void group_segment(const TableSoftmaxArgs &a, int seg, bool act, int beg, int end, int L, int cl) {
  const int len = end - beg;
  const float *own_score = SIDE ? a.node : a.edge;
  const float own = (BODY != kBodySum && own_score && act) ? own_score[seg] : 0.f;
  int pp[NS];  // the candidate's position, or -1
#pragma unroll
  for (int u = 0; u < NS; ++u) pp[u] = -1;

  if constexpr (BODY == kBodySoftmax) {
    float x[NS];
    float m = -INFINITY;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool on = cl + u * L < len;
      if (NS > 1 && !__any(on)) break;
      int p, j;
      const bool ok = seg_entry<SIDE>(a, beg + cl + u * L, on, p, j);
      x[u] = leaky(seg_raw<SIDE>(a, own, p, j), a.slope);
      pp[u] = ok ? p : -1;
      m = ok ? fmaxf(m, x[u]) : m;
    }
    m = group_join<true>(m, L);
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      if (NS > 1 && !__any(cl + u * L < len)) break;
      x[u] = __expf(x[u] - m);
      s = pp[u] >= 0 ? s + x[u] : s;
    }
    s = group_join<false>(s, L);
    const float inv = 1.f / s;  // the maximum's entry contributes exp(0) = 1: s >= 1 wherever inv is used
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool on = cl + u * L < len;
      if (NS > 1 && !__any(on)) break;
      if (SIDE) {
        if (pp[u] >= 0) a.out_entry[pp[u]] = x[u] * inv;
      } else if (on) {
        a.out_entry[beg + cl + u * L] = pp[u] >= 0 ? x[u] * inv : 0.f;
      }
    }
  } else if constexpr (BODY == kBodySoftmaxBwd) {
    float av[NS], dv[NS], gv[NS];
    float dot = 0.f;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool on = cl + u * L < len;
      if (NS > 1 && !__any(on)) break;
      int p, j;
      const bool ok = seg_entry<SIDE>(a, beg + cl + u * L, on, p, j);
      gv[u] = seg_raw<SIDE>(a, own, p, j) > 0.f ? 1.f : a.slope;
      av[u] = a.val[p];
      dv[u] = a.dval[p];
      pp[u] = ok ? p : -1;
      dot = ok ? dot + av[u] * dv[u] : dot;
    }
    dot = group_join<false>(dot, L);
    float dsum = 0.f;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool on = cl + u * L < len;
      if (NS > 1 && !__any(on)) break;
      const float ds = (av[u] * (dv[u] - dot)) * gv[u];
      dsum = pp[u] >= 0 ? dsum + ds : dsum;
      if (SIDE) {
        if (pp[u] >= 0) a.out_entry[pp[u]] = ds;
      } else if (on) {
        a.out_entry[beg + cl + u * L] = pp[u] >= 0 ? ds : 0.f;
      }
    }
    if (a.out_seg) {
      dsum = group_join<false>(dsum, L);
      if (act && cl == 0) a.out_seg[seg] = dsum;
    }
  } else {
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const bool on = cl + u * L < len;
      if (NS > 1 && !__any(on)) break;
      int p, j;
      const bool ok = seg_entry<SIDE>(a, beg + cl + u * L, on, p, j);
      const float v = a.val[p];
      s = ok ? s + v : s;
    }
    s = group_join<false>(s, L);
    if (act && cl == 0) a.out_seg[seg] = s;
  }
}

// One side-1 segment of more than HG_TABLE_SEQ_MAX entries, by the whole workgroup: thread t takes beg + t, beg + t + 256 ..
template <int BODY>
__device__ __forceinline__ void block_segment(const TableSoftmaxArgs &a, int seg, int beg, int end, int t, float (*slot)[kTableWaves],
                                              int &buf) {
  const int w = t >> 6, lane = t & 63;
  const unsigned len = (unsigned)(end - beg);
  const float own = (BODY != kBodySum && a.node) ? a.node[seg] : 0.f;
  int p, j;
  if constexpr (BODY == kBodySoftmax) {
    float m = -INFINITY;
    for (unsigned o = t; o < len; o += kSoftBlock) {
      const bool ok = seg_entry<1>(a, beg + (int)o, true, p, j);
      const float x = leaky(seg_raw<1>(a, own, p, j), a.slope);
      m = ok ? fmaxf(m, x) : m;
    }
    m = block_join<true>(m, slot, buf, w, lane);
    float s = 0.f;
    for (unsigned o = t; o < len; o += kSoftBlock) {
      const bool ok = seg_entry<1>(a, beg + (int)o, true, p, j);
      const float e = __expf(leaky(seg_raw<1>(a, own, p, j), a.slope) - m);
      s = ok ? s + e : s;
    }
    s = block_join<false>(s, slot, buf, w, lane);
    const float inv = 1.f / s;
    for (unsigned o = t; o < len; o += kSoftBlock) {
      const bool ok = seg_entry<1>(a, beg + (int)o, true, p, j);
      const float e = __expf(leaky(seg_raw<1>(a, own, p, j), a.slope) - m);
      if (ok) a.out_entry[p] = e * inv;
    }
  } else if constexpr (BODY == kBodySoftmaxBwd) {
    float dot = 0.f;
    for (unsigned o = t; o < len; o += kSoftBlock) {
      const bool ok = seg_entry<1>(a, beg + (int)o, true, p, j);
      const float term = a.val[p] * a.dval[p];
      dot = ok ? dot + term : dot;
    }
    dot = block_join<false>(dot, slot, buf, w, lane);
    float dsum = 0.f;
    for (unsigned o = t; o < len; o += kSoftBlock) {
      const bool ok = seg_entry<1>(a, beg + (int)o, true, p, j);
      const float g = seg_raw<1>(a, own, p, j) > 0.f ? 1.f : a.slope;
      const float ds = (a.val[p] * (a.dval[p] - dot)) * g;
      dsum = ok ? dsum + ds : dsum;
      if (ok) a.out_entry[p] = ds;
    }
    if (a.out_seg) {
      dsum = block_join<false>(dsum, slot, buf, w, lane);
      if (t == 0) a.out_seg[seg] = dsum;
    }
  } else {
    float s = 0.f;
    for (unsigned o = t; o < len; o += kSoftBlock) {
      const bool ok = seg_entry<1>(a, beg + (int)o, true, p, j);
      const float v = a.val[p];
      s = ok ? s + v : s;
    }
    s = block_join<false>(s, slot, buf, w, lane);
    if (t == 0) a.out_seg[seg] = s;
  }
}

template <int SIDE, int BODY>
__global__ __launch_bounds__(kSoftBlock) void table_softmax_kernel(TableSoftmaxArgs a) {
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int L = a.L, R = a.R;
  const int sub = lane / L, cl = lane - sub * L;
  const int RW = R * kTableWaves;

  if constexpr (SIDE == 1 && BODY != kBodySum) {
    // the positions no vertex owns: this workgroup's slice of the table
    const int64_t chunk = ((int64_t)a.entries + gridDim.x - 1) / gridDim.x;
    const int64_t pb = (int64_t)blockIdx.x * chunk, pe = min(pb + chunk, (int64_t)a.entries);
    for (int64_t p = pb + t; p < pe; p += kSoftBlock)
      if ((unsigned)a.idx[p] >= (unsigned)a.n) a.out_entry[p] = 0.f;
  }

  const int64_t seg0 = (int64_t)blockIdx.x * RW;
  const int64_t seg64 = seg0 + w * R + sub;
  const bool seg_on = seg64 < a.nseg;
  const int seg = seg_on ? (int)seg64 : 0;
  int beg = 0, end = 0;
  if (seg_on) seg_range<SIDE>(a, seg, beg, end);
  const bool is_long = SIDE == 1 && end - beg > kTableSeqMax;
  const bool act = seg_on && !is_long;
  group_segment<SIDE, BODY, SIDE ? kSoftKeep : 1>(a, seg, act, beg, act ? end : beg, L, cl);

  if constexpr (SIDE == 1) {
    __shared__ float slot[2][kTableWaves];
    __shared__ unsigned long long long_rows[kTableWaves];
    const unsigned long long mine = __ballot(seg_on && is_long && cl == 0);
    if (lane == 0) long_rows[w] = mine;
    __syncthreads();
    int buf = 0;
    for (int ww = 0; ww < kTableWaves; ++ww) {
      const unsigned long long mm = long_rows[ww];
      unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)mm), hi = __builtin_amdgcn_readfirstlane((unsigned)(mm >> 32));
      unsigned long long m = ((unsigned long long)hi << 32) | lo;
      while (m) {
        const int ln = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int lseg = (int)(seg0 + ww * R + ln / L);
        int lbeg, lend;
        seg_range<1>(a, lseg, lbeg, lend);
        block_segment<BODY>(a, lseg, lbeg, lend, t, slot, buf);
      }
    }
  }
}

int pow2_at_least(int k) {
  int L = 1;
  while (L < k) L <<= 1;
  return L;
}

template <int BODY>
int launch_table_softmax(const char *entry, int side, TableSoftmaxArgs a, hg_stream_t stream) {
  a.entries = a.rows * a.k;
  a.nseg = side ? a.n : a.rows;
  a.L = side ? std::max(kSoftMinL, pow2_at_least(a.k)) : pow2_at_least(a.k);
  a.R = 64 / a.L;
  const int RW = a.R * kTableWaves;
  const dim3 grid((unsigned)(((int64_t)a.nseg + RW - 1) / RW)), block(kSoftBlock);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (side) hipLaunchKernelGGL((table_softmax_kernel<1, BODY>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((table_softmax_kernel<0, BODY>), grid, block, 0, s, a);
  return launch_check(entry);
}

// what the three entries refuse, in the table entries' order: null pointers, the sizes, the side, the alignment
int softmax_refusal(const char *entry, const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t side, const char *side_name,
                    const int32_t *ptr_v, const int32_t *pos_v, bool arrays_given, const char *null_text,
                    std::initializer_list<const void *> arrays) {
  if (!idx) return fail(entry, HG_ERR_INVALID, "null idx");
  if (!arrays_given) return fail(entry, HG_ERR_INVALID, null_text);
  if (side == HG_TABLE_VERTEX && (!ptr_v || !pos_v))
    return fail(entry, HG_ERR_INVALID, std::string("null ptr_v or pos_v (") + side_name + " = HG_TABLE_VERTEX walks the transpose)");
  if (const int st = size_refusal(entry, rows, k, n, 1)) return st;
  if (side != HG_TABLE_HYPEREDGE && side != HG_TABLE_VERTEX)
    return fail(entry, HG_ERR_INVALID,
                std::string(side_name) + " must be HG_TABLE_HYPEREDGE or HG_TABLE_VERTEX, got " + std::to_string(side));
  for (const void *p : {(const void *)idx, (const void *)ptr_v, (const void *)pos_v})
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, "the table, its transpose and every array must be 4-byte aligned");
  for (const void *p : arrays)
    if ((uintptr_t)p % 4) return fail(entry, HG_ERR_UNSUPPORTED, "the table, its transpose and every array must be 4-byte aligned");
  return HG_OK;
}

TableSoftmaxArgs softmax_args(const int32_t *idx, int32_t rows, int32_t k, int32_t n, const float *node, const float *edge,
                              const float *entry_score, float slope, const int32_t *ptr_v, const int32_t *pos_v) {
  TableSoftmaxArgs a{};
  a.idx = idx;
  a.ptr_v = ptr_v;
  a.pos_v = pos_v;
  a.node = node;
  a.edge = edge;
  a.entry = entry_score;
  a.slope = slope;
  a.rows = rows;
  a.k = k;
  a.n = n;
  return a;
}

}  // namespace
}  // namespace hg

extern "C" {

int hg_table_softmax_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t group, const float *node_score,
                         const float *edge_score, const float *entry_score, float slope, const int32_t *ptr_v,
                         const int32_t *pos_v, float *alpha, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_softmax_f32";
  if (const int st = softmax_refusal(entry, idx, rows, k, n, group, "group", ptr_v, pos_v,
                                     alpha && (node_score || edge_score || entry_score),
                                     "null alpha, or node_score, edge_score and entry_score all null",
                                     {node_score, edge_score, entry_score, alpha}))
    return st;
  TableSoftmaxArgs a = softmax_args(idx, rows, k, n, node_score, edge_score, entry_score, slope, ptr_v, pos_v);
  a.out_entry = alpha;
  return launch_table_softmax<kBodySoftmax>(entry, group, a, stream);
}

int hg_table_softmax_bwd_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t group, const float *node_score,
                             const float *edge_score, const float *entry_score, float slope, const int32_t *ptr_v,
                             const int32_t *pos_v, const float *alpha, const float *dalpha, float *ds, float *dgroup,
                             hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_softmax_bwd_f32";
  if (const int st = softmax_refusal(entry, idx, rows, k, n, group, "group", ptr_v, pos_v,
                                     alpha && dalpha && ds && (node_score || edge_score || entry_score),
                                     "null alpha, dalpha or ds, or node_score, edge_score and entry_score all null",
                                     {node_score, edge_score, entry_score, alpha, dalpha, ds, dgroup}))
    return st;
  TableSoftmaxArgs a = softmax_args(idx, rows, k, n, node_score, edge_score, entry_score, slope, ptr_v, pos_v);
  a.val = alpha;
  a.dval = dalpha;
  a.out_entry = ds;
  a.out_seg = dgroup;
  return launch_table_softmax<kBodySoftmaxBwd>(entry, group, a, stream);
}

int hg_table_sum_f32(const int32_t *idx, int32_t rows, int32_t k, int32_t n, int32_t side, const int32_t *ptr_v,
                     const int32_t *pos_v, const float *val, float *out, hg_stream_t stream) {
  using namespace hg;
  const char *entry = "hg_table_sum_f32";
  if (const int st = softmax_refusal(entry, idx, rows, k, n, side, "side", ptr_v, pos_v, val && out, "null val or out", {val, out}))
    return st;
  TableSoftmaxArgs a = softmax_args(idx, rows, k, n, nullptr, nullptr, nullptr, 1.f, ptr_v, pos_v);
  a.val = val;
  a.out_seg = out;
  return launch_table_softmax<kBodySum>(entry, side, a, stream);
}

}  // extern "C"
