// Aggregation over a dense neighbour table idx [rows, k] (hg_table.hip): the transpose and the two row gathers of a
// hypergraph whose every hyperedge has exactly k members -- what hg_knn_f32 writes.  No schedule, no host step: the
// entries hg_table_transpose / hg_table_gather_f32 / hg_table_gather_t_f32 launch on the caller's stream and nothing else.
//
// Transpose: a least-significant-digit radix sort of the positions p = 0 .. rows k - 1 by the key idx[p] (an entry outside
// 0 .. n - 1 has the key n and so lands behind every vertex), kTableRadixBits bits a pass.  Only the positions move: a
// pass reads the key of a position from idx.  A workgroup of kTableBlock threads ranks a tile of kTableTile positions
// with wave ballots, so every pass is stable and the result is the stable sort, a function of idx alone.
//
// Gathers: a lane group of L = min(ceil(F / V), 64) lanes owns a destination row (V = 4 columns a lane where F % 4 == 0
// and the rows are 16-byte aligned, else 1), 64 / L rows a wave, kTableWaves waves a workgroup.  A row of at most
// HG_TABLE_SEQ_MAX entries is summed by its lane group in ascending order, kTableBatch gathers in flight; a longer row of
// the transposed gather is summed by the whole workgroup that owns it: lane group g of the P = kTableWaves (64 / L) takes
// the entries [g c, (g + 1) c), c = ceil(len / P), in ascending order, and the P partial rows are added through LDS in
// the fixed tree part[g] += part[g + s], s = P' / 2, P' / 4 .. 1 (P' the power of two at or above P).
// The difference gathers (hg_table_gather_diff_f32 / hg_table_gather_t_diff_f32) are the same kernel under a template flag:
// the term starts from ctr[destination row] - src[j], the centre's column chunk loaded once per (row, column chunk).
//
// Distances (hg_table_dist_f32): one lane per table position walks the query row and the gathered row, kTableDistLoads
// loads of each in flight, one fma chain in ascending c -- hg_knn_f32's d2, bit for bit.
//
// Dot products (hg_table_dot_f32): a lane group of L lanes (the power of two at or above min(ceil(F / V), 64)) owns a table
// row, keeps its B / D chunk in registers over the row's k entries, gathers kTableDotBatch rows of A / C at a time, and
// adds the lanes' fma chains in an xor butterfly L / 2 .. 1.
#pragma once
#include <cstddef>
#include <cstdint>

#include "hg_aggr.h"

namespace hg {

constexpr int kTableSeqMax = HG_TABLE_SEQ_MAX;  // rows up to this long: one lane group, ascending
constexpr int kTableMaxK = 64;
constexpr int kTableWaves = 4;                  // gather: waves per workgroup
constexpr int kTableBatch = 8;                  // gather: row loads issued before the first add
constexpr int kTableDistLoads = 4;              // dist: loads of each of the two rows a lane issues before the first fma
constexpr int kTableDotBatch = 4;               // dot: gathered rows in flight per lane group
constexpr int kTableBlock = 256;                // transpose and dist: threads per workgroup
constexpr int kTableItems = 8;                  // transpose: positions per thread and pass
constexpr int kTableTile = kTableBlock * kTableItems;
constexpr int kTableRadixBits = 8;
constexpr int kTableBins = 1 << kTableRadixBits;
constexpr int kTableScanBlock = 1024;           // the one workgroup that scans the tile histograms

static_assert(kTableSeqMax >= kTableMaxK, "hop 0 (k entries a row) must always be sequential");

// The caller's workspace: [the second position buffer, rows k int32][the tile histograms, kTableBins x tiles int32]
struct TableLayout {
  size_t alt, hist, total;
  int64_t entries, tiles;
  int passes;  // radix passes: the keys 0 .. n have ceil(log2(n + 1)) bits
};
TableLayout table_layout(int64_t rows, int k, int64_t n);

}  // namespace hg
