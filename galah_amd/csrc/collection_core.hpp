// The index arithmetic of the resident collection, stated
// once for the kernels (collection.hip), the host runtime (collection.cpp)
// and a stand-alone host test (tests/cpp/test_collection_core.cpp).
//
//   merge    old pairs have j < n_old, border pairs j >= n_old, both lists in
//            (i, j) order: inside a row i every old pair precedes every border
//            pair, so the merged position of a pair is closed-form from the
//            two lists' row boundaries -- no sort;
//   remove   new_index[] from the keep flags by an exclusive scan; a pair
//            survives iff both ends do, and the relabel is monotone, so the
//            compacted list stays in (i, j) order -- no sort;
//   batches  the in-place row compaction in stream-ordered batches of source
//            rows through a bounce buffer: rows only move down.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_COLLECTION_HD __host__ __device__
#else
#define GG_COLLECTION_HD
#endif

namespace gg {
namespace collection {

constexpr uint32_t kNone = 0xFFFFFFFFu;  // new_index of a removed row

// ---- row boundaries of an (i, j)-sorted list --------------------------------
// The first position p in [0, cnt) with pairs[p].i >= r (cnt when there is
// none): the boundary of row r.  P has a member i.
template <class P>
GG_COLLECTION_HD inline uint32_t row_boundary(const P* pairs, uint32_t cnt, uint32_t r) {
  uint32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pairs[mid].i < r)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// ---- the merge ---------------------------------------------------------------
// old_start / border_start: [n + 1] row boundaries of the two lists
// (row_boundary of r = 0 .. n; entry n is the list's length).
// Old pair p of row i: the old pairs before it and the border pairs of rows < i.
GG_COLLECTION_HD inline uint32_t merged_old(uint32_t p, uint32_t i, const uint32_t* border_start) {
  return p + border_start[i];
}
// Border pair q of row i: the border pairs before it and the old pairs of rows <= i.
GG_COLLECTION_HD inline uint32_t merged_border(uint32_t q, uint32_t i, const uint32_t* old_start) {
  return q + old_start[i + 1];
}

// ---- removal -------------------------------------------------------------------
// keep[r] != 0: row r stays.  below[r] = rows kept among 0 .. r-1 (below[n] =
// the rows kept), new_index[r] = below[r] for a kept row, kNone otherwise.
// Returns the first removed row (n: none).  Host side: it is the plan of the
// row batches too.
inline uint32_t relabel_rows(const uint8_t* keep, uint32_t n, uint32_t* below, uint32_t* new_index) {
  uint32_t kept = 0, first = n;
  for (uint32_t r = 0; r < n; ++r) {
    below[r] = kept;
    new_index[r] = keep[r] ? kept : kNone;
    if (keep[r])
      ++kept;
    else if (first == n)
      first = r;
  }
  below[n] = kept;
  return first;
}
GG_COLLECTION_HD inline bool pair_survives(const uint32_t* new_index, uint32_t i, uint32_t j) {
  return new_index[i] != kNone && new_index[j] != kNone;
}

// ---- the batches of the row compaction ------------------------------------------
// Rows before `first` (the first removed row) stay where they are.  Batch b
// covers the source rows [first + b * rows_per_batch, ... + rows_per_batch)
// clipped to n; its kept rows are gathered into the bounce buffer and then
// copied to the destination rows [below[src0], below[src1]).  below[r] <= r, so
// a batch's destinations end at or before its own last source row + 1 = the
// next batch's first source row: no batch writes a row that a later batch has
// yet to read, and inside a batch every source is in the bounce buffer before
// the first destination is written (the two steps are stream-ordered).
struct Batch {
  uint32_t src0, src1;  // source rows [src0, src1)
  uint32_t dst0, dst1;  // destination rows [dst0, dst1): the kept ones among them
};
GG_COLLECTION_HD inline uint32_t batch_count(uint32_t first, uint32_t n, uint32_t rows_per_batch) {
  return first >= n ? 0 : (n - first + rows_per_batch - 1) / rows_per_batch;
}
inline Batch batch_of(uint32_t b, uint32_t first, uint32_t n, uint32_t rows_per_batch, const uint32_t* below) {
  Batch x;
  x.src0 = first + b * rows_per_batch;
  x.src1 = n - x.src0 > rows_per_batch ? x.src0 + rows_per_batch : n;
  x.dst0 = below[x.src0];
  x.dst1 = below[x.src1];
  return x;
}
// Source rows per batch for a bounce buffer of at most bounce_bytes: at least
// one row (a row of the largest sketch is 96 KB).
GG_COLLECTION_HD inline uint32_t batch_rows(uint64_t bounce_bytes, uint32_t sketch_size) {
  const uint64_t row = (uint64_t)sketch_size * sizeof(uint64_t) + sizeof(uint32_t);
  const uint64_t rows = bounce_bytes / row;
  return rows < 1 ? 1 : rows > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)rows;
}

// ---- growth ------------------------------------------------------------------
// The capacity after a geometric growth that holds `need`.
GG_COLLECTION_HD inline uint64_t grown(uint64_t cap, uint64_t need) {
  const uint64_t twice = cap * 2;
  return twice > need ? twice : need;
}

}  // namespace collection
}  // namespace gg
