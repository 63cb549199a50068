// The rules of the dense ANI matrix, stated once for the
// kernels (ani_matrix.hip), the host reference (gg_ani_matrix_host) and a
// stand-alone host test (tests/cpp/test_matrix_core.cpp).
//
// m positions name rows of a sketch matrix (any order, a row may be listed
// more than once).  For positions a, b the cell holds finch's merge counts of
// the two rows (src/finch.rs:57, validate_core.hpp) and gg_ani_f32 of them.
//
//   The column rule.  A *column* is a distinct hash held at two or more of
//     the listed positions; a hash held at one position only adds nothing to
//     any off-diagonal common and is dropped.  Column ids ascend with the
//     hash, so a row's kept ids (its *piece*) ascend as the row does.
//   The diagonal rule.  The same position, or the same row index listed
//     twice: (len, len).  An empty row on either side: (0, 0).
//   Off the diagonal.  common(a, b) = the number of columns both positions
//     hold = (A A^T)[a][b] for the 0/1 incidence matrix A [positions x
//     columns]; total by validate::total_from_rank / rank_le: with T the row
//     whose last element is the smaller,
//       total = |T| + #{s in S : s <= last T} - common.
//   The tiled product.  The positions in tiles of kTile, one workgroup per
//     tile pair (ti <= tj); the columns in chunks of kChunk, a chunk being a
//     [kTile x kChunk] byte image per row tile (row stride kRowBytes), read
//     as 16-byte fragments of the i8 16x16x64 matrix instruction.  A chunk in
//     which either tile holds no entry is skipped: the next chunk begins at
//     the larger of the two tiles' smallest remaining column ids.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "validate_core.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_MATRIX_HD __host__ __device__
#else
#define GG_MATRIX_HD
#endif

namespace gg {
namespace matrix {

constexpr uint32_t kMaxRows = 32768;          // m of one call
constexpr uint32_t kTile = 64;                // positions of a tile
constexpr uint32_t kChunk = 512;              // columns of a K chunk
constexpr uint32_t kRowBytes = kChunk + 16;   // a tile row in LDS: 132 dwords, 16 rows fall on 16 x 4 different banks
constexpr uint32_t kTileBytes = kTile * kRowBytes;
constexpr uint32_t kKSteps = kChunk / 64;     // matrix instructions per chunk and 16 x 16 block
constexpr uint32_t kNoColumn = 0xFFFFFFFFu;   // an entry in no column; no further column

// ---- the column rule over the sorted keys K[0 .. ne) ------------------------
// entry i lies in a column: a neighbour holds the same hash
GG_MATRIX_HD inline bool in_column(const uint64_t* K, uint64_t i, uint64_t ne) {
  return (i > 0 && K[i] == K[i - 1]) || (i + 1 < ne && K[i + 1] == K[i]);
}
// entry i is the first of a run of two or more: it opens a column
GG_MATRIX_HD inline bool column_head(const uint64_t* K, uint64_t i, uint64_t ne) {
  return (i == 0 || K[i] != K[i - 1]) && i + 1 < ne && K[i + 1] == K[i];
}
// the two flags packed for one inclusive sum: low word columns opened up to
// and including i, high word entries in columns
GG_MATRIX_HD inline uint64_t column_flags(const uint64_t* K, uint64_t i, uint64_t ne) {
  return (uint64_t)column_head(K, i, ne) | ((uint64_t)in_column(K, i, ne) << 32);
}
// the column id of entry i from the inclusive sum at i
GG_MATRIX_HD inline uint32_t column_id(uint64_t inclusive_sum) { return (uint32_t)inclusive_sum - 1u; }

// ---- tiles --------------------------------------------------------------------
GG_MATRIX_HD inline uint32_t tiles_of(uint32_t m) { return (m + kTile - 1) / kTile; }
GG_MATRIX_HD inline uint32_t tile_pairs_of(uint32_t tiles) { return tiles * (tiles + 1) / 2; }  // <= 131,328
// workgroup p -> (ti <= tj), p = tj (tj + 1) / 2 + ti
GG_MATRIX_HD inline void tile_pair_of(uint32_t p, uint32_t* ti, uint32_t* tj) {
  uint32_t j = (uint32_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
  while (j * (j + 1) / 2 > p) --j;
  while ((j + 1) * (j + 2) / 2 <= p) ++j;
  *tj = j;
  *ti = p - j * (j + 1) / 2;
}

// ---- a row's piece against the chunks -----------------------------------------
// the cursor of a piece at the chunk that begins at column k0: the first index
// >= lo whose id is >= k0 (lo: the cursor at an earlier chunk)
template <typename Ptr>
GG_MATRIX_HD inline uint32_t cursor_at(Ptr piece, uint32_t lo, uint32_t cnt, uint32_t k0) {
  uint32_t hi = cnt;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (piece[mid] < k0) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the chunk to run next from the smallest remaining ids of the two tiles
// (kNoColumn: a tile has none left, the product is complete)
GG_MATRIX_HD inline uint32_t next_chunk(uint32_t min_a, uint32_t min_b) {
  if (min_a == kNoColumn || min_b == kNoColumn) return kNoColumn;
  return (min_a > min_b ? min_a : min_b) / kChunk * kChunk;
}
// byte of (row r of the tile, column c of the chunk) in the tile's image
GG_MATRIX_HD inline uint32_t image_offset(uint32_t r, uint32_t c) { return r * kRowBytes + c; }
// the 16-byte fragment lane `lane` feeds to k-step ks for the 16-row block
// `block` of a tile; the A lane and the B lane of the same (lane >> 4) read
// the same 16 columns, which is all the sum over k needs
GG_MATRIX_HD inline uint32_t fragment_offset(uint32_t lane, uint32_t ks, uint32_t block) {
  return image_offset(block * 16 + (lane & 15), ks * 64 + (lane >> 4) * 16);
}
// C/D of the 16x16 instruction: register reg of lane `lane` is (row, col);
// rows come from the A operand's lanes, columns from the B operand's
GG_MATRIX_HD inline uint32_t cd_row(uint32_t lane, uint32_t reg) { return (lane >> 4) * 4 + reg; }
GG_MATRIX_HD inline uint32_t cd_col(uint32_t lane) { return lane & 15; }

// ---- a cell ---------------------------------------------------------------------
// same: the same position or the same row index.  A / B the two rows, la / lb
// their lengths, last_a / last_b their last elements (read when la, lb != 0),
// common_ab the product's count.
template <typename Ptr>
GG_MATRIX_HD inline void cell_counts(bool same, Ptr A, uint32_t la, uint64_t last_a, Ptr B, uint32_t lb, uint64_t last_b,
                                     uint32_t common_ab, uint32_t* common, uint32_t* total) {
  if (la == 0 || lb == 0) {
    *common = *total = 0;
  } else if (same) {
    *common = *total = la;
  } else {
    const bool a_ends = last_a <= last_b;  // A is exhausted first (or both together)
    const uint32_t lt = a_ends ? la : lb, ls = a_ends ? lb : la;
    const uint32_t rank = validate::rank_le(a_ends ? B : A, ls, validate::hibit_of(ls), a_ends ? last_a : last_b);
    *common = common_ab;
    *total = validate::total_from_rank(lt, rank, common_ab);
  }
}

// ---- the columns on the host ------------------------------------------------------
// What the device builds with a radix sort and a scan: piece[a] the ascending
// column ids of position a.  rows == nullptr: position a is row a.
struct Columns {
  uint64_t n_entries = 0, n_columns = 0, column_entries = 0;
  std::vector<std::vector<uint32_t>> piece;
};
inline Columns columns_host(const uint64_t* sketches, const uint32_t* lens, uint32_t sketch_size, const uint32_t* rows,
                            uint32_t m) {
  struct Key {
    uint64_t hash;
    uint64_t slot;
  };
  std::vector<Key> keys;
  for (uint32_t a = 0; a < m; ++a) {
    const uint32_t g = rows ? rows[a] : a;
    for (uint32_t e = 0; e < lens[g]; ++e)
      keys.push_back(Key{sketches[(size_t)g * sketch_size + e], (uint64_t)a * sketch_size + e});
  }
  std::stable_sort(keys.begin(), keys.end(), [](const Key& x, const Key& y) { return x.hash < y.hash; });
  std::vector<uint64_t> K(keys.size());
  for (size_t i = 0; i < keys.size(); ++i) K[i] = keys[i].hash;
  Columns c;
  c.n_entries = K.size();
  std::vector<uint32_t> id_of((size_t)m * sketch_size, kNoColumn);
  uint64_t sum = 0;
  for (uint64_t i = 0; i < K.size(); ++i) {
    sum += column_flags(K.data(), i, K.size());
    if (in_column(K.data(), i, K.size())) id_of[keys[i].slot] = column_id(sum);
  }
  c.n_columns = (uint32_t)sum;
  c.column_entries = sum >> 32;
  c.piece.resize(m);
  for (uint32_t a = 0; a < m; ++a) {
    const uint32_t g = rows ? rows[a] : a;
    for (uint32_t e = 0; e < lens[g]; ++e)
      if (id_of[(size_t)a * sketch_size + e] != kNoColumn) c.piece[a].push_back(id_of[(size_t)a * sketch_size + e]);
  }
  return c;
}

}  // namespace matrix
}  // namespace gg
