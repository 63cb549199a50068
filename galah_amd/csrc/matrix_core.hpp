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
GG_MATRIX_HD inline uint32_t tile_pairs_of(uint32_t tiles) { return tiles * (tiles + 1) / 2; }  // (tiles < 2^16)
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

// ---- the pair form -------------------------------------------------
// The same product with a thresholded epilogue: instead of an [m x m] matrix,
// the list of pairs that pass gg_pairs' test (the rule of the gate kernel's
// epilogue, pairs_gate.hip).  cmin[t] is the smallest common that passes at
// total t (tmax = 2 s), sufmin[t] = min(cmin[t .. tmax]), zero_passes whether
// some cmin[t] is 0, all three as ensure_cmin builds them.
//   Cells visited.  Positions pa < pb only, in a diagonal tile as well; two
//     positions that name the same row emit nothing (positions whose index is
//     out of range all name the one row kNoRow, which is empty).
//   An empty row on either side passes iff cmin[0] == 0, as (i, j, 0, 0).
//   The candidate test, before any memory is touched: common >=
//     sufmin[min(la, lb)].  finch's merge ends when the row that ends first
//     is exhausted, so total >= that row's length >= min(la, lb) (not
//     max(la, lb): {1, 2} against 100 larger hashes gives total 2), and
//     sufmin[min(la, lb)] <= cmin[total]: no passing pair fails it.  Only a
//     candidate pays the rank search of cell_counts.
//   The pass test.  total <= tmax and common >= cmin[total].
//   The early exit.  A tile pair that ran no chunk holds only zero counts;
//     without zero_passes every cmin[t] >= 1, so nothing of it can pass.
//   What is emitted.  (min(row_a, row_b), max(row_a, row_b), common, total):
//     row indices of the sketch matrix, not positions.
//   Limits.  m s < 2^31 sketch slots, fewer than 2^31 tile pairs; kMaxRows
//     does not apply (there is no cell index).
//   Launches.  One launch takes fewer than 2^32 threads, so fewer than 2^24
//     workgroups of 256: the tile pairs go in slices of kPairSlice, workgroup
//     w of the slice that begins at `base` taking tile pair base + w.
constexpr uint32_t kPairSlice = 1u << 23;      // tile pairs of one launch (2^31 threads)
constexpr uint32_t kPairStage = 4096;          // pairs a workgroup stages in the image area (kTile^2, 16 B each)
static_assert(kPairStage == kTile * kTile && kPairStage * 16 <= 2 * kTileBytes, "the image area holds a tile pair's pairs");

inline bool pair_limits_ok(uint64_t m, uint64_t sketch_size) {
  const uint64_t tiles = (m + kTile - 1) / kTile;
  return m * sketch_size < (1ull << 31) && m < (1ull << 31) && tiles * (tiles + 1) / 2 < (1ull << 31);
}
GG_MATRIX_HD inline bool pair_visited(uint32_t pa, uint32_t pb, uint32_t row_a, uint32_t row_b) {
  return pa < pb && row_a != row_b;
}
GG_MATRIX_HD inline bool pair_early_exit(bool ran_a_chunk, bool zero_passes) { return !ran_a_chunk && !zero_passes; }
template <typename Tab>
GG_MATRIX_HD inline bool pair_candidate(uint32_t la, uint32_t lb, uint32_t common_ab, Tab cmin, Tab sufmin) {
  if (la == 0 || lb == 0) return cmin[0] == 0;
  return common_ab >= sufmin[la < lb ? la : lb];
}
template <typename Tab>
GG_MATRIX_HD inline bool pair_passes(uint32_t common, uint32_t total, Tab cmin, uint32_t tmax) {
  return total <= tmax && common >= cmin[total];
}
// One visited cell (pair_visited holds): whether it passes, and its counts.
// A / B, la / lb, last_a / last_b and common_ab as cell_counts takes them.
template <typename Ptr, typename Tab>
GG_MATRIX_HD inline bool pair_cell(Ptr A, uint32_t la, uint64_t last_a, Ptr B, uint32_t lb, uint64_t last_b,
                                   uint32_t common_ab, Tab cmin, Tab sufmin, uint32_t tmax, uint32_t* common,
                                   uint32_t* total) {
  *common = *total = 0;
  if (!pair_candidate(la, lb, common_ab, cmin, sufmin)) return false;
  if (la == 0 || lb == 0) return true;  // finch: common 0, total 0
  cell_counts(false, A, la, last_a, B, lb, last_b, common_ab, common, total);
  return pair_passes(*common, *total, cmin, tmax);
}
// The upper bound of the product's work and the lower bound of the inverted
// index's member reads (sum of g^2 over the columns >= column_entries^2 /
// n_columns, Cauchy-Schwarz), from the counts the call reads back anyway.
inline uint64_t pair_chunk_rounds(uint64_t m, uint64_t n_columns) {
  const uint64_t tiles = (m + kTile - 1) / kTile;
  return tiles * (tiles + 1) / 2 * ((n_columns + kChunk - 1) / kChunk);
}
inline uint64_t pair_index_reads(uint64_t n_columns, uint64_t column_entries) {
  return n_columns ? column_entries * column_entries / n_columns : 0;  // (column_entries < 2^31)
}

// ---- the border form -----------------------------------------------
// The pair form over rows 0 .. n-1 of which the last n_new = n - n_old are new:
// only the pairs that involve a new row (gg_pairs_border's set), so that the
// product can leave out most of its tile pairs and most of its columns.
//   Positions.  Position a names row n_old + a for a < n_new and row a - n_new
//     otherwise: the new rows come first, the sketch matrix is not moved (the
//     positions part is given this map as its row list).
//   Cells visited.  pair_visited and pa < n_new: every new x new pair once,
//     every new x old pair once; in the tile row that holds new and old
//     positions (n_new % kTile != 0) the cells with pa >= n_new are skipped.
//     The emitted record is the pair form's, (old, new) for a new x old cell.
//   Tile pairs.  ti < Tn = tiles_of(n_new) and ti <= tj < T = tiles_of(n):
//     the first Tn (Tn + 1) / 2 workgroups are the pair form's triangle over
//     the new tiles (tile_pair_of); workgroup p' behind them is tj = Tn +
//     p' / Tn, ti = p' % Tn, a rectangle of Tn x (T - Tn).  Slices of
//     kPairSlice and wg_base as in the pair form.
//   The border column rule.  A column is a distinct hash held at two or more
//     positions, at least one of them new: a hash shared among old rows only
//     adds nothing to a visited cell and is dropped (an old row unrelated to
//     every new row has an empty piece, its tile pairs take the early exit).
//     After the stable sort of (hash, slot), slots in position order, the
//     first entry of a run of equal hashes is the run's lowest position: a run
//     is kept iff it has two entries or more and that position is < n_new.
//   Unchanged.  The candidate test, the pass test, the empty-row rule,
//     zero_passes and the early exit; total comes from the rank search on the
//     full rows, so a dropped column changes no total.
//   Limits.  n_old <= n, n s < 2^31 sketch slots, fewer than 2^31 border tile
//     pairs.  n_old == n: nothing; n_old == 0: the pair form over all rows.
GG_MATRIX_HD inline uint32_t border_row_of(uint32_t a, uint32_t n, uint32_t n_old) {
  const uint32_t n_new = n - n_old;
  return a < n_new ? n_old + a : a - n_new;
}
GG_MATRIX_HD inline bool border_visited(uint32_t pa, uint32_t pb, uint32_t n_new, uint32_t row_a, uint32_t row_b) {
  return pa < n_new && pair_visited(pa, pb, row_a, row_b);
}
// a run of equal hashes whose first entry lies at position head_pos is a border column (given two entries or more)
GG_MATRIX_HD inline bool border_column_kept(uint32_t head_pos, uint32_t n_new) { return head_pos < n_new; }
// (tiles_new <= tiles; the result < 2^31: border_limits_ok)
GG_MATRIX_HD inline uint32_t border_tile_pairs(uint32_t tiles_new, uint32_t tiles) {
  return tile_pairs_of(tiles_new) + tiles_new * (tiles - tiles_new);
}
// workgroup p -> (ti < tiles_new, ti <= tj)
GG_MATRIX_HD inline void border_tile_pair_of(uint32_t p, uint32_t tiles_new, uint32_t* ti, uint32_t* tj) {
  const uint32_t tri = tile_pairs_of(tiles_new);
  if (p < tri) {
    tile_pair_of(p, ti, tj);
  } else {
    const uint32_t q = p - tri;
    *tj = tiles_new + q / tiles_new;
    *ti = q % tiles_new;
  }
}
// its inverse
GG_MATRIX_HD inline uint32_t border_tile_pair_index(uint32_t ti, uint32_t tj, uint32_t tiles_new) {
  return tj < tiles_new ? tj * (tj + 1) / 2 + ti : tile_pairs_of(tiles_new) + (tj - tiles_new) * tiles_new + ti;
}
inline bool border_limits_ok(uint64_t n, uint64_t n_old, uint64_t sketch_size) {
  if (n_old > n || n * sketch_size >= (1ull << 31) || n >= (1ull << 31)) return false;
  const uint64_t tiles = (n + kTile - 1) / kTile, tiles_new = (n - n_old + kTile - 1) / kTile;  // (< 2^25)
  return tiles_new * (tiles_new + 1) / 2 + tiles_new * (tiles - tiles_new) < (1ull << 31);
}
// AUTO's two bounds for a border, from the counts the positions part reads
// back: the kept columns, their entries, and those of them at new positions.
// The index border kernel lets every new entry read the members before it: a
// column held by a new and b old rows (a >= 1, a + b >= 2; the new rows are
// its last members) costs a b + a (a - 1) / 2 reads.  Over the columns,
// sum a b >= sum b = old_entries (a >= 1), and sum a (a - 1) / 2 >=
// (new_entries^2 / n_columns - new_entries) / 2 (Cauchy-Schwarz; the left side
// is an integer, so the floors only lower the right; new_entries >= n_columns).
inline uint64_t border_chunk_rounds(uint64_t n, uint64_t n_old, uint64_t n_columns) {
  const uint64_t tiles = (n + kTile - 1) / kTile, tiles_new = (n - n_old + kTile - 1) / kTile;
  return (tiles_new * (tiles_new + 1) / 2 + tiles_new * (tiles - tiles_new)) * ((n_columns + kChunk - 1) / kChunk);
}
inline uint64_t border_index_reads(uint64_t n_columns, uint64_t column_entries, uint64_t new_entries) {
  if (!n_columns) return 0;  // (new_entries <= column_entries < 2^31)
  return (column_entries - new_entries) + (new_entries * new_entries / n_columns - new_entries) / 2;
}

// ---- the columns on the host ------------------------------------------------------
// What the device builds with a radix sort and a scan: piece[a] the ascending
// column ids of position a.  rows == nullptr: position a is row a.  n_new <
// kNoColumn: the border column rule with the first n_new positions new
// (new_entries then counts their kept entries).
struct Columns {
  uint64_t n_entries = 0, n_columns = 0, column_entries = 0, new_entries = 0;
  std::vector<std::vector<uint32_t>> piece;
};
inline Columns columns_host(const uint64_t* sketches, const uint32_t* lens, uint32_t sketch_size, const uint32_t* rows,
                            uint32_t m, uint32_t n_new = kNoColumn) {
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
  uint64_t sum = 0, head = 0;  // head: the first entry of the run of equal hashes that holds i
  for (uint64_t i = 0; i < K.size(); ++i) {
    if (i == 0 || K[i] != K[i - 1]) head = i;
    const bool kept = n_new == kNoColumn || border_column_kept((uint32_t)(keys[head].slot / sketch_size), n_new);
    if (!kept) continue;
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
    if (n_new != kNoColumn && a < n_new) c.new_entries += c.piece[a].size();
  }
  return c;
}

// ---- groups ------------------------------------------------------
// The matrices of many groups in one call.  Group g is members[offsets[g] ..
// offsets[g + 1]): row indices in any order, a row may be listed twice in a
// group and in several groups, a group may be empty.  Positions are numbered
// through all groups (P = offsets[n_groups]); tiles of kTile positions are
// local to a group, the first tile of group g begins at offsets[g].
//   The grouped column rule.  A column of group g is a distinct hash held at
//     two or more positions *of g*: the same hash in two groups gives two
//     columns (or none, held once in each).  The entries are sorted by
//     (group, hash), Gr[i] the group of entry i; column ids ascend with
//     (group, hash), and a piece stores ids local to its group (the id minus
//     the group's first id), so that cursor_at, next_chunk and the chunk loop
//     see one group's columns numbered from 0.
//   Cells.  A cell exists only inside a group: block g begins at cell_off[g] =
//     sum over h < g of m_h^2 and is row-major [m_g x m_g]; the diagonal rule,
//     the off-diagonal rule and cell_counts are unchanged.
//   Workgroups.  Group g takes group_tile_pairs(m_g) workgroups, none when
//     m_g < 2 (the one cell of a single position is (len, len) without a
//     product); tp_off is their exclusive sum and workgroup w belongs to the
//     group g with tp_off[g] <= w < tp_off[g + 1].
GG_MATRIX_HD inline bool same_column(const uint64_t* K, const uint32_t* Gr, uint64_t i, uint64_t j) {
  return K[i] == K[j] && Gr[i] == Gr[j];
}
GG_MATRIX_HD inline bool in_column(const uint64_t* K, const uint32_t* Gr, uint64_t i, uint64_t ne) {
  return (i > 0 && same_column(K, Gr, i, i - 1)) || (i + 1 < ne && same_column(K, Gr, i + 1, i));
}
GG_MATRIX_HD inline bool column_head(const uint64_t* K, const uint32_t* Gr, uint64_t i, uint64_t ne) {
  return (i == 0 || !same_column(K, Gr, i, i - 1)) && i + 1 < ne && same_column(K, Gr, i + 1, i);
}
GG_MATRIX_HD inline uint64_t column_flags(const uint64_t* K, const uint32_t* Gr, uint64_t i, uint64_t ne) {
  return (uint64_t)column_head(K, Gr, i, ne) | ((uint64_t)in_column(K, Gr, i, ne) << 32);
}
// the first column id of the group whose first sorted entry is e0, from the inclusive sums
GG_MATRIX_HD inline uint32_t group_first_id(const uint64_t* sums, uint64_t e0) {
  return e0 ? (uint32_t)sums[e0 - 1] : 0u;
}

GG_MATRIX_HD inline uint32_t group_tile_pairs(uint32_t m) { return m >= 2 ? tile_pairs_of(tiles_of(m)) : 0u; }
// the group of workgroup w: the last g with tp_off[g] <= w (w < tp_off[n_groups]; groups without workgroups are passed over)
template <typename Ptr>
GG_MATRIX_HD inline uint32_t group_of_workgroup(Ptr tp_off, uint32_t n_groups, uint32_t w) {
  uint32_t lo = 0, hi = n_groups;  // tp_off[lo] <= w < tp_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (tp_off[mid] <= w) lo = mid; else hi = mid;
  }
  return lo;
}
// the group of position p: the last g with offsets[g] <= p (p < offsets[n_groups]; empty groups are passed over)
template <typename Ptr>
GG_MATRIX_HD inline uint32_t group_of_position(Ptr offsets, uint32_t n_groups, uint32_t p) {
  return group_of_workgroup(offsets, n_groups, p);
}

// The limits of one grouped call: P s < 2^31 sketch slots, fewer than 2^32
// cells, fewer than 2^31 workgroups.  (group_tile_pairs(m) <= m^2 / 4, so the
// cells' limit is always the first of the last two to break.)
inline bool group_limits_ok(uint64_t positions, uint64_t sketch_size, uint64_t cells, uint64_t tile_pairs) {
  return positions * sketch_size < (1ull << 31) && cells < (1ull << 32) && tile_pairs < (1ull << 31);
}
// cell_off[0 .. n_groups] and tp_off[0 .. n_groups] (either may be null) of
// ascending offsets; false when a limit is broken (sketch_size 1: the
// positions alone)
inline bool group_layout(const uint32_t* offsets, uint32_t n_groups, uint64_t sketch_size, uint64_t* cell_off,
                         uint32_t* tp_off) {
  uint64_t cells = 0, pairs = 0;
  for (uint32_t g = 0; g <= n_groups; ++g) {
    if (cell_off) cell_off[g] = cells;
    if (tp_off) tp_off[g] = (uint32_t)pairs;
    if (g == n_groups) break;
    const uint64_t m = offsets[g + 1] - offsets[g];
    cells += m * m;
    pairs += m < (1ull << 16) ? group_tile_pairs((uint32_t)m) : (1ull << 31);
    if (!group_limits_ok(offsets[g + 1], sketch_size, cells, pairs)) return false;
  }
  return true;
}

// The columns of every group on the host: piece[p] the ascending group-local
// column ids of position p, first_id[g] the group's first id.
struct GroupColumns {
  uint64_t n_entries = 0, n_columns = 0, column_entries = 0;
  std::vector<std::vector<uint32_t>> piece;
  std::vector<uint32_t> first_id;
};
inline GroupColumns columns_host(const uint64_t* sketches, const uint32_t* lens, uint32_t sketch_size,
                                 const uint32_t* members, const uint32_t* offsets, uint32_t n_groups) {
  struct Key {
    uint32_t group;
    uint64_t hash;
    uint64_t slot;
  };
  const uint32_t P = offsets[n_groups];
  std::vector<Key> keys;
  std::vector<uint64_t> first_entry(n_groups + 1, 0);
  for (uint32_t g = 0; g < n_groups; ++g) {
    first_entry[g] = keys.size();
    for (uint32_t p = offsets[g]; p < offsets[g + 1]; ++p) {
      const uint32_t row = members[p];
      for (uint32_t e = 0; e < lens[row]; ++e)
        keys.push_back(Key{g, sketches[(size_t)row * sketch_size + e], (uint64_t)p * sketch_size + e});
    }
  }
  first_entry[n_groups] = keys.size();
  std::stable_sort(keys.begin(), keys.end(), [](const Key& x, const Key& y) {
    return x.group != y.group ? x.group < y.group : x.hash < y.hash;
  });
  std::vector<uint64_t> K(keys.size()), sums(keys.size());
  std::vector<uint32_t> Gr(keys.size());
  for (size_t i = 0; i < keys.size(); ++i) {
    K[i] = keys[i].hash;
    Gr[i] = keys[i].group;
  }
  GroupColumns c;
  c.n_entries = K.size();
  uint64_t sum = 0;
  for (uint64_t i = 0; i < K.size(); ++i) sums[i] = sum += column_flags(K.data(), Gr.data(), i, K.size());
  c.first_id.resize(n_groups);
  for (uint32_t g = 0; g < n_groups; ++g) c.first_id[g] = group_first_id(sums.data(), first_entry[g]);
  std::vector<uint32_t> id_of((size_t)P * sketch_size, kNoColumn);
  for (uint64_t i = 0; i < K.size(); ++i)
    if (in_column(K.data(), Gr.data(), i, K.size()))
      id_of[keys[i].slot] = column_id(sums[i]) - group_first_id(sums.data(), first_entry[Gr[i]]);
  c.n_columns = (uint32_t)sum;
  c.column_entries = sum >> 32;
  c.piece.resize(P);
  for (uint32_t p = 0; p < P; ++p)
    for (uint32_t e = 0; e < lens[members[p]]; ++e)
      if (id_of[(size_t)p * sketch_size + e] != kNoColumn) c.piece[p].push_back(id_of[(size_t)p * sketch_size + e]);
  return c;
}

}  // namespace matrix
}  // namespace gg
