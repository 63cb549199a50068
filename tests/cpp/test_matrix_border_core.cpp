// The border form of the matrix product (galah_amd/csrc/matrix_core.hpp, "the
// border form") driven on the host, stand-alone.  As test_matrix_pairs_core.cpp
// walks the pair form: the tiled incidence product through the core's own
// index arithmetic (cursors, chunk jumps, byte images, fragments, the C/D map;
// the matrix instruction emulated from its definition), here over the border's
// positions (new rows first), the border tile-pair numbering, the border column
// rule and the border's visited rule.
//
// The reference is validate::merge_counts and the pass test over all border
// pairs (i < j, j >= n_old).  Inputs are random -- empty rows, identical rows,
// n on both sides of the tile edges, every class of n_old (0, 1, inside the
// first tile, at and around the tile edges, n - 1, n) -- under random cmin
// tables, non-monotone ones, cmin[0] == 0, all zero and nothing passes.  It
// asserts beyond the equality of the lists:
//   - the numbering covers every border tile pair once and its inverse round-
//     trips, Tn == T, Tn == 1 and slices across the triangle / rectangle seam
//     included;
//   - no visited cell loses a count to a dropped column (the product's count
//     is the merge's common), and a tile pair left early holds no shared hash;
//   - the column counts equal a count from a map, and AUTO's lower bound of
//     the index border's member reads never exceeds their exact sum;
//   - border_limits_ok on both sides of each boundary.
//
// Prints "ok <cases> <pairs>" and returns 0, or the first mismatch and 1.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../../galah_amd/csrc/matrix_core.hpp"

using namespace gg;
using matrix::kChunk;
using matrix::kNoColumn;
using matrix::kTile;
using matrix::kTileBytes;

static uint64_t rng_state = 0xA0761D6478BD642Full;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }

struct Input {
  uint32_t n = 0, s = 0, n_old = 0;
  std::vector<uint64_t> sk;
  std::vector<uint32_t> lens;
};

struct Tables {
  std::vector<uint32_t> cmin, sufmin;
  uint32_t tmax = 0;
  bool zero_passes = false;
};

// kind 0: a threshold-like table, cmin[t] = ceil(f t); 1: non-monotone, with
// totals at which nothing passes; 2: the same with cmin[0] == 0; 3: everything
// passes; 4: nothing passes
static Tables make_tables(uint32_t s, uint32_t kind) {
  Tables T;
  T.tmax = 2 * s;
  T.cmin.assign(T.tmax + 1, 0);
  const uint32_t num = 1 + rnd_below(9);
  for (uint32_t t = 0; t <= T.tmax; ++t) {
    uint32_t v;
    if (kind == 0) v = t == 0 ? 0xFFFFFFFFu : (t * num + 9) / 10;
    else if (kind == 1) v = rnd_below(5) == 0 ? 0xFFFFFFFFu : 1 + rnd_below(t + 1);  // never 0
    else if (kind == 2) v = rnd_below(5) == 0 ? 0xFFFFFFFFu : rnd_below(t + 2);
    else if (kind == 3) v = 0;
    else v = 0xFFFFFFFFu;
    T.cmin[t] = v;
  }
  if (kind == 2) T.cmin[0] = 0;
  // as ensure_cmin: sufmin[t] = min(cmin[t .. tmax]); zero_passes = sufmin[0] == 0
  T.sufmin.assign(T.tmax + 1, 0xFFFFFFFFu);
  uint32_t mn = 0xFFFFFFFFu;
  for (uint32_t t = T.tmax + 1; t-- > 0;) {
    mn = std::min(mn, T.cmin[t]);
    T.sufmin[t] = mn;
  }
  T.zero_passes = T.sufmin[0] == 0;
  return T;
}

static void mfma_16x16x64(const uint8_t* img_a, const uint8_t* img_b, uint32_t ks, uint32_t blk_a, uint32_t blk_b,
                          int32_t acc[64][4]) {
  for (uint32_t lane = 0; lane < 64; ++lane)
    for (uint32_t reg = 0; reg < 4; ++reg) {
      const uint32_t i = matrix::cd_row(lane, reg), j = matrix::cd_col(lane);
      int32_t sum = 0;
      for (uint32_t g = 0; g < 4; ++g) {
        const uint8_t* fa = img_a + matrix::fragment_offset(i + 16 * g, ks, blk_a);
        const uint8_t* fb = img_b + matrix::fragment_offset(j + 16 * g, ks, blk_b);
        uint64_t a0, a1, b0, b1;
        memcpy(&a0, fa, 8);
        memcpy(&a1, fa + 8, 8);
        if ((a0 | a1) == 0) continue;
        memcpy(&b0, fb, 8);
        memcpy(&b1, fb + 8, 8);
        sum += __builtin_popcountll(a0 & b0) + __builtin_popcountll(a1 & b1);
      }
      acc[lane][reg] += sum;
    }
}

using Rec = std::array<uint32_t, 4>;  // i, j, common, total
static uint64_t n_pairs = 0, n_early = 0, n_rejected = 0, n_mixed_skipped = 0, n_dropped_columns = 0, n_empty_old = 0;

static bool run(const Input& in, const Tables& T, const char* what) {
  const uint32_t n = in.n, s = in.s, n_old = in.n_old, n_new = n - n_old;
  if (!matrix::border_limits_ok(n, n_old, s)) {
    printf("%s: limits\n", what);
    return false;
  }
  std::vector<uint32_t> rows(n);  // the border's positions: the new rows first
  for (uint32_t a = 0; a < n; ++a) rows[a] = matrix::border_row_of(a, n, n_old);
  for (uint32_t a = 0; a < n; ++a)
    if (rows[a] >= n || (a < n_new) != (rows[a] >= n_old)) {
      printf("%s: position %u names row %u\n", what, a, rows[a]);
      return false;
    }
  const matrix::Columns col = matrix::columns_host(in.sk.data(), in.lens.data(), s, rows.data(), n, n_new);

  // ---- the column counts from a map, and the exact member reads of the index border
  std::map<uint64_t, std::vector<uint32_t>> holders;  // hash -> rows, ascending
  for (uint32_t g = 0; g < n; ++g)
    for (uint32_t e = 0; e < in.lens[g]; ++e) holders[in.sk[(size_t)g * s + e]].push_back(g);
  uint64_t want_cols = 0, want_entries = 0, want_new = 0, exact_reads = 0, all_cols = 0;
  for (const auto& h : holders) {
    const auto& r = h.second;
    uint64_t a = 0;
    for (uint32_t g : r) a += g >= n_old;
    if (r.size() >= 2) ++all_cols;
    if (r.size() >= 2 && a >= 1) {
      ++want_cols;
      want_entries += r.size();
      want_new += a;
    }
    // every new entry reads the members before it (the rows are ascending: the new ones are the last)
    for (size_t x = 0; x < r.size(); ++x)
      if (r[x] >= n_old) exact_reads += x;
  }
  if (col.n_columns != want_cols || col.column_entries != want_entries || col.new_entries != want_new) {
    printf("%s: columns %llu / %llu / %llu, the map counts %llu / %llu / %llu\n", what, (unsigned long long)col.n_columns,
           (unsigned long long)col.column_entries, (unsigned long long)col.new_entries, (unsigned long long)want_cols,
           (unsigned long long)want_entries, (unsigned long long)want_new);
    return false;
  }
  n_dropped_columns += all_cols - want_cols;
  const uint64_t bound = matrix::border_index_reads(col.n_columns, col.column_entries, col.new_entries);
  if (bound > exact_reads) {
    printf("%s: index_reads %llu overstates the exact %llu\n", what, (unsigned long long)bound,
           (unsigned long long)exact_reads);
    return false;
  }
  for (uint32_t a = n_new; a < n; ++a) n_empty_old += col.piece[a].empty() && in.lens[rows[a]] > 0;

  // ---- the reference: the merge and the pass test over all border pairs
  std::vector<Rec> want;
  for (uint32_t i = 0; i + 1 < n; ++i)
    for (uint32_t j = std::max(i + 1, n_old); j < n; ++j) {
      uint32_t c, t;
      validate::merge_counts(in.sk.data() + (size_t)i * s, in.lens[i], in.sk.data() + (size_t)j * s, in.lens[j], &c, &t);
      if (t <= T.tmax && c >= T.cmin[t]) want.push_back(Rec{i, j, c, t});
    }

  // ---- the tiled product and the pair epilogue, as the kernel walks them
  std::vector<Rec> got;
  const uint32_t NT = matrix::tiles_of(n), Tn = matrix::tiles_of(n_new);
  const uint32_t P = n_new ? matrix::border_tile_pairs(Tn, NT) : 0;
  if (matrix::border_chunk_rounds(n, n_old, col.n_columns) != (uint64_t)P * ((col.n_columns + kChunk - 1) / kChunk)) {
    printf("%s: chunk rounds\n", what);
    return false;
  }
  std::vector<uint8_t> image(2 * kTileBytes);
  std::set<std::pair<uint32_t, uint32_t>> seen_cells;
  for (uint32_t p = 0; p < P; ++p) {
    uint32_t ti, tj;
    matrix::border_tile_pair_of(p, Tn, &ti, &tj);
    if (!(ti < Tn && ti <= tj && tj < NT) || matrix::border_tile_pair_index(ti, tj, Tn) != p) {
      printf("%s: workgroup %u is tile pair (%u, %u)\n", what, p, ti, tj);
      return false;
    }
    const bool diag = ti == tj;
    const uint32_t sides = diag ? 1u : 2u;
    auto pos_of = [&](uint32_t r) { return (r < kTile ? ti : tj) * kTile + (r & (kTile - 1)); };
    auto piece_of = [&](uint32_t r) -> const std::vector<uint32_t>& {
      static const std::vector<uint32_t> none;
      return pos_of(r) < n ? col.piece[pos_of(r)] : none;
    };
    uint32_t cur[2 * kTile] = {0};
    static int32_t acc[4][4][64][4];  // [wave][block of tj][lane][reg]
    memset(acc, 0, sizeof acc);
    uint32_t k0 = 0;
    bool ran = false;
    for (;;) {
      uint32_t mn[2] = {kNoColumn, kNoColumn};
      for (uint32_t r = 0; r < sides * kTile; ++r) {
        const auto& pc = piece_of(r);
        cur[r] = matrix::cursor_at(pc.data(), cur[r], (uint32_t)pc.size(), k0);
        if (cur[r] < pc.size() && pc[cur[r]] < mn[r / kTile]) mn[r / kTile] = pc[cur[r]];
      }
      const uint32_t kc = matrix::next_chunk(mn[0], diag ? mn[0] : mn[1]);
      if (kc == kNoColumn) break;
      if (kc != k0) {
        k0 = kc;
        continue;
      }
      std::fill(image.begin(), image.begin() + sides * kTileBytes, 0);
      for (uint32_t r = 0; r < sides * kTile; ++r) {
        const auto& pc = piece_of(r);
        for (uint32_t e = cur[r]; e < pc.size() && pc[e] - k0 < kChunk; ++e)
          image[(r < kTile ? 0 : kTileBytes) + matrix::image_offset(r & (kTile - 1), pc[e] - k0)] = 1;
      }
      const uint8_t* img_a = image.data();
      const uint8_t* img_b = image.data() + (diag ? 0 : kTileBytes);
      for (uint32_t wave = 0; wave < 4; ++wave)
        for (uint32_t ks = 0; ks < matrix::kKSteps; ++ks)
          for (uint32_t nb = 0; nb < 4; ++nb) mfma_16x16x64(img_a, img_b, ks, wave, nb, acc[wave][nb]);
      k0 += kChunk;
      ran = true;
    }

    const bool early = matrix::pair_early_exit(ran, T.zero_passes);
    uint32_t staged = 0;
    for (uint32_t wave = 0; wave < 4; ++wave)
      for (uint32_t nb = 0; nb < 4; ++nb)
        for (uint32_t lane = 0; lane < 64; ++lane)
          for (uint32_t reg = 0; reg < 4; ++reg) {
            const uint32_t ra = wave * 16 + matrix::cd_row(lane, reg), rb = nb * 16 + matrix::cd_col(lane);
            const uint32_t pa = ti * kTile + ra, pb = tj * kTile + rb;
            if (!(pa < n && pb < n)) continue;
            const uint32_t ga = rows[pa], gb = rows[pb], la = in.lens[ga], lb = in.lens[gb];
            if (!matrix::border_visited(pa, pb, n_new, ga, gb)) {
              n_mixed_skipped += pa < pb && pa >= n_new;
              continue;
            }
            if (!seen_cells.insert({std::min(ga, gb), std::max(ga, gb)}).second) {
              printf("%s: rows (%u, %u) visited twice\n", what, ga, gb);
              return false;
            }
            const uint64_t* A = in.sk.data() + (size_t)ga * s;
            const uint64_t* B = in.sk.data() + (size_t)gb * s;
            uint32_t c_ref, t_ref;
            validate::merge_counts(A, la, B, lb, &c_ref, &t_ref);
            const bool ref_pass = t_ref <= T.tmax && c_ref >= T.cmin[t_ref];
            const uint32_t common_ab = ran ? (uint32_t)acc[wave][nb][lane][reg] : 0u;
            if (common_ab != c_ref) {  // a dropped column took a count from a visited cell, or a chunk was missed
              printf("%s: cell (%u, %u) rows (%u, %u): the product counts %u, the merge %u\n", what, pa, pb, ga, gb,
                     common_ab, c_ref);
              return false;
            }
            if (early) {  // the kernel returns before the epilogue: nothing of the tile pair may pass
              if (ref_pass) {
                printf("%s: early exit of tile pair (%u, %u), yet (%u, %u) passes\n", what, ti, tj, pa, pb);
                return false;
              }
              continue;
            }
            const bool cand = matrix::pair_candidate(la, lb, common_ab, T.cmin.data(), T.sufmin.data());
            if (ref_pass && !cand) {
              printf("%s: the candidate test drops (%u, %u)\n", what, pa, pb);
              return false;
            }
            if (!cand) ++n_rejected;
            uint32_t common, total;
            if (matrix::pair_cell(A, la, la ? A[la - 1] : 0, B, lb, lb ? B[lb - 1] : 0, common_ab, T.cmin.data(),
                                  T.sufmin.data(), T.tmax, &common, &total)) {
              got.push_back(Rec{std::min(ga, gb), std::max(ga, gb), common, total});
              ++staged;
            }
          }
    if (early) ++n_early;
    if (staged > matrix::kPairStage) {
      printf("%s: tile pair (%u, %u) stages %u pairs\n", what, ti, tj, staged);
      return false;
    }
  }
  // every border pair is a visited cell, once
  if (seen_cells.size() != (uint64_t)n_new * n_old + (uint64_t)n_new * (n_new ? n_new - 1 : 0) / 2) {
    printf("%s: %zu cells visited\n", what, seen_cells.size());
    return false;
  }
  for (const auto& cell : seen_cells)
    if (cell.second < n_old) {
      printf("%s: the old pair (%u, %u) was visited\n", what, cell.first, cell.second);
      return false;
    }
  std::sort(want.begin(), want.end());
  std::sort(got.begin(), got.end());
  if (got != want) {
    printf("%s: %zu pairs emitted, the merge passes %zu", what, got.size(), want.size());
    for (size_t x = 0; x < std::max(got.size(), want.size()); ++x)
      if (x >= got.size() || x >= want.size() || got[x] != want[x]) {
        if (x < got.size()) printf("; first emitted (%u, %u, %u, %u)", got[x][0], got[x][1], got[x][2], got[x][3]);
        if (x < want.size()) printf("; wanted (%u, %u, %u, %u)", want[x][0], want[x][1], want[x][2], want[x][3]);
        break;
      }
    printf("\n");
    return false;
  }
  n_pairs += got.size();
  return true;
}

// rows over a shared pool: empty rows, length-1 rows, full rows, identical rows
static Input random_input(uint32_t n, uint32_t s, uint32_t pool) {
  Input in;
  in.n = n;
  in.s = s;
  in.sk.assign((size_t)n * s, 0);
  in.lens.assign(n, 0);
  pool = std::max(pool, s + 1);
  for (uint32_t g = 0; g < n; ++g) {
    const uint32_t kind = rnd_below(10);
    if (kind == 3 && g > 0) {  // identical to an earlier row
      const uint32_t o = rnd_below(g);
      memcpy(&in.sk[(size_t)g * s], &in.sk[(size_t)o * s], s * sizeof(uint64_t));
      in.lens[g] = in.lens[o];
      continue;
    }
    const uint32_t len = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? s : 1 + rnd_below(s);
    std::set<uint64_t> h;
    while (h.size() < len) h.insert(1001 + (uint64_t)rnd_below(pool) * 0x9E3779B97F4A7C15ull);
    uint32_t e = 0;
    for (uint64_t v : h) in.sk[(size_t)g * s + e++] = v;
    in.lens[g] = e;
  }
  return in;
}

// every class of n_old for n rows
static std::vector<uint32_t> n_old_classes(uint32_t n) {
  std::set<uint32_t> c{0u, n};
  for (uint32_t v : {1u, 13u, 63u, 64u, 65u, 100u, 128u, 129u}) {
    if (v <= n) c.insert(v);      // n_old itself
    if (v <= n) c.insert(n - v);  // n_new
  }
  return std::vector<uint32_t>(c.begin(), c.end());
}

// The numbering and its inverse over every (Tn, T) of a range and at large
// counts, the slices across the seam, and the limits at their boundaries.
static bool numbering_and_limits() {
  for (uint32_t T = 1; T <= 14; ++T)
    for (uint32_t Tn = 1; Tn <= T; ++Tn) {
      const uint32_t P = matrix::border_tile_pairs(Tn, T);
      uint32_t expect = 0;
      for (uint32_t ti = 0; ti < Tn; ++ti) expect += T - ti;
      if (P != expect) return false;
      std::set<std::pair<uint32_t, uint32_t>> seen;
      for (uint32_t slice = 1; slice <= P; slice += slice < 8 ? 1 : P) {  // slices of 1 .. 8 and of everything
        seen.clear();
        uint32_t launched = 0;
        for (uint32_t base = 0; base < P; base += std::min(slice, P - base)) {
          const uint32_t grid = std::min(slice, P - base);
          if (base != launched) return false;
          launched += grid;
          for (uint32_t w = 0; w < grid; ++w) {
            uint32_t ti, tj;
            matrix::border_tile_pair_of(base + w, Tn, &ti, &tj);
            if (!(ti < Tn && ti <= tj && tj < T)) return false;
            if (matrix::border_tile_pair_index(ti, tj, Tn) != base + w) return false;
            if (!seen.insert({ti, tj}).second) return false;
          }
        }
        if (launched != P || seen.size() != P) return false;
      }
    }
  {  // large: 1,000 new tiles of 60,000 -- around the seam and at the end
    const uint32_t Tn = 1000, T = 60000, tri = matrix::tile_pairs_of(Tn), P = matrix::border_tile_pairs(Tn, T);
    if (P != tri + Tn * (T - Tn)) return false;
    for (uint32_t p : {0u, tri - 1, tri, tri + 1, tri + Tn - 1, tri + Tn, P - 1}) {
      uint32_t ti, tj;
      matrix::border_tile_pair_of(p, Tn, &ti, &tj);
      if (!(ti < Tn && ti <= tj && tj < T) || matrix::border_tile_pair_index(ti, tj, Tn) != p) return false;
      if ((p < tri) != (tj < Tn)) return false;
    }
    uint32_t ti, tj;
    matrix::border_tile_pair_of(P - 1, Tn, &ti, &tj);
    if (ti != Tn - 1 || tj != T - 1) return false;
  }
  // the limits: n_old <= n; n s < 2^31; fewer than 2^31 border tile pairs
  const uint64_t most = 65535ull * kTile;  // all rows new: the pair form's triangle, 2^31 - 32,768 tile pairs
  bool ok = matrix::border_limits_ok(10, 10, 1000) && !matrix::border_limits_ok(10, 11, 1000) &&
            matrix::border_limits_ok(0, 0, 1000) && !matrix::border_limits_ok(0, 1, 1000);
  ok = ok && matrix::border_limits_ok(2147483, 0, 1000) && !matrix::border_limits_ok(2147484, 2147483, 1000);
  ok = ok && matrix::border_limits_ok(2147483, 2147483, 1000) && !matrix::border_limits_ok(2147484, 2147484, 1000);
  ok = ok && matrix::border_limits_ok(most, 0, 1) && !matrix::border_limits_ok(most + 1, 0, 1);
  ok = ok && !matrix::border_limits_ok(most + 1, 1, 1);  // one row old: the same triangle and 65,535 pairs with the old tile
  ok = ok && matrix::border_limits_ok(most, kTile, 1);  // 65,534 new tiles of 65,535: one pair fewer than all new
  // n = 2^31 - 1 rows at s = 1 (2^25 tiles): 64 new tiles give 2080 + 64 (2^25 - 64) < 2^31, 65 do not
  const uint64_t big = (1ull << 31) - 1;
  ok = ok && matrix::border_limits_ok(big, big - 4096, 1) && !matrix::border_limits_ok(big, big - 4097, 1);
  ok = ok && !matrix::border_limits_ok(big + 1, big, 1) && matrix::border_limits_ok(big, big, 1);
  // the bounds' arithmetic at hand-made counts
  ok = ok && matrix::border_index_reads(0, 0, 0) == 0 && matrix::border_index_reads(1, 2, 1) == 1 &&
       matrix::border_index_reads(1, 2, 2) == 1 && matrix::border_index_reads(1, 5, 3) == 2 + 3 &&
       matrix::border_chunk_rounds(200, 100, 513) == 7 * 2 && matrix::border_chunk_rounds(200, 200, 513) == 0;
  return ok;
}

int main() {
  uint64_t cases = 0;
  char what[128];
  if (!numbering_and_limits()) {
    printf("numbering and limits\n");
    return 1;
  }
  // many tiny inputs under every kind of table: one tile pair, one chunk, every n_old
  for (uint32_t it = 0; it < 3000; ++it, ++cases) {
    const uint32_t n = 1 + rnd_below(12), s = 1 + rnd_below(24), kind = it % 5;
    Input in = random_input(n, s, 1 + rnd_below(3 * s));
    in.n_old = rnd_below(n + 1);
    snprintf(what, sizeof what, "tiny %u (n %u, s %u, n_old %u, table %u)", it, n, s, in.n_old, kind);
    if (!run(in, make_tables(s, kind), what)) return 1;
  }
  // n on both sides of the tile edges, every class of n_old; dense and sparse pools
  uint32_t rep = 0;
  for (uint32_t n : {2u, 63u, 64u, 65u, 130u, 193u})
    for (uint32_t n_old : n_old_classes(n)) {
      for (uint32_t dense = 0; dense < 2; ++dense, ++rep, ++cases) {
        const uint32_t s = 16, kind = rep % 5;
        Input in = random_input(n, s, dense ? 40 : 6000);
        in.n_old = n_old;
        snprintf(what, sizeof what, "tile edge n %u n_old %u pool %u table %u", n, n_old, dense, kind);
        if (!run(in, make_tables(s, kind), what)) return 1;
      }
    }
  // old rows that share more than a chunk of hashes among themselves only, a few new rows related to two old
  // rows, and old rows unrelated to every new row: dropped columns, empty pieces, early exits
  for (uint32_t kind = 0; kind < 5; ++kind, ++cases) {
    Input in;
    in.n = 200;
    in.n_old = 190;
    in.s = 24;
    in.sk.assign((size_t)in.n * in.s, 0);
    in.lens.assign(in.n, 0);
    for (uint32_t g = 0; g < in.n; ++g) {
      std::set<uint64_t> h;
      if (g < in.n_old) {
        for (uint32_t e = 0; e < 12; ++e) h.insert(5000 + 12 * (uint64_t)(g / 2) + e);  // shared with one old neighbour
        for (uint32_t e = 0; e < 6; ++e) h.insert(100000 + 10 * (uint64_t)g + e);        // its own
      } else {
        for (uint32_t e = 0; e < 8; ++e) h.insert(5000 + 12 * (uint64_t)(g - in.n_old) * 9 + e);  // of old rows 18 x, 18 x + 1
        for (uint32_t e = 0; e < 4; ++e) h.insert(900000 + (uint64_t)(g % 3) * 7 + e);             // among new rows
        h.insert(800000 + g);                                                                      // alone
      }
      uint32_t e = 0;
      for (uint64_t v : h) in.sk[(size_t)g * in.s + e++] = v;
      in.lens[g] = e;
    }
    snprintf(what, sizeof what, "old-only columns, table %u", kind);
    if (!run(in, make_tables(in.s, kind), what)) return 1;
  }
  if (n_early == 0 || n_rejected == 0 || n_pairs == 0 || n_mixed_skipped == 0 || n_dropped_columns < 512 ||
      n_empty_old == 0) {
    printf("coverage: %llu early exits, %llu rejected, %llu pairs, %llu mixed-row cells skipped, %llu dropped columns, "
           "%llu old rows with an empty piece\n",
           (unsigned long long)n_early, (unsigned long long)n_rejected, (unsigned long long)n_pairs,
           (unsigned long long)n_mixed_skipped, (unsigned long long)n_dropped_columns, (unsigned long long)n_empty_old);
    return 1;
  }
  printf("ok %llu %llu\n", (unsigned long long)cases, (unsigned long long)n_pairs);
  return 0;
}
