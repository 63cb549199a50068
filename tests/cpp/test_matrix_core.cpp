// The rules of the dense ANI matrix (galah_amd/csrc/matrix_core.hpp) driven on
// the host, stand-alone.  For a few thousand small random inputs -- empty
// rows, length-1 rows, identical rows, a hash in every row, rows listed
// twice, m on both sides of the tile edges and column counts on both sides
// of the chunk edges -- the tiled incidence product is run through the
// core's own index arithmetic (tile pairs, cursors, chunk jumps, byte images,
// fragments, the C/D map; the matrix instruction itself is emulated from its
// definition D[i][j] = sum_k A[i][k] B[k][j]) and every cell must equal
// validate::merge_counts.  The column rule (columns, entries in them, each
// row's piece) is checked against a std::map.
//
// Prints "ok <cases> <cells>" and returns 0, or the first mismatch and 1.
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }

struct Input {
  uint32_t n = 0, s = 0;
  std::vector<uint64_t> sk;
  std::vector<uint32_t> lens;
  std::vector<uint32_t> rows;  // empty: positions are rows 0 .. m-1
  uint32_t m = 0;
  void set_row(uint32_t g, const std::set<uint64_t>& h) {
    uint32_t e = 0;
    for (uint64_t v : h) sk[(size_t)g * s + e++] = v;
    lens[g] = e;
  }
};

static Input make(uint32_t n, uint32_t s) {
  Input in;
  in.n = n;
  in.s = s;
  in.sk.assign((size_t)n * s, 0);
  in.lens.assign(n, 0);
  in.m = n;
  return in;
}

// one 16 x 16 x 64 step from its definition: lane (i + 16 g) holds A[i][16 g .. 16 g + 15],
// lane (j + 16 g) holds B[16 g .. 16 g + 15][j]; register reg of lane l is D[cd_row][cd_col]
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
        // (the bytes are 0 or 1: the i8 dot product is the count of common ones)
        sum += __builtin_popcountll(a0 & b0) + __builtin_popcountll(a1 & b1);
      }
      acc[lane][reg] += sum;
    }
}

static uint64_t n_cells = 0;

static bool run(const Input& in, const char* what, int64_t want_columns = -1) {
  const uint32_t m = in.m, s = in.s;
  const uint32_t* rows = in.rows.empty() ? nullptr : in.rows.data();
  auto row_of = [&](uint32_t a) { return rows ? rows[a] : a; };
  const matrix::Columns col = matrix::columns_host(in.sk.data(), in.lens.data(), s, rows, m);

  // ---- the column rule against a map: hash -> positions holding it
  std::map<uint64_t, std::vector<uint32_t>> held;
  uint64_t entries = 0;
  for (uint32_t a = 0; a < m; ++a)
    for (uint32_t e = 0; e < in.lens[row_of(a)]; ++e, ++entries) held[in.sk[(size_t)row_of(a) * s + e]].push_back(a);
  std::vector<std::vector<uint32_t>> piece(m);
  uint64_t n_columns = 0, column_entries = 0;
  for (const auto& kv : held) {
    if (kv.second.size() < 2) continue;
    for (uint32_t a : kv.second) piece[a].push_back((uint32_t)n_columns);
    ++n_columns;
    column_entries += kv.second.size();
  }
  if (col.n_entries != entries || col.n_columns != n_columns || col.column_entries != column_entries ||
      col.piece != piece || (want_columns >= 0 && (uint64_t)want_columns != n_columns)) {
    printf("%s: column rule: entries %llu/%llu columns %llu/%llu (wanted %lld) column entries %llu/%llu pieces %s\n", what,
           (unsigned long long)col.n_entries, (unsigned long long)entries, (unsigned long long)col.n_columns,
           (unsigned long long)n_columns, (long long)want_columns, (unsigned long long)col.column_entries,
           (unsigned long long)column_entries, col.piece == piece ? "equal" : "differ");
    return false;
  }

  // ---- the tiled product, as the kernel walks it
  const uint32_t T = matrix::tiles_of(m), P = matrix::tile_pairs_of(T);
  std::vector<uint8_t> seen((size_t)T * T, 0);
  std::vector<uint8_t> image(2 * kTileBytes);
  for (uint32_t p = 0; p < P; ++p) {
    uint32_t ti, tj;
    matrix::tile_pair_of(p, &ti, &tj);
    if (!(ti <= tj && tj < T) || seen[(size_t)ti * T + tj]++) {
      printf("%s: tile pair %u -> (%u, %u) of %u tiles\n", what, p, ti, tj, T);
      return false;
    }
    const bool diag = ti == tj;
    const uint32_t sides = diag ? 2u - 1u : 2u;
    auto pos_of = [&](uint32_t r) { return (r < kTile ? ti : tj) * kTile + (r & (kTile - 1)); };
    auto piece_of = [&](uint32_t r) -> const std::vector<uint32_t>& {
      static const std::vector<uint32_t> none;
      return pos_of(r) < m ? col.piece[pos_of(r)] : none;
    };
    uint32_t cur[2 * kTile] = {0};
    static int32_t acc[4][4][64][4];  // [wave][block of tj][lane][reg]
    memset(acc, 0, sizeof acc);
    uint32_t k0 = 0, chunks = 0;
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
        if (kc < k0 || kc % kChunk) {
          printf("%s: chunk %u after %u\n", what, kc, k0);
          return false;
        }
        k0 = kc;
        continue;
      }
      std::fill(image.begin(), image.begin() + sides * kTileBytes, 0);
      bool any[2] = {false, false};
      for (uint32_t r = 0; r < sides * kTile; ++r) {
        const auto& pc = piece_of(r);
        for (uint32_t e = cur[r]; e < pc.size() && pc[e] - k0 < kChunk; ++e) {
          image[(r < kTile ? 0 : kTileBytes) + matrix::image_offset(r & (kTile - 1), pc[e] - k0)] = 1;
          any[r / kTile] = true;
        }
      }
      if (!any[0] || (!diag && !any[1])) {
        printf("%s: chunk %u run with an empty tile\n", what, k0);
        return false;
      }
      const uint8_t* img_a = image.data();
      const uint8_t* img_b = image.data() + (diag ? 0 : kTileBytes);
      for (uint32_t wave = 0; wave < 4; ++wave)
        for (uint32_t ks = 0; ks < matrix::kKSteps; ++ks)
          for (uint32_t nb = 0; nb < 4; ++nb) mfma_16x16x64(img_a, img_b, ks, wave, nb, acc[wave][nb]);
      k0 += kChunk;
      if (++chunks > col.n_columns / kChunk + 1) {
        printf("%s: more chunks than the columns have\n", what);
        return false;
      }
    }
    // the epilogue
    for (uint32_t wave = 0; wave < 4; ++wave)
      for (uint32_t nb = 0; nb < 4; ++nb)
        for (uint32_t lane = 0; lane < 64; ++lane)
          for (uint32_t reg = 0; reg < 4; ++reg) {
            const uint32_t ra = wave * 16 + matrix::cd_row(lane, reg), rb = nb * 16 + matrix::cd_col(lane);
            const uint32_t pa = ti * kTile + ra, pb = tj * kTile + rb;
            if (!(pa < m && pb < m && (!diag || pa <= pb))) continue;
            const uint32_t ga = row_of(pa), gb = row_of(pb), la = in.lens[ga], lb = in.lens[gb];
            const uint64_t* A = in.sk.data() + (size_t)ga * s;
            const uint64_t* B = in.sk.data() + (size_t)gb * s;
            uint32_t common, total, c_ref, t_ref;
            matrix::cell_counts(pa == pb || ga == gb, A, la, la ? A[la - 1] : 0, B, lb, lb ? B[lb - 1] : 0,
                                (uint32_t)acc[wave][nb][lane][reg], &common, &total);
            validate::merge_counts(A, la, B, lb, &c_ref, &t_ref);
            ++n_cells;
            if (common != c_ref || total != t_ref) {
              printf("%s: cell (%u, %u) rows (%u, %u): (%u, %u), the merge gives (%u, %u)\n", what, pa, pb, ga, gb, common,
                     total, c_ref, t_ref);
              return false;
            }
          }
  }
  return true;
}

// rows over a shared pool: every kind of row the issue names
static Input random_input(uint32_t n, uint32_t s, uint32_t pool, bool list_rows) {
  Input in = make(n, s);
  pool = std::max(pool, s + 1);  // (a full row can be drawn)
  const uint64_t everywhere = 1 + rnd() % 1000;  // a hash in every non-empty row, for some inputs
  const bool with_everywhere = rnd_below(3) == 0;
  for (uint32_t g = 0; g < n; ++g) {
    std::set<uint64_t> h;
    const uint32_t kind = rnd_below(10);
    const uint32_t len = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? s : 1 + rnd_below(s);
    if (kind == 3 && g > 0) {  // identical to an earlier row
      const uint32_t o = rnd_below(g);
      memcpy(&in.sk[(size_t)g * s], &in.sk[(size_t)o * s], s * sizeof(uint64_t));
      in.lens[g] = in.lens[o];
      continue;
    }
    if (with_everywhere && len) h.insert(everywhere);
    while (h.size() < len) h.insert(1001 + (uint64_t)rnd_below(pool) * 0x9E3779B97F4A7C15ull);
    in.set_row(g, h);
  }
  if (list_rows) {
    in.m = 1 + rnd_below(2 * n);
    for (uint32_t a = 0; a < in.m; ++a) in.rows.push_back(rnd_below(n));  // shuffled, with repeats
  }
  return in;
}

// three rows whose column count is exactly `columns`: rows 0 and 1 share
// `columns` hashes, every row has hashes of its own, row 2 shares none
static Input exact_columns(uint32_t columns) {
  const uint32_t s = columns + 7;
  Input in = make(3, s);
  std::set<uint64_t> a, b, c;
  for (uint32_t x = 0; x < columns; ++x) {
    const uint64_t v = 10 + 3 * (uint64_t)x;
    a.insert(v);
    b.insert(v);
  }
  for (uint32_t x = 0; x < 5; ++x) {
    a.insert(11 + 3 * (uint64_t)rnd_below(columns + 50));
    b.insert(12 + 3 * (uint64_t)rnd_below(columns + 50));
    c.insert((1ull << 40) + rnd_below(1000));
  }
  in.set_row(0, a);
  in.set_row(1, b);
  in.set_row(2, c);
  return in;
}

int main() {
  uint64_t cases = 0;
  char what[96];
  // many tiny inputs: one tile pair, one chunk
  for (uint32_t it = 0; it < 3000; ++it, ++cases) {
    const uint32_t n = 1 + rnd_below(12), s = 1 + rnd_below(24);
    const Input in = random_input(n, s, 1 + rnd_below(3 * s), it & 1);
    snprintf(what, sizeof what, "tiny %u (n %u, s %u, m %u)", it, n, s, in.m);
    if (!run(in, what)) return 1;
  }
  // m on both sides of the tile edges
  for (uint32_t m : {1u, 2u, 15u, 16u, 17u, 63u, 64u, 65u, 127u, 128u, 129u, 130u})
    for (uint32_t rep = 0; rep < 3; ++rep, ++cases) {
      Input in = random_input(std::max(m, 2u), 16, 40, false);
      in.m = m;
      if (rep == 2) {  // listed in another order, one row twice
        for (uint32_t a = 0; a < m; ++a) in.rows.push_back((a * 7 + 3) % in.n);
        in.rows[m - 1] = in.rows[0];
      }
      snprintf(what, sizeof what, "tile edge m %u rep %u", m, rep);
      if (!run(in, what)) return 1;
    }
  // column counts on both sides of the chunk edges, exactly
  for (uint32_t c : {0u, 1u, 63u, 64u, 65u, 255u, 256u, 257u, 511u, 512u, 513u, 1023u, 1024u, 1025u, 1536u, 1537u}) {
    snprintf(what, sizeof what, "exact columns %u", c);
    if (!run(exact_columns(c), what, c)) return 1;
    ++cases;
  }
  // many columns and several tiles at once: chunks are skipped (sparse pool) or all run (dense pool)
  for (uint32_t it = 0; it < 12; ++it, ++cases) {
    const uint32_t n = 60 + rnd_below(80), s = 24 + rnd_below(24);
    const Input in = random_input(n, s, it & 1 ? 60 : 4000, it % 3 == 0);
    snprintf(what, sizeof what, "large %u (n %u, s %u, m %u)", it, n, s, in.m);
    if (!run(in, what)) return 1;
  }
  // two rows that share exactly one hash, in the first and the last tile, nothing else shared
  {
    Input in = make(130, 8);
    for (uint32_t g = 0; g < 130; ++g) {
      std::set<uint64_t> h;
      for (uint32_t e = 0; e < 5; ++e) h.insert(1000 + 10 * (uint64_t)g + e);
      if (g == 1 || g == 129) h.insert(7);
      in.set_row(g, h);
    }
    if (!run(in, "one shared hash across tiles", 1)) return 1;
    ++cases;
  }
  printf("ok %llu %llu\n", (unsigned long long)cases, (unsigned long long)n_cells);
  return 0;
}
