// The pair form of the matrix product (galah_amd/csrc/matrix_core.hpp, "the
// pair form") driven on the host, stand-alone.  The tiled incidence product is
// walked through the core's own index arithmetic as the kernel walks it (tile
// pairs, cursors, chunk jumps, byte images, fragments, the C/D map; the matrix
// instruction emulated from its definition), then the pair epilogue's rule
// decides what a tile pair emits: the early exit, the cells visited, the
// candidate test, the pass test and the emitted record.
//
// The reference is validate::merge_counts and the pass test over all pairs of
// positions.  Inputs are random -- empty rows, identical rows, a row listed
// twice, m on both sides of the tile edges -- under random cmin tables,
// non-monotone ones and cmin[0] == 0 included, with sufmin and zero_passes
// derived as the library derives them.  Beyond the equality of the emitted and
// the reference lists it asserts that the candidate test never drops a passing
// pair and that the early exit is taken only where nothing can pass.
//
// Prints "ok <cases> <pairs>" and returns 0, or the first mismatch and 1.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "../../galah_amd/csrc/matrix_core.hpp"

using namespace gg;
using matrix::kChunk;
using matrix::kNoColumn;
using matrix::kTile;
using matrix::kTileBytes;

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }

struct Input {
  uint32_t n = 0, s = 0, m = 0;
  std::vector<uint64_t> sk;
  std::vector<uint32_t> lens;
  std::vector<uint32_t> rows;  // empty: positions are rows 0 .. m-1
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
static uint64_t n_pairs = 0, n_early = 0, n_rejected = 0;

static bool run(const Input& in, const Tables& T, const char* what) {
  const uint32_t m = in.m, s = in.s;
  const uint32_t* rows = in.rows.empty() ? nullptr : in.rows.data();
  auto row_of = [&](uint32_t a) { return rows ? rows[a] : a; };
  if (!matrix::pair_limits_ok(m, s)) {
    printf("%s: limits\n", what);
    return false;
  }
  const matrix::Columns col = matrix::columns_host(in.sk.data(), in.lens.data(), s, rows, m);

  // ---- the reference: the merge and the pass test over all pairs of positions
  std::vector<Rec> want;
  for (uint32_t pa = 0; pa < m; ++pa)
    for (uint32_t pb = pa + 1; pb < m; ++pb) {
      const uint32_t ga = row_of(pa), gb = row_of(pb);
      if (ga == gb) continue;  // the same row listed twice: nothing
      uint32_t c, t;
      validate::merge_counts(in.sk.data() + (size_t)ga * s, in.lens[ga], in.sk.data() + (size_t)gb * s, in.lens[gb], &c,
                             &t);
      if (t <= T.tmax && c >= T.cmin[t]) want.push_back(Rec{std::min(ga, gb), std::max(ga, gb), c, t});
    }

  // ---- the tiled product and the pair epilogue, as the kernel walks them
  std::vector<Rec> got;
  const uint32_t NT = matrix::tiles_of(m), P = matrix::tile_pairs_of(NT);
  std::vector<uint8_t> image(2 * kTileBytes);
  for (uint32_t p = 0; p < P; ++p) {
    uint32_t ti, tj;
    matrix::tile_pair_of(p, &ti, &tj);
    const bool diag = ti == tj;
    const uint32_t sides = diag ? 1u : 2u;
    auto pos_of = [&](uint32_t r) { return (r < kTile ? ti : tj) * kTile + (r & (kTile - 1)); };
    auto piece_of = [&](uint32_t r) -> const std::vector<uint32_t>& {
      static const std::vector<uint32_t> none;
      return pos_of(r) < m ? col.piece[pos_of(r)] : none;
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

    // what the merge lets pass inside this tile pair, for the two assertions
    const bool early = matrix::pair_early_exit(ran, T.zero_passes);
    uint32_t staged = 0;
    for (uint32_t wave = 0; wave < 4; ++wave)
      for (uint32_t nb = 0; nb < 4; ++nb)
        for (uint32_t lane = 0; lane < 64; ++lane)
          for (uint32_t reg = 0; reg < 4; ++reg) {
            const uint32_t ra = wave * 16 + matrix::cd_row(lane, reg), rb = nb * 16 + matrix::cd_col(lane);
            const uint32_t pa = ti * kTile + ra, pb = tj * kTile + rb;
            if (!(pa < m && pb < m)) continue;
            const uint32_t ga = row_of(pa), gb = row_of(pb), la = in.lens[ga], lb = in.lens[gb];
            if (!matrix::pair_visited(pa, pb, ga, gb)) continue;
            const uint64_t* A = in.sk.data() + (size_t)ga * s;
            const uint64_t* B = in.sk.data() + (size_t)gb * s;
            uint32_t c_ref, t_ref;
            validate::merge_counts(A, la, B, lb, &c_ref, &t_ref);
            const bool ref_pass = t_ref <= T.tmax && c_ref >= T.cmin[t_ref];
            if (early) {  // the kernel returns before the epilogue: nothing of the tile pair may pass
              if (ref_pass) {
                printf("%s: early exit of tile pair (%u, %u), yet (%u, %u) passes with (%u, %u)\n", what, ti, tj, pa, pb,
                       c_ref, t_ref);
                return false;
              }
              continue;
            }
            const uint32_t common_ab = (uint32_t)acc[wave][nb][lane][reg];
            const bool cand = matrix::pair_candidate(la, lb, common_ab, T.cmin.data(), T.sufmin.data());
            if (ref_pass && !cand) {
              printf("%s: the candidate test drops (%u, %u): common %u, (%u, %u) passes\n", what, pa, pb, common_ab, c_ref,
                     t_ref);
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
  in.n = in.m = n;
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

// The limits at their boundaries, and the workgroup numbering at the largest
// tile pairs and across the launches' slices.
static bool limits_and_slices() {
  const uint64_t most = 65535ull * kTile;  // 65,535 tiles: 2^31 - 32,768 tile pairs
  bool ok = matrix::pair_limits_ok(most, 1) && matrix::pair_limits_ok(most, 512) && !matrix::pair_limits_ok(most, 513) &&
            !matrix::pair_limits_ok(most + 1, 1) && matrix::pair_limits_ok(2147483, 1000) &&
            !matrix::pair_limits_ok(2147484, 1000);
  const uint32_t P = matrix::tile_pairs_of(65535);
  ok = ok && P == 2147450880u && matrix::kPairSlice * 256ull < (1ull << 32);
  uint64_t launched = 0;  // the slices cover [0, P) once, each launch under 2^32 threads
  for (uint32_t base = 0; base < P; base += std::min(matrix::kPairSlice, P - base)) {
    const uint32_t grid = std::min(matrix::kPairSlice, P - base);
    ok = ok && base == launched && grid * 256ull < (1ull << 32);
    launched += grid;
    for (uint32_t w : {0u, grid / 2, grid - 1}) {  // tile_pair_of inverts p = tj (tj + 1) / 2 + ti
      uint32_t ti, tj;
      matrix::tile_pair_of(base + w, &ti, &tj);
      ok = ok && ti <= tj && tj < 65535 && (uint64_t)tj * (tj + 1) / 2 + ti == base + w;
    }
  }
  return ok && launched == P;
}

int main() {
  uint64_t cases = 0;
  char what[112];
  if (!limits_and_slices()) {
    printf("limits and slices\n");
    return 1;
  }
  // many tiny inputs under every kind of table: one tile pair, one chunk
  for (uint32_t it = 0; it < 3000; ++it, ++cases) {
    const uint32_t n = 1 + rnd_below(12), s = 1 + rnd_below(24), kind = it % 5;
    Input in = random_input(n, s, 1 + rnd_below(3 * s));
    if (it & 1) {  // listed in any order, with repeats
      in.m = 1 + rnd_below(2 * n);
      for (uint32_t a = 0; a < in.m; ++a) in.rows.push_back(rnd_below(n));
    }
    snprintf(what, sizeof what, "tiny %u (n %u, s %u, m %u, table %u)", it, n, s, in.m, kind);
    if (!run(in, make_tables(s, kind), what)) return 1;
  }
  // m on both sides of the tile edges; dense and sparse pools (chunks all run, or skipped and tile pairs left early)
  for (uint32_t m : {1u, 2u, 63u, 64u, 65u, 130u})
    for (uint32_t rep = 0; rep < 10; ++rep, ++cases) {
      const uint32_t s = 16, kind = rep % 5;
      Input in = random_input(std::max(m, 2u), s, rep < 5 ? 40 : 6000);
      in.m = m;
      if (rep % 2 == 1) {  // another order, one row listed twice
        for (uint32_t a = 0; a < m; ++a) in.rows.push_back((a * 7 + 3) % in.n);
        in.rows[m - 1] = in.rows[0];
      }
      snprintf(what, sizeof what, "tile edge m %u rep %u table %u", m, rep, kind);
      if (!run(in, make_tables(s, kind), what)) return 1;
    }
  // two tiles apart: rows that share hashes only across the first and the last tile, the rest unrelated,
  // so most tile pairs take the early exit
  for (uint32_t kind = 0; kind < 5; ++kind, ++cases) {
    Input in;
    in.n = in.m = 130;
    in.s = 8;
    in.sk.assign((size_t)in.n * in.s, 0);
    in.lens.assign(in.n, 0);
    for (uint32_t g = 0; g < in.n; ++g) {
      std::set<uint64_t> h;
      for (uint32_t e = 0; e < 5; ++e) h.insert(1000 + 10 * (uint64_t)g + e);
      if (g == 1 || g == 129) h.insert({7, 8, 9});
      if (g == 70) h.clear();  // an empty row
      uint32_t e = 0;
      for (uint64_t v : h) in.sk[(size_t)g * in.s + e++] = v;
      in.lens[g] = e;
    }
    snprintf(what, sizeof what, "shared across tiles, table %u", kind);
    if (!run(in, make_tables(in.s, kind), what)) return 1;
  }
  if (n_early == 0 || n_rejected == 0 || n_pairs == 0) {
    printf("coverage: %llu early exits, %llu cells rejected as candidates, %llu pairs\n", (unsigned long long)n_early,
           (unsigned long long)n_rejected, (unsigned long long)n_pairs);
    return 1;
  }
  printf("ok %llu %llu\n", (unsigned long long)cases, (unsigned long long)n_pairs);
  return 0;
}
