// The grouped rules of the dense ANI matrix (galah_amd/csrc/matrix_core.hpp,
// "groups") driven on the host, stand-alone:
//   - the grouped column rule (columns, entries in them, every position's
//     group-local piece, every group's first id) against a
//     std::map<(group, hash), positions>;
//   - workgroup -> (group, ti, tj): for random size vectors in which the sizes
//     0, 1, 63, 64, 65 and 200 are all present, every workgroup lands in a
//     group of two positions or more, and every tile pair of every such group
//     is reached exactly once, in group order;
//   - cell_off against the running sum of m^2, and the three limits;
//   - the tiled product walked as the kernel walks it (group-local tiles,
//     cursors, chunk jumps, byte images, fragments, the C/D map; the matrix
//     instruction emulated from its definition) with every cell of every
//     block equal to validate::merge_counts, the single cell of a group of
//     one by the diagonal rule.
//
// Prints "ok <cases> <cells> <workgroups>" and returns 0, or the first mismatch and 1.
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

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
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
  std::vector<uint32_t> lens, members, offsets;  // offsets: n_groups + 1
  uint32_t groups() const { return (uint32_t)offsets.size() - 1; }
};

// one 16 x 16 x 64 step from its definition (test_matrix_core.cpp)
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

static uint64_t n_cells = 0, n_workgroups = 0;

static bool run(const Input& in, const char* what) {
  const uint32_t s = in.s, G = in.groups(), P = in.offsets[G];
  const uint32_t* mem = in.members.data();
  const uint32_t* off = in.offsets.data();
  const matrix::GroupColumns col = matrix::columns_host(in.sk.data(), in.lens.data(), s, mem, off, G);

  // ---- the grouped column rule against a map: (group, hash) -> positions holding it
  std::map<std::pair<uint32_t, uint64_t>, std::vector<uint32_t>> held;
  uint64_t entries = 0;
  for (uint32_t g = 0; g < G; ++g)
    for (uint32_t p = off[g]; p < off[g + 1]; ++p) {
      if (matrix::group_of_position(off, G, p) != g) {
        printf("%s: position %u is not found in group %u\n", what, p, g);
        return false;
      }
      for (uint32_t e = 0; e < in.lens[mem[p]]; ++e, ++entries) held[{g, in.sk[(size_t)mem[p] * s + e]}].push_back(p);
    }
  std::vector<std::vector<uint32_t>> piece(P);
  std::vector<uint32_t> first_id(G, 0), local(G, 0);
  uint64_t n_columns = 0, column_entries = 0;
  for (const auto& kv : held) {  // (the map ascends with (group, hash))
    if (kv.second.size() < 2) continue;
    const uint32_t g = kv.first.first;
    for (uint32_t p : kv.second) piece[p].push_back(local[g]);
    ++local[g];
    ++n_columns;
    column_entries += kv.second.size();
  }
  for (uint32_t g = 1; g < G; ++g) first_id[g] = first_id[g - 1] + local[g - 1];
  if (col.n_entries != entries || col.n_columns != n_columns || col.column_entries != column_entries ||
      col.piece != piece || col.first_id != first_id) {
    printf("%s: column rule: entries %llu/%llu columns %llu/%llu column entries %llu/%llu pieces %s first ids %s\n", what,
           (unsigned long long)col.n_entries, (unsigned long long)entries, (unsigned long long)col.n_columns,
           (unsigned long long)n_columns, (unsigned long long)col.column_entries, (unsigned long long)column_entries,
           col.piece == piece ? "equal" : "differ", col.first_id == first_id ? "equal" : "differ");
    return false;
  }

  // ---- the layout: cells and workgroups
  std::vector<uint64_t> cell_off(G + 1);
  std::vector<uint32_t> tp_off(G + 1);
  if (!matrix::group_layout(off, G, s, cell_off.data(), tp_off.data())) {
    printf("%s: the layout is refused\n", what);
    return false;
  }
  uint64_t cells = 0, pairs = 0;
  for (uint32_t g = 0; g <= G; ++g) {
    if (cell_off[g] != cells || tp_off[g] != pairs) {
      printf("%s: group %u begins at cell %llu / workgroup %u, expected %llu / %llu\n", what, g,
             (unsigned long long)cell_off[g], tp_off[g], (unsigned long long)cells, (unsigned long long)pairs);
      return false;
    }
    if (g == G) break;
    const uint64_t m = off[g + 1] - off[g];
    cells += m * m;
    if (m >= 2) pairs += (uint64_t)((m + 63) / 64) * ((m + 63) / 64 + 1) / 2;
  }

  // ---- every cell, written once (or twice by the mirror): 0 unwritten, 1 written
  std::vector<uint8_t> written(cells, 0);
  auto check_cell = [&](uint64_t cell, uint32_t ga, uint32_t gb, uint32_t common, uint32_t total) {
    uint32_t c_ref, t_ref;
    validate::merge_counts(in.sk.data() + (size_t)ga * s, in.lens[ga], in.sk.data() + (size_t)gb * s, in.lens[gb], &c_ref,
                           &t_ref);
    ++n_cells;
    written[cell] = 1;
    if (common != c_ref || total != t_ref) {
      printf("%s: cell %llu rows (%u, %u): (%u, %u), the merge gives (%u, %u)\n", what, (unsigned long long)cell, ga, gb,
             common, total, c_ref, t_ref);
      return false;
    }
    return true;
  };
  // groups of one: the diagonal rule
  for (uint32_t g = 0; g < G; ++g)
    if (off[g + 1] - off[g] == 1) {
      const uint32_t row = mem[off[g]], len = in.lens[row];
      if (!check_cell(cell_off[g], row, row, len, len)) return false;
    }

  // ---- the tiled product, workgroup by workgroup
  std::vector<uint8_t> image(2 * kTileBytes);
  uint32_t last_g = 0, last_p = 0;
  bool first = true;
  for (uint32_t w = 0; w < tp_off[G]; ++w, ++n_workgroups) {
    const uint32_t g = matrix::group_of_workgroup(tp_off.data(), G, w);
    const uint32_t p0 = off[g], m = off[g + 1] - p0, T = matrix::tiles_of(m), p = w - tp_off[g];
    uint32_t ti, tj;
    matrix::tile_pair_of(p, &ti, &tj);
    const bool in_order = first || (g == last_g ? p == last_p + 1 : g > last_g && p == 0);
    if (g >= G || m < 2 || !(tp_off[g] <= w && w < tp_off[g + 1]) || !(ti <= tj && tj < T) || !in_order) {
      printf("%s: workgroup %u -> group %u (m %u) tile pair %u (%u, %u) of %u tiles\n", what, w, g, m, p, ti, tj, T);
      return false;
    }
    first = false;
    last_g = g;
    last_p = p;
    const bool diag = ti == tj;
    const uint32_t sides = diag ? 1u : 2u;
    auto pos_of = [&](uint32_t r) { return (r < kTile ? ti : tj) * kTile + (r & (kTile - 1)); };  // local to the group
    auto piece_of = [&](uint32_t r) -> const std::vector<uint32_t>& {
      static const std::vector<uint32_t> none;
      return pos_of(r) < m ? col.piece[p0 + pos_of(r)] : none;
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
      // the chunk loop sees the group's columns only: never more chunks than they fill
      if (++chunks > local[g] / kChunk + 1) {
        printf("%s: group %u of %u columns ran %u chunks\n", what, g, local[g], chunks);
        return false;
      }
    }
    for (uint32_t wave = 0; wave < 4; ++wave)
      for (uint32_t nb = 0; nb < 4; ++nb)
        for (uint32_t lane = 0; lane < 64; ++lane)
          for (uint32_t reg = 0; reg < 4; ++reg) {
            const uint32_t ra = wave * 16 + matrix::cd_row(lane, reg), rb = nb * 16 + matrix::cd_col(lane);
            const uint32_t pa = ti * kTile + ra, pb = tj * kTile + rb;
            if (!(pa < m && pb < m && (!diag || pa <= pb))) continue;
            const uint32_t ga = mem[p0 + pa], gb = mem[p0 + pb], la = in.lens[ga], lb = in.lens[gb];
            const uint64_t* A = in.sk.data() + (size_t)ga * s;
            const uint64_t* B = in.sk.data() + (size_t)gb * s;
            uint32_t common, total;
            matrix::cell_counts(pa == pb || ga == gb, A, la, la ? A[la - 1] : 0, B, lb, lb ? B[lb - 1] : 0,
                                (uint32_t)acc[wave][nb][lane][reg], &common, &total);
            if (!check_cell(cell_off[g] + (uint64_t)pa * m + pb, ga, gb, common, total)) return false;
            if (!check_cell(cell_off[g] + (uint64_t)pb * m + pa, gb, ga, common, total)) return false;
          }
  }
  for (uint64_t c = 0; c < cells; ++c)
    if (!written[c]) {
      printf("%s: cell %llu of %llu is never written\n", what, (unsigned long long)c, (unsigned long long)cells);
      return false;
    }
  return true;
}

// n rows over a shared pool (empty, length-1, full, identical and random rows), grouped by `sizes`:
// members drawn at random, so a row is listed twice in a group and in several groups
static Input random_input(uint32_t n, uint32_t s, uint32_t pool, const std::vector<uint32_t>& sizes) {
  Input in;
  in.n = n;
  in.s = s;
  in.sk.assign((size_t)n * s, 0);
  in.lens.assign(n, 0);
  pool = std::max(pool, s + 1);
  const uint64_t everywhere = 1 + rnd() % 1000;
  const bool with_everywhere = rnd_below(3) == 0;
  for (uint32_t g = 0; g < n; ++g) {
    const uint32_t kind = rnd_below(10);
    const uint32_t len = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? s : 1 + rnd_below(s);
    if (kind == 3 && g > 0) {
      const uint32_t o = rnd_below(g);
      memcpy(&in.sk[(size_t)g * s], &in.sk[(size_t)o * s], s * sizeof(uint64_t));
      in.lens[g] = in.lens[o];
      continue;
    }
    std::set<uint64_t> h;
    if (with_everywhere && len) h.insert(everywhere);
    while (h.size() < len) h.insert(1001 + (uint64_t)rnd_below(pool) * 0x9E3779B97F4A7C15ull);
    uint32_t e = 0;
    for (uint64_t v : h) in.sk[(size_t)g * s + e++] = v;
    in.lens[g] = e;
  }
  in.offsets.push_back(0);
  for (uint32_t m : sizes) {
    for (uint32_t a = 0; a < m; ++a) in.members.push_back(rnd_below(n));
    in.offsets.push_back((uint32_t)in.members.size());
  }
  if (in.members.empty()) in.members.push_back(0);  // (data() of an empty vector)
  return in;
}

// group g holds two rows sharing exactly columns[g] hashes -- the same hashes
// in every group -- and a third row sharing none
static Input exact_columns(const std::vector<uint32_t>& columns) {
  uint32_t most = 0;
  for (uint32_t c : columns) most = std::max(most, c);
  Input in;
  in.s = most + 5;
  in.n = 3 * (uint32_t)columns.size();
  in.sk.assign((size_t)in.n * in.s, 0);
  in.lens.assign(in.n, 0);
  in.offsets.push_back(0);
  for (uint32_t g = 0; g < columns.size(); ++g) {
    for (uint32_t r = 0; r < 3; ++r) {
      std::set<uint64_t> h;
      if (r < 2)
        for (uint32_t x = 0; x < columns[g]; ++x) h.insert(10 + 3 * (uint64_t)x);
      for (uint32_t x = 0; x < 4; ++x) h.insert((1ull << 40) * (r + 1) + 3 * (uint64_t)rnd_below(1000) + 1 + g % 2);
      const uint32_t row = 3 * g + r;
      uint32_t e = 0;
      for (uint64_t v : h) in.sk[(size_t)row * in.s + e++] = v;
      in.lens[row] = e;
      in.members.push_back(row);
    }
    in.offsets.push_back((uint32_t)in.members.size());
  }
  return in;
}

int main() {
  uint64_t cases = 0;
  char what[96];
  // many tiny inputs: a few small groups
  for (uint32_t it = 0; it < 2000; ++it, ++cases) {
    const uint32_t n = 1 + rnd_below(12), s = 1 + rnd_below(24);
    std::vector<uint32_t> sizes(rnd_below(7));
    for (uint32_t& m : sizes) m = rnd_below(6);
    const Input in = random_input(n, s, 1 + rnd_below(3 * s), sizes);
    snprintf(what, sizeof what, "tiny %u (n %u, s %u, %zu groups)", it, n, s, sizes.size());
    if (!run(in, what)) return 1;
  }
  // size vectors with 0, 1, 63, 64, 65 and 200 present, in a random order among random sizes
  for (uint32_t it = 0; it < 10; ++it, ++cases) {
    std::vector<uint32_t> sizes = {0, 1, 63, 64, 65, 200};
    for (uint32_t x = rnd_below(8); x > 0; --x) sizes.push_back(rnd_below(3) ? rnd_below(4) : rnd_below(140));
    for (size_t i = sizes.size() - 1; i > 0; --i) std::swap(sizes[i], sizes[rnd_below((uint32_t)i + 1)]);
    const Input in = random_input(40 + rnd_below(60), 12, it & 1 ? 30 : 2000, sizes);
    snprintf(what, sizeof what, "sizes %u (%zu groups, %u positions)", it, sizes.size(), in.offsets.back());
    if (!run(in, what)) return 1;
  }
  // the same hashes in several groups; column counts on both sides of the chunk edges after a first group of 7
  {
    const Input in = exact_columns({7, 0, 511, 512, 513, 1025});
    if (!run(in, "exact columns")) return 1;
    const matrix::GroupColumns col = matrix::columns_host(in.sk.data(), in.lens.data(), in.s, in.members.data(),
                                                          in.offsets.data(), in.groups());
    if (col.n_columns != 7 + 0 + 511 + 512 + 513 + 1025 || col.first_id != std::vector<uint32_t>{0, 7, 7, 518, 1030, 1543}) {
      printf("exact columns: %llu columns\n", (unsigned long long)col.n_columns);
      return 1;
    }
    ++cases;
  }
  // the limits, each alone
  {
    const uint64_t big = 1ull << 31;
    bool ok = matrix::group_limits_ok(big / 1000 - 1, 1000, 0, 0) && !matrix::group_limits_ok(big / 1000 + 1, 1000, 0, 0) &&
              matrix::group_limits_ok(1, 1, 2 * big - 1, 0) && !matrix::group_limits_ok(1, 1, 2 * big, 0) &&
              matrix::group_limits_ok(1, 1, 0, big - 1) && !matrix::group_limits_ok(1, 1, 0, big);
    const uint32_t one_group[2] = {0, 65536}, under[2] = {0, 65535}, two[3] = {0, 46341, 92682};
    uint64_t cell_off[3];
    ok = ok && !matrix::group_layout(one_group, 1, 1, cell_off, nullptr) && matrix::group_layout(under, 1, 1, cell_off, nullptr) &&
         cell_off[1] == 65535ull * 65535ull && !matrix::group_layout(two, 2, 1, cell_off, nullptr) &&
         !matrix::group_layout(under, 1, 1u << 16, nullptr, nullptr);
    if (!ok) {
      printf("limits\n");
      return 1;
    }
    ++cases;
  }
  printf("ok %llu %llu %llu\n", (unsigned long long)cases, (unsigned long long)n_cells, (unsigned long long)n_workgroups);
  return 0;
}
