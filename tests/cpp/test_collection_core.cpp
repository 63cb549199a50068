// Host test of galah_amd/csrc/collection_core.hpp: the merge
// positions, the survivor / relabel rule and the batch plan of the row
// compaction, on random and edge lists, against std::sort / std::remove_if.
// Stand-alone (its own main); tests/test_collection_core.py builds it plainly
// and with the address and undefined-behaviour sanitizers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../../galah_amd/csrc/collection_core.hpp"

namespace co = gg::collection;

struct Pair {
  uint32_t i, j, common, total;
  bool operator==(const Pair& o) const { return i == o.i && j == o.j && common == o.common && total == o.total; }
};
static bool by_ij(const Pair& a, const Pair& b) { return a.i != b.i ? a.i < b.i : a.j < b.j; }

static uint64_t n_cases = 0, n_pairs = 0;

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

// `count` distinct pairs i < j < n, each kept by `want(i, j)`, in (i, j) order
template <class Want>
static std::vector<Pair> random_pairs(std::mt19937_64& rng, uint32_t n, uint32_t count, Want want) {
  std::set<std::pair<uint32_t, uint32_t>> seen;
  std::vector<Pair> out;
  if (n < 2) return out;
  for (uint32_t t = 0; t < 4 * count && out.size() < count; ++t) {
    uint32_t a = (uint32_t)(rng() % n), b = (uint32_t)(rng() % n);
    if (a == b) continue;
    if (a > b) std::swap(a, b);
    if (!want(a, b) || !seen.insert({a, b}).second) continue;
    out.push_back(Pair{a, b, (uint32_t)(rng() % 1000), (uint32_t)(rng() % 2000)});
  }
  std::sort(out.begin(), out.end(), by_ij);
  return out;
}

// ---- the merge -------------------------------------------------------------------
static void check_merge(const std::vector<Pair>& all, uint32_t n, uint32_t n_old) {
  std::vector<Pair> old_list, border;
  for (const Pair& p : all) (p.j < n_old ? old_list : border).push_back(p);
  const uint32_t no = (uint32_t)old_list.size(), nb = (uint32_t)border.size();
  std::vector<uint32_t> old_start(n + 1), border_start(n + 1);
  for (uint32_t r = 0; r <= n; ++r) {
    old_start[r] = co::row_boundary(old_list.data(), no, r);
    border_start[r] = co::row_boundary(border.data(), nb, r);
    // against the definition
    CHECK(old_start[r] == (uint32_t)(std::lower_bound(old_list.begin(), old_list.end(), Pair{r, 0, 0, 0}, by_ij) - old_list.begin()));
    CHECK(border_start[r] == (uint32_t)(std::lower_bound(border.begin(), border.end(), Pair{r, 0, 0, 0}, by_ij) - border.begin()));
  }
  const Pair none{co::kNone, co::kNone, 0, 0};
  std::vector<Pair> out(all.size(), none);
  for (uint32_t p = 0; p < no; ++p) {
    const uint32_t at = co::merged_old(p, old_list[p].i, border_start.data());
    CHECK(at < out.size() && out[at] == none);  // in range, written once
    out[at] = old_list[p];
  }
  for (uint32_t q = 0; q < nb; ++q) {
    const uint32_t at = co::merged_border(q, border[q].i, old_start.data());
    CHECK(at < out.size() && out[at] == none);
    out[at] = border[q];
  }
  std::vector<Pair> ref = old_list;
  ref.insert(ref.end(), border.begin(), border.end());
  std::sort(ref.begin(), ref.end(), by_ij);
  CHECK(ref == all && out == ref);
  ++n_cases;
  n_pairs += all.size();
}

static void merge_cases(std::mt19937_64& rng) {
  auto any = [](uint32_t, uint32_t) { return true; };
  for (uint32_t n : {0u, 1u, 2u, 3u, 17u, 64u, 200u}) {
    for (uint32_t density : {0u, 1u, 3u, 40u}) {
      const std::vector<Pair> all = random_pairs(rng, n, n * density, any);
      for (uint32_t n_old : {0u, 1u, n / 3, n / 2, n > 0 ? n - 1 : 0, n})
        if (n_old <= n) check_merge(all, n, n_old);  // n_old = 0: an empty old list; n_old = n: an empty border
    }
  }
  const uint32_t n = 120, n_old = 80;
  // rows with only old pairs, rows with only border pairs
  check_merge(random_pairs(rng, n, 900, [&](uint32_t i, uint32_t j) { return i % 2 ? j < n_old : j >= n_old; }), n, n_old);
  // border pairs with both ends new, and nothing else
  check_merge(random_pairs(rng, n, 300, [&](uint32_t i, uint32_t) { return i >= n_old; }), n, n_old);
  // old pairs only in the last old row's neighbourhood, a border in every row
  check_merge(random_pairs(rng, n, 900, [&](uint32_t i, uint32_t j) { return j >= n_old || i + 2 >= j; }), n, n_old);
  // every pair
  std::vector<Pair> full;
  for (uint32_t i = 0; i < 40; ++i)
    for (uint32_t j = i + 1; j < 40; ++j) full.push_back(Pair{i, j, i, j});
  for (uint32_t k = 0; k <= 40; ++k) check_merge(full, 40, k);
}

// ---- removal: the pair list and the rows ----------------------------------------
static void check_remove(std::mt19937_64& rng, uint32_t n, const std::vector<uint8_t>& keep, uint32_t rows_per_batch) {
  std::vector<uint32_t> below(n + 1), new_index(std::max(n, 1u));
  const uint32_t first = co::relabel_rows(keep.data(), n, below.data(), new_index.data());
  // new_index against std::remove_if over the row numbers
  std::vector<uint32_t> rows(n);
  for (uint32_t r = 0; r < n; ++r) rows[r] = r;
  std::vector<uint32_t> left = rows;
  left.erase(std::remove_if(left.begin(), left.end(), [&](uint32_t r) { return !keep[r]; }), left.end());
  CHECK(below[n] == left.size());
  for (uint32_t x = 0; x < left.size(); ++x) CHECK(new_index[left[x]] == x);
  for (uint32_t r = 0; r < n; ++r) {
    CHECK(keep[r] || new_index[r] == co::kNone);
    CHECK(below[r] <= r);
    CHECK(r < first ? (keep[r] && new_index[r] == r) : true);
  }
  CHECK(first == n || !keep[first]);

  // the pair list: flags, exclusive scan, scatter (the device's three steps)
  const std::vector<Pair> all = random_pairs(rng, n, n * 6, [](uint32_t, uint32_t) { return true; });
  std::vector<uint32_t> flags(all.size() + 1, 0), at(all.size() + 1, 0);
  for (size_t p = 0; p < all.size(); ++p) flags[p] = co::pair_survives(new_index.data(), all[p].i, all[p].j);
  for (size_t p = 0; p < all.size(); ++p) at[p + 1] = at[p] + flags[p];
  std::vector<Pair> out(at[all.size()]);
  for (size_t p = 0; p < all.size(); ++p)
    if (flags[p]) out[at[p]] = Pair{new_index[all[p].i], new_index[all[p].j], all[p].common, all[p].total};
  std::vector<Pair> ref = all;
  ref.erase(std::remove_if(ref.begin(), ref.end(), [&](const Pair& p) { return !keep[p.i] || !keep[p.j]; }), ref.end());
  for (Pair& p : ref) {
    p.i = (uint32_t)(std::lower_bound(left.begin(), left.end(), p.i) - left.begin());
    p.j = (uint32_t)(std::lower_bound(left.begin(), left.end(), p.j) - left.begin());
  }
  CHECK(out == ref);
  for (size_t p = 1; p < out.size(); ++p) CHECK(by_ij(out[p - 1], out[p]));  // still strictly ascending: no sort needed
  for (const Pair& p : out) CHECK(p.i < p.j && p.j < below[n]);

  // the rows: batches through a bounce buffer, in place
  std::vector<uint32_t> matrix = rows;        // matrix[r] = the row stored at r
  std::vector<uint8_t> unread(n, 1);          // source rows no batch has gathered yet
  const uint32_t nb = co::batch_count(first, n, rows_per_batch);
  CHECK(first < n ? nb >= 1 : nb == 0);
  uint32_t next_src = first;
  for (uint32_t b = 0; b < nb; ++b) {
    const co::Batch x = co::batch_of(b, first, n, rows_per_batch, below.data());
    CHECK(x.src0 == next_src && x.src1 > x.src0 && x.src1 <= n && x.src1 - x.src0 <= rows_per_batch);
    next_src = x.src1;
    CHECK(x.dst0 >= first && x.dst1 - x.dst0 <= x.src1 - x.src0);
    std::vector<uint32_t> bounce(x.dst1 - x.dst0, co::kNone);
    for (uint32_t r = x.src0; r < x.src1; ++r) {
      CHECK(unread[r]);
      unread[r] = 0;
      if (new_index[r] == co::kNone) continue;
      const uint32_t slot = new_index[r] - x.dst0;
      CHECK(slot < bounce.size() && bounce[slot] == co::kNone);
      bounce[slot] = matrix[r];
    }
    // the destinations never reach a source that is yet to be read
    CHECK(x.dst1 <= x.src1);
    for (uint32_t d = x.dst0; d < x.dst1; ++d) {
      CHECK(!unread[d]);
      CHECK(bounce[d - x.dst0] != co::kNone);
      matrix[d] = bounce[d - x.dst0];
    }
  }
  CHECK(nb == 0 || next_src == n);
  for (uint32_t x = 0; x < left.size(); ++x) CHECK(matrix[x] == left[x]);
  ++n_cases;
  n_pairs += all.size();
}

static void remove_cases(std::mt19937_64& rng) {
  for (uint32_t n : {0u, 1u, 2u, 5u, 64u, 65u, 300u}) {
    for (uint32_t batch : {1u, 7u, 64u, 1000u}) {
      std::vector<uint8_t> keep(n, 1);
      check_remove(rng, n, keep, batch);  // nothing
      std::fill(keep.begin(), keep.end(), 0);
      check_remove(rng, n, keep, batch);  // everything
      if (n == 0) continue;
      std::fill(keep.begin(), keep.end(), 1);
      keep[0] = 0;
      check_remove(rng, n, keep, batch);  // row 0
      std::fill(keep.begin(), keep.end(), 1);
      keep[n - 1] = 0;
      check_remove(rng, n, keep, batch);  // the last row
      if (n >= 64) {  // a stretch longer than a batch, kept rows on both sides
        std::fill(keep.begin(), keep.end(), 1);
        for (uint32_t r = 10; r < 10 + std::min(n - 20, 3 * batch + 1); ++r) keep[r] = 0;
        check_remove(rng, n, keep, batch);
      }
      for (uint32_t percent : {1u, 10u, 50u, 90u}) {
        for (uint32_t r = 0; r < n; ++r) keep[r] = rng() % 100 >= percent;
        check_remove(rng, n, keep, batch);
      }
    }
  }
}

static void sizing_cases() {
  CHECK(co::batch_rows(64ull << 20, 1000) == (64ull << 20) / 8004);
  CHECK(co::batch_rows(64ull << 20, 12000) >= 1);
  CHECK(co::batch_rows(16, 12000) == 1);  // at least one row
  CHECK(co::batch_count(5, 5, 7) == 0 && co::batch_count(0, 1, 7) == 1 && co::batch_count(3, 17, 7) == 2 &&
        co::batch_count(3, 18, 7) == 3);
  CHECK(co::grown(0, 5) == 5 && co::grown(4, 5) == 8 && co::grown(4, 100) == 100 && co::grown(1, 2) == 2);
  ++n_cases;
}

int main() {
  std::mt19937_64 rng(20240607);
  merge_cases(rng);
  remove_cases(rng);
  sizing_cases();
  printf("ok %llu %llu\n", (unsigned long long)n_cases, (unsigned long long)n_pairs);
  return 0;
}
