// Host test of galah_amd/csrc/query_core.hpp (no GPU, no library): the slot
// function, the probe step, the capacity rule and the best-hit key.
//
//   table   adversarial key sets inserted and found against std::unordered_map,
//           at column counts 0, 1, capacity / 2 and capacity / 2 + 1; keys that
//           were not inserted are not found; the probe visits every slot once
//           and wraps; the longest chain of every set is printed and is below
//           the capacity;
//   key     the largest best_key over a candidate list is the first of a
//           brute-force sort by (ANI descending, rank ascending), with
//           bit-equal ANI and -0.0 / 0.0.
//
// Prints "ok <cases> <keys>" as its last line.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../galah_amd/csrc/query_core.hpp"

using namespace gg;

static uint64_t n_cases = 0, n_keys = 0;

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

static std::vector<uint64_t> key_set(int kind, size_t count, std::mt19937_64& rng) {
  std::vector<uint64_t> v;
  for (size_t x = 0; v.size() < count; ++x) {
    switch (kind) {
      case 0:  // 0 and 2^64 - 1 first, then their neighbours
        v.push_back(x % 2 ? ~0ull - x / 2 : x / 2);
        break;
      case 1:  // equal in the low 32 bits
        v.push_back(((uint64_t)(x + 1) << 32) | 0xDEADBEEFull);
        break;
      case 2:  // equal in the high 32 bits
        v.push_back((0xABCDEF01ull << 32) | (x + 1));
        break;
      case 3:  // like a real bottom-s sketch: below 2^44
        v.push_back(rng() >> 20);
        break;
      default:  // consecutive small integers
        v.push_back(x + 1);
    }
  }
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}

// `count` keys of a set in a table of the capacity the rule gives -> the longest chain
static uint64_t check_table(int kind, size_t count, std::mt19937_64& rng, uint64_t slots = 0) {
  std::vector<uint64_t> keys = key_set(kind, count, rng);
  while (keys.size() < count) keys.push_back(keys.back() + 0x9E3779B97F4A7C15ull * keys.size());  // (case 3 repeats)
  keys.resize(count);
  if (!slots) slots = query::capacity(count);
  CHECK(slots >= query::kMinCapacity && (slots & (slots - 1)) == 0 && (slots >= 2 * count || slots > count));
  const uint64_t mask = slots - 1;
  std::vector<query::Slot> table(slots, query::Slot{~0ull, query::kEmpty, ~0u});  // as the 0xFF fill leaves it
  std::unordered_map<uint64_t, uint32_t> ref;
  uint64_t longest = 0;
  for (size_t c = 0; c < keys.size(); ++c) {
    const uint64_t tried = query::insert(table.data(), mask, keys[c], (uint32_t)c, query::HostClaim());
    CHECK(tried >= 1 && tried <= slots);
    ref[keys[c]] = (uint32_t)c;
  }
  CHECK(ref.size() == keys.size());
  uint64_t used = 0;
  for (const query::Slot& s : table) used += s.col != query::kEmpty;
  CHECK(used == keys.size());
  for (const auto& kv : ref) {
    uint64_t steps = 0;
    CHECK(query::find(table.data(), mask, kv.first, &steps) == kv.second);
    CHECK(steps >= 1 && steps <= slots);
    longest = std::max(longest, steps);
    ++n_keys;
  }
  // keys that are not there: the neighbours of every key, the other sets' keys, 0 and 2^64 - 1
  std::vector<uint64_t> absent = {0ull, ~0ull, 1ull, ~0ull - 1};
  for (uint64_t k : keys) {
    absent.push_back(k + 1);
    absent.push_back(k - 1);
    absent.push_back(k ^ (1ull << 63));
    absent.push_back(k ^ (1ull << 31));
  }
  for (int other = 0; other < 5; ++other)
    for (uint64_t k : key_set(other, 64, rng)) absent.push_back(k);
  for (uint64_t k : absent) {
    uint64_t steps = 0;
    const uint32_t got = query::find(table.data(), mask, k, &steps);
    const auto it = ref.find(k);
    CHECK(got == (it == ref.end() ? query::kEmpty : it->second));
    CHECK(steps <= slots);
    longest = std::max(longest, steps);
    ++n_keys;
  }
  CHECK(slots >= 2 * count ? longest < slots : longest <= slots);
  ++n_cases;
  return longest;
}

static void check_capacity_rule() {
  CHECK(query::capacity(0) == query::kMinCapacity && query::capacity(1) == query::kMinCapacity);
  for (uint64_t cap = query::kMinCapacity; cap <= (1ull << 24); cap <<= 1) {
    CHECK(query::capacity(cap / 2) == cap);          // exactly half full
    CHECK(query::capacity(cap / 2 + 1) == 2 * cap);  // one more column: the next power of two
    ++n_cases;
  }
  CHECK(query::batch_queries(1000) == query::kQueryBatch && query::batch_queries(12000) >= 1 &&
        (uint64_t)query::batch_queries(12000) * 12000 <= query::kBatchEntries && query::batch_queries(0) >= 1);
  CHECK(query::capacity((uint64_t)query::batch_queries(12000) * 12000) * sizeof(query::Slot) <= (128ull << 20));
  CHECK(sizeof(query::Slot) == 16);
}

// the probe from any slot visits every slot once, wraps, and is back after `slots` steps
static void check_probe_walk(std::mt19937_64& rng) {
  for (uint64_t slots : {query::kMinCapacity, (uint64_t)1024}) {
    const uint64_t mask = slots - 1;
    for (uint64_t h : std::vector<uint64_t>{0, ~0ull, 1, rng(), rng() >> 20}) {
      const uint64_t start = query::slot_of(h, mask);
      CHECK(start <= mask);
      std::vector<uint8_t> seen(slots, 0);
      uint64_t at = start;
      bool wrapped = false;
      for (uint64_t x = 0; x < slots; ++x) {
        CHECK(!seen[at]);
        seen[at] = 1;
        const uint64_t nx = query::next_slot(at, mask);
        wrapped |= nx < at;
        CHECK(nx == (at == mask ? 0 : at + 1));
        at = nx;
      }
      CHECK(at == start && (wrapped || start == 0));
      ++n_cases;
    }
    CHECK(query::next_slot(mask, mask) == 0);
  }
  // the probe step itself: an empty slot ends the search whatever its hash field holds
  CHECK(query::probe(query::kEmpty, 7, 7) == query::kMiss && query::probe(query::kEmpty, ~0ull, ~0ull) == query::kMiss);
  CHECK(query::probe(0, 7, 7) == query::kHit && query::probe(3, ~0ull, ~0ull) == query::kHit);
  CHECK(query::probe(0, 0, ~0ull) == query::kNext && query::probe(5, 8, 7) == query::kNext);
  // all 64 bits reach the slot: keys that differ in one bit only land apart more often than not
  uint64_t apart = 0;
  for (int b = 0; b < 64; ++b) apart += query::slot_of(0x0123456789ABCDEFull, 1023) != query::slot_of(0x0123456789ABCDEFull ^ (1ull << b), 1023);
  CHECK(apart >= 60);
}

struct Cand {
  float ani;
  uint32_t rank;
};

static void check_best_key(std::mt19937_64& rng) {
  const float pool[] = {0.0f, -0.0f, 1.0f, 0.95f, 0.9500001f, 0.94999994f, 0.5f, 1e-30f, 0.99f, -1.0f, 0.25f};
  for (int trial = 0; trial < 20000; ++trial) {
    const size_t m = 1 + rng() % 12;
    std::vector<Cand> c;
    std::vector<uint32_t> ranks;
    while (ranks.size() < m) {
      const uint32_t r = trial % 3 == 0 ? (uint32_t)(rng() % 16) : (uint32_t)rng() % 0xFFFFFFFFu;
      if (std::find(ranks.begin(), ranks.end(), r) == ranks.end()) ranks.push_back(r);
    }
    for (size_t x = 0; x < m; ++x) {
      // few distinct values: bit-equal ANI and -0.0 / 0.0 meet in most lists
      const float a = trial % 2 ? pool[rng() % (sizeof(pool) / sizeof(pool[0]))] : (float)(rng() % 4) / 4.0f;
      c.push_back(Cand{a, ranks[x]});
    }
    uint64_t best = 0;
    size_t arg = m;
    for (size_t x = 0; x < m; ++x) {
      const uint64_t k = query::best_key(c[x].ani, c[x].rank);
      CHECK(k > 0 && query::key_rank(k) == c[x].rank);
      if (k > best) {
        best = k;
        arg = x;
      }
    }
    std::vector<Cand> sorted = c;
    std::stable_sort(sorted.begin(), sorted.end(), [](const Cand& a, const Cand& b) {
      return a.ani != b.ani ? a.ani > b.ani : a.rank < b.rank;  // (-0.0 == 0.0 as values)
    });
    CHECK(arg < m && c[arg].rank == sorted[0].rank && c[arg].ani == sorted[0].ani);
    ++n_cases;
  }
  CHECK(query::best_key(0.0f, 3) == query::best_key(-0.0f, 3));
  CHECK(query::best_key(0.95f, 2) > query::best_key(0.95f, 3) && query::best_key(0.9500001f, 9) > query::best_key(0.95f, 0));
}

int main() {
  std::mt19937_64 rng(17);
  check_capacity_rule();
  check_probe_walk(rng);
  const char* names[] = {"0 and 2^64-1", "equal low 32 bits", "equal high 32 bits", "below 2^44", "small integers"};
  for (int kind = 0; kind < 5; ++kind) {
    uint64_t longest = 0;
    for (uint64_t cap : {query::kMinCapacity, (uint64_t)1024, (uint64_t)(1 << 16)})
      for (size_t count : {(size_t)0, (size_t)1, (size_t)2, (size_t)(cap / 2), (size_t)(cap / 2 + 1)})
        longest = std::max(longest, check_table(kind, count, rng));
    // past the rule: one slot left empty, a chain may run the whole table and wrap; it still ends
    const uint64_t full = check_table(kind, query::kMinCapacity - 1, rng, query::kMinCapacity);
    std::printf("%-20s longest chain %llu slots at the rule's load (%llu in a table with one empty slot of %llu)\n",
                names[kind], (unsigned long long)longest, (unsigned long long)full,
                (unsigned long long)query::kMinCapacity);
  }
  check_best_key(rng);
  std::printf("ok %llu %llu\n", (unsigned long long)n_cases, (unsigned long long)n_keys);
  return 0;
}
