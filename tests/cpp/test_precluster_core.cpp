// The rules of the device precluster step (galah_amd/csrc/precluster_core.hpp)
// on the host, without a device:
//   - the hook step on 8 std::threads over each case file's pairs (the order
//     of the file, dealt round-robin), then the jump rounds, against a plain
//     union-find: the same sets, every vertex at its set's smallest member,
//     the rounds within the bound;
//   - hand-made and generated stale-read schedules of the hook step: a walk
//     is fed older values of parent[] and must converge to the same sets;
//   - the set key and the pair key: round trip, order and width at n = 2,
//     65,536, 65,537 and 2^32 - 1.
// A case file: u32 n, u64 m, then m x (u32 i, u32 j).  Prints "ok <cases>".
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <numeric>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "../../galah_amd/csrc/precluster_core.hpp"

namespace pc = gg::precluster;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

using Pairs = std::vector<std::pair<uint32_t, uint32_t>>;

// the policy over std::atomic: what the kernel does with HIP atomics
struct StdParents {
  std::atomic<uint32_t>* parent;
  uint32_t load(uint32_t x) const { return parent[x].load(std::memory_order_relaxed); }
  void store(uint32_t x, uint32_t v) const { parent[x].store(v, std::memory_order_relaxed); }
  uint32_t fetch_min(uint32_t x, uint32_t v) const {
    uint32_t cur = parent[x].load(std::memory_order_relaxed);
    while (v < cur && !parent[x].compare_exchange_weak(cur, v, std::memory_order_relaxed)) {
    }
    return cur;
  }
  uint32_t cas(uint32_t x, uint32_t expect, uint32_t v) const {
    parent[x].compare_exchange_strong(expect, v, std::memory_order_relaxed);
    return expect;
  }
};

// A single-threaded policy whose loads are stale: every value parent[x] has
// held is kept, and load(x) answers with one of them, chosen by `pick`
// (history size -> index; 0 is the oldest, x itself).  The two
// read-modify-writes act on the newest value, as an atomic does.  Checks
// invariants (1) and (2) at every write.
struct StaleParents {
  std::vector<std::vector<uint32_t>>* hist;
  uint32_t (*pick)(uint32_t size, uint64_t* state);
  uint64_t* state;
  uint64_t* loads;
  uint32_t load(uint32_t x) const {
    ++*loads;
    const auto& h = (*hist)[x];
    return h[pick((uint32_t)h.size(), state)];
  }
  void write(uint32_t x, uint32_t v) const {
    CHECK(v <= x && v <= (*hist)[x].back());
    if (v != (*hist)[x].back()) (*hist)[x].push_back(v);
  }
  uint32_t fetch_min(uint32_t x, uint32_t v) const {
    const uint32_t cur = (*hist)[x].back();
    if (v < cur) write(x, v);
    return cur;
  }
  uint32_t cas(uint32_t x, uint32_t expect, uint32_t v) const {
    const uint32_t cur = (*hist)[x].back();
    if (cur == expect) write(x, v);
    return cur;
  }
};

uint32_t pick_oldest(uint32_t, uint64_t*) { return 0; }
uint32_t pick_one_behind(uint32_t size, uint64_t*) { return size >= 2 ? size - 2 : 0; }
uint32_t pick_random(uint32_t size, uint64_t* s) {
  *s = *s * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((*s >> 33) % size);
}
// fresh and oldest in turn
uint32_t pick_alternate(uint32_t size, uint64_t* s) { return (++*s & 1) ? size - 1 : 0; }

// the smallest member of every vertex's set, by a plain union-find
std::vector<uint32_t> smallest_members(uint32_t n, const Pairs& pairs) {
  std::vector<uint32_t> p(n);
  std::iota(p.begin(), p.end(), 0u);
  auto find = [&](uint32_t x) {
    while (p[x] != x) x = p[x] = p[p[x]];
    return x;
  };
  for (auto& e : pairs) {
    const uint32_t a = find(e.first), b = find(e.second);
    if (a != b) p[std::max(a, b)] = std::min(a, b);
  }
  std::vector<uint32_t> out(n);
  for (uint32_t g = 0; g < n; ++g) out[g] = find(g);  // (roots are the smallest: larger goes under smaller)
  return out;
}

// the jump rounds (sequential sweeps, each reading what the sweep already wrote)
template <class A>
uint32_t flatten(A& a, uint32_t n) {
  uint32_t rounds = 0;
  for (;;) {
    bool changed = false;
    for (uint32_t x = 0; x < n; ++x) changed |= pc::jump(a, x);
    ++rounds;
    CHECK(rounds <= pc::jump_launch_bound(n));
    if (!changed) return rounds;
  }
}

void threaded_case(uint32_t n, const Pairs& pairs) {
  std::unique_ptr<std::atomic<uint32_t>[]> parent(new std::atomic<uint32_t>[std::max(n, 1u)]);
  for (uint32_t g = 0; g < n; ++g) parent[g].store(g);
  constexpr unsigned T = 8;
  std::vector<std::thread> th;
  std::atomic<uint64_t> tries{0};
  for (unsigned t = 0; t < T; ++t)
    th.emplace_back([&, t] {
      StdParents a{parent.get()};
      uint64_t mine = 0;
      for (size_t p = t; p < pairs.size(); p += T) mine += pc::hook(a, pairs[p].first, pairs[p].second);
      tries += mine;
    });
  for (auto& t : th) t.join();
  // a pair costs one cas when nobody interferes; each retry follows another thread's success
  CHECK(tries.load() <= 2 * (uint64_t)pairs.size() + (uint64_t)T * n);
  // after the hooks alone: parent[x] <= x, and x's root is its set's smallest member
  const std::vector<uint32_t> want = smallest_members(n, pairs);
  for (uint32_t g = 0; g < n; ++g) CHECK(parent[g].load() <= g);
  StdParents a{parent.get()};
  if (n) flatten(a, n);
  for (uint32_t g = 0; g < n; ++g) CHECK(parent[g].load() == want[g]);
}

void stale_case(uint32_t n, const Pairs& pairs, uint32_t (*pick)(uint32_t, uint64_t*)) {
  std::vector<std::vector<uint32_t>> hist(n);
  for (uint32_t g = 0; g < n; ++g) hist[g].push_back(g);
  uint64_t state = 12345, loads = 0, tries = 0;
  StaleParents a{&hist, pick, &state, &loads};
  for (auto& e : pairs) tries += pc::hook(a, e.first, e.second);
  // every retry follows a failed cas, which moved the walk strictly down
  CHECK(tries <= (uint64_t)pairs.size() * (uint64_t)std::max(n, 1u));
  const std::vector<uint32_t> want = smallest_members(n, pairs);
  // the newest values, jumped to the roots with fresh reads
  std::unique_ptr<std::atomic<uint32_t>[]> parent(new std::atomic<uint32_t>[std::max(n, 1u)]);
  for (uint32_t g = 0; g < n; ++g) parent[g].store(hist[g].back());
  StdParents f{parent.get()};
  if (n) flatten(f, n);
  for (uint32_t g = 0; g < n; ++g) CHECK(parent[g].load() == want[g]);
}

// Hand-made schedules: the reads of one walk are scripted.
struct ScriptedParents {
  std::vector<uint32_t>* parent;
  std::map<uint32_t, std::vector<uint32_t>>* script;  // x -> answers of the next loads of x, then fresh
  uint32_t load(uint32_t x) const {
    auto it = script->find(x);
    if (it != script->end() && !it->second.empty()) {
      const uint32_t v = it->second.front();
      it->second.erase(it->second.begin());
      return v;
    }
    return (*parent)[x];
  }
  void store(uint32_t x, uint32_t v) const { (*parent)[x] = v; }
  uint32_t fetch_min(uint32_t x, uint32_t v) const {
    const uint32_t cur = (*parent)[x];
    (*parent)[x] = std::min(cur, v);
    return cur;
  }
  uint32_t cas(uint32_t x, uint32_t expect, uint32_t v) const {
    const uint32_t cur = (*parent)[x];
    if (cur == expect) (*parent)[x] = v;
    return cur;
  }
};

void hand_made_schedules() {
  // 1. a stale root: 3 -> 2 -> 1 exists, but the walk from 3 is told 3 is
  //    still a root.  cas(3, 3, 0) fails with 2, 3 is shortcut to 1, and the
  //    hook goes on from 1.
  {
    std::vector<uint32_t> parent = {0, 1, 1, 2};
    std::map<uint32_t, std::vector<uint32_t>> script = {{3, {3}}};
    ScriptedParents a{&parent, &script};
    const uint32_t tries = pc::hook(a, 3, 0);
    CHECK(tries == 2 && parent[1] == 0 && parent[3] <= 2 && parent[2] == 1);
    flatten(a, 4);
    CHECK((parent == std::vector<uint32_t>{0, 0, 0, 0}));
  }
  // 2. a stale middle: 5 -> 4 -> 2 -> 0, the walk from 5 reads parent[4] as
  //    4 (its first value), twice: 4 is taken for a root and hooked under 3;
  //    the cas fails with 2, 4 is shortcut to 0, and the walk ends at 0 <- 1.
  {
    std::vector<uint32_t> parent = {0, 1, 0, 1, 2, 4};
    std::map<uint32_t, std::vector<uint32_t>> script = {{4, {4, 4}}};
    ScriptedParents a{&parent, &script};
    CHECK(pc::hook(a, 5, 3) == 2 && parent[4] == 0 && parent[1] == 0);
    flatten(a, 6);
    CHECK((parent == std::vector<uint32_t>{0, 0, 0, 0, 0, 0}));
  }
  // 3. both walks stale, and the same vertex reached from both: (4, 3) with
  //    4 -> 2 and 3 -> 2 already there; 2's own parent is read as 2 although
  //    it is 0 by now.  u == v == 2: nothing to do, and nothing is undone.
  {
    std::vector<uint32_t> parent = {0, 1, 0, 2, 2};
    std::map<uint32_t, std::vector<uint32_t>> script = {{2, {2, 2}}};
    ScriptedParents a{&parent, &script};
    CHECK(pc::hook(a, 4, 3) == 0);
    CHECK((parent == std::vector<uint32_t>{0, 1, 0, 2, 2}));
  }
  // 4. two stale roots in a row: 4 -> 3 -> 2 -> 0; the walk from 4 reads
  //    parent[3] as 3's first value 3 (so 3 looks like a root) and hooks 3
  //    under 1: fails with 2; parent[2] is read as the old value 2 as well,
  //    that cas fails with 0, and the walk ends hooking 1 under 0.
  {
    std::vector<uint32_t> parent = {0, 1, 0, 2, 3};
    std::map<uint32_t, std::vector<uint32_t>> script = {{3, {3, 3}}, {2, {2, 2}}};
    ScriptedParents a{&parent, &script};
    const uint32_t tries = pc::hook(a, 4, 1);
    CHECK(tries == 3);
    for (uint32_t g = 0; g < 5; ++g) CHECK(parent[g] <= g);
    flatten(a, 5);
    CHECK((parent == std::vector<uint32_t>{0, 0, 0, 0, 0}));
  }
  // 5. an old grandparent in a shortcut: 3 -> 2 -> 0, and parent[2] is read
  //    as its older value 1 (1 -> 0).  The shortcut stores min(2, 1) = 1 in
  //    parent[3]: an ancestor still, and never above what was there.
  {
    std::vector<uint32_t> parent = {0, 0, 0, 2};
    std::map<uint32_t, std::vector<uint32_t>> script = {{2, {1}}};
    ScriptedParents a{&parent, &script};
    CHECK(pc::hook(a, 3, 0) == 0);
    CHECK((parent == std::vector<uint32_t>{0, 0, 0, 1}));
  }
}

void key_checks() {
  const uint32_t ns[] = {2u, 65536u, 65537u, 0xFFFFFFFFu};
  const uint32_t want_bits[] = {1, 16, 17, 32};
  std::mt19937_64 rng(7);
  for (int c = 0; c < 4; ++c) {
    const uint32_t n = ns[c], bits = pc::index_bits(n);
    CHECK(bits == want_bits[c]);
    CHECK(pc::set_key_bits(n) == 32 + bits && pc::pair_key_bits(n) == 2 * bits);
    CHECK(pc::pair_sort_bits(n) == std::min(64u, 2 * bits + 1));
    auto index = [&] { return (uint32_t)(rng() % n); };
    // the corners, then random values
    std::vector<uint32_t> vals = {0, n - 1, n / 2, (uint32_t)((1ull << (bits - 1)) % n)};
    for (int r = 0; r < 200; ++r) vals.push_back(index());
    struct S { uint32_t size, root; uint64_t key; };
    std::vector<S> sets;
    for (uint32_t root : vals)
      for (uint32_t sz : vals) {
        const uint32_t size = sz + 1;  // 1 .. n
        const uint64_t key = pc::set_key(n, size, root);
        CHECK(pc::set_key_root(key) == root && pc::set_key_size(n, key) == size);
        CHECK(pc::set_key_bits(n) == 64 || (key >> pc::set_key_bits(n)) == 0);
        sets.push_back({size, root, key});
      }
    for (size_t x = 0; x + 1 < sets.size(); ++x) {
      const S &p = sets[x], &q = sets[sets.size() - 1 - x];
      const bool before = p.size != q.size ? p.size > q.size : p.root < q.root;  // size descending, root ascending
      CHECK(before == (p.key < q.key));
    }
    struct P { uint32_t a, b; uint64_t key; };
    std::vector<P> ps;
    const uint64_t none = pc::pair_key_none(bits);
    CHECK(pc::pair_sort_bits(n) == 64 || (none >> pc::pair_sort_bits(n)) == 0);
    CHECK(pc::pair_key_floor(n, bits) <= none || bits == 32);
    for (uint32_t x : vals)
      for (uint32_t y : vals) {
        const uint32_t a = std::min(x, y), b = std::max(x, y);
        const uint64_t key = pc::pair_key(a, b, bits);
        CHECK(pc::pair_key_a(key, bits) == a && pc::pair_key_b(key, bits) == b);
        CHECK(key < none && (bits == 32 || (key >> pc::pair_key_bits(n)) == 0));
        CHECK(pc::pair_key_floor(a, bits) <= key && (a == n - 1 || key < pc::pair_key_floor(a + 1, bits)));
        ps.push_back({a, b, key});
      }
    for (size_t x = 0; x + 1 < ps.size(); ++x) {
      const P &p = ps[x], &q = ps[ps.size() - 1 - x];
      CHECK((std::make_pair(p.a, p.b) < std::make_pair(q.a, q.b)) == (p.key < q.key));
    }
    CHECK(pc::member_key_rank(pc::member_key(n - 1, n - 2)) == n - 1);
    CHECK(pc::member_key_genome(pc::member_key(n - 1, n - 2)) == n - 2);
    CHECK(pc::member_key(1, 0) > pc::member_key(0, n - 1));
  }
  CHECK(pc::jump_launch_bound(1) == 1 && pc::jump_launch_bound(2) == 2 && pc::jump_launch_bound(20000) == 16 &&
        pc::jump_launch_bound(65536) == 17 && pc::jump_launch_bound(65537) == 18);
}

bool read_case(const char* path, uint32_t* n, Pairs* pairs) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint64_t m = 0;
  bool ok = fread(n, 4, 1, f) == 1 && fread(&m, 8, 1, f) == 1;
  std::vector<uint32_t> raw(2 * m);
  ok = ok && (m == 0 || fread(raw.data(), 8, m, f) == m);
  fclose(f);
  pairs->clear();
  for (uint64_t p = 0; ok && p < m; ++p) {
    if (raw[2 * p] >= *n || raw[2 * p + 1] >= *n) return false;
    pairs->emplace_back(raw[2 * p], raw[2 * p + 1]);
  }
  return ok;
}

int main(int argc, char** argv) {
  key_checks();
  hand_made_schedules();
  int cases = 0;
  for (int k = 1; k < argc; ++k) {
    uint32_t n = 0;
    Pairs pairs;
    if (!read_case(argv[k], &n, &pairs)) {
      fprintf(stderr, "cannot read case %s\n", argv[k]);
      return 1;
    }
    threaded_case(n, pairs);
    if (pairs.size() <= 100000) {  // (the stale policies keep every value: the smaller cases)
      stale_case(n, pairs, pick_oldest);
      stale_case(n, pairs, pick_one_behind);
      stale_case(n, pairs, pick_random);
      stale_case(n, pairs, pick_alternate);
    }
    ++cases;
  }
  printf("ok %d\n", cases);
  return 0;
}
