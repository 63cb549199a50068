// The shared rules of cluster validation (galah_amd/csrc/validate_core.hpp)
// on the host, without the library: the rank formula the kernel uses against
// finch's merge, the fixed-step search against a linear count, the two f32
// rules at a threshold and its neighbours, the superset threshold of the
// representative side, and the member list.  Prints "ok <checks>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../../galah_amd/csrc/validate_core.hpp"

using namespace gg::validate;

static uint64_t checks = 0;
#define CHECK(x)                                                 \
  do {                                                           \
    ++checks;                                                    \
    if (!(x)) {                                                  \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);      \
      exit(1);                                                   \
    }                                                            \
  } while (0)

// src/finch.rs:56-64 (1 - mash distance, Rust's f64::min / f64::max)
static double ani_f64(uint32_t common, uint32_t total, int k) {
  const double j = (double)common / (double)total;
  double d = -1.0 * std::log((2.0 * j) / (1.0 + j)) / (double)k;
  d = std::isnan(d) ? 1.0 : std::fmin(d, 1.0);
  d = std::fmax(d, 0.0);
  return 1.0 - d;
}

static std::vector<uint64_t> draw_row(std::mt19937_64& rng, const std::vector<uint64_t>& pool, uint32_t len) {
  std::set<uint64_t> s;
  while (s.size() < len) s.insert(pool[rng() % pool.size()]);
  return std::vector<uint64_t>(s.begin(), s.end());
}

// what the kernel computes, on one thread
static void by_rank(const std::vector<uint64_t>& A, const std::vector<uint64_t>& B, uint32_t* common, uint32_t* total) {
  *common = *total = 0;
  if (A.empty() || B.empty()) return;
  const bool a_ends = A.back() <= B.back();
  const std::vector<uint64_t>& T = a_ends ? A : B;
  const std::vector<uint64_t>& S = a_ends ? B : A;
  const uint32_t ls = (uint32_t)S.size(), hb = hibit_of(ls);
  uint32_t c = 0;
  for (uint64_t v : T) {
    const uint32_t r = rank_le(S.data(), ls, hb, v);
    c += (r && S[r - 1] == v) ? 1u : 0u;
  }
  *common = c;
  *total = total_from_rank((uint32_t)T.size(), rank_le(S.data(), ls, hb, T.back()), c);
}

int main() {
  std::mt19937_64 rng(12345);

  // rank_le against a linear count, every length up to 200 and a few large ones
  for (uint32_t len : std::vector<uint32_t>{0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200, 1000, 2047, 2048,
                                           2049, 4096, 12000}) {
    std::vector<uint64_t> S(len);
    for (uint32_t e = 0; e < len; ++e) S[e] = 10 + 3ull * e;
    const uint32_t hb = hibit_of(len);
    CHECK(len == 0 ? hb == 0 : (hb <= len && 2 * (uint64_t)hb > len && (hb & (hb - 1)) == 0));
    for (uint64_t v = 0; v < 10 + 3ull * len + 5; v += (len > 300 ? 7 : 1)) {
      uint32_t lin = 0;
      while (lin < len && S[lin] <= v) ++lin;
      CHECK(rank_le(S.data(), len, hb, v) == lin);
    }
    CHECK(rank_le(S.data(), len, hb, ~0ull) == len);
  }

  // the rank formula against the merge
  const uint32_t lens[] = {0, 1, 2, 3, 63, 64, 65, 100, 257};
  std::vector<uint64_t> pool;
  for (int i = 0; i < 600; ++i) pool.push_back(rng() | 1);
  for (int rep = 0; rep < 40; ++rep)
    for (uint32_t la : lens)
      for (uint32_t lb : lens) {
        const std::vector<uint64_t> A = draw_row(rng, pool, la), B = draw_row(rng, pool, lb);
        uint32_t c0, t0, c1, t1;
        merge_counts(A.data(), la, B.data(), lb, &c0, &t0);
        by_rank(A, B, &c1, &t1);
        CHECK(c0 == c1 && t0 == t1);
        merge_counts(B.data(), lb, A.data(), la, &c1, &t1);  // symmetric
        CHECK(c0 == c1 && t0 == t1);
        if (la == 0 || lb == 0) CHECK(c0 == 0 && t0 == 0);
        merge_counts(A.data(), la, A.data(), la, &c1, &t1);
        CHECK(c1 == la && t1 == la);
        if (la && lb) {  // equal last elements
          std::vector<uint64_t> B2 = B;
          if (B2.back() != A.back()) {
            while (!B2.empty() && B2.back() >= A.back()) B2.pop_back();
            B2.push_back(A.back());
          }
          merge_counts(A.data(), la, B2.data(), (uint32_t)B2.size(), &c0, &t0);
          by_rank(A, B2, &c1, &t1);
          CHECK(c0 == c1 && t0 == t1 && t0 == la + (uint32_t)B2.size() - c0);
        }
      }

  // the two rules: f32 against f32, equality belongs to "member ok" and "representatives bad"
  for (float thr : {0.0f, 0.5f, 0.95f, 0.98174739f, 1.0f}) {
    const float below = std::nextafterf(thr, -1.0f), above = std::nextafterf(thr, 2.0f);
    CHECK(!member_bad(thr, thr) && member_bad(below, thr) && !member_bad(above, thr));
    CHECK(reps_bad(thr, thr) && !reps_bad(below, thr) && reps_bad(above, thr));
    CHECK(superset_threshold(thr) == below || thr == 0.0f);
    CHECK(superset_threshold(thr) < thr);
  }

  // the superset threshold: whenever the f32 rule calls a pair of
  // representatives bad, the f64 test of the all-pairs path at the lowered
  // threshold keeps it -- over every (common, total) of small sketches at
  // the thresholds next to the pair's own f32, and the issue's example
  uint64_t rounded_up = 0;
  for (int k : {21, 31})
    for (uint32_t t = 1; t <= 400; ++t)
      for (uint32_t c = 0; c <= t && c <= 200; ++c) {
        const double x = ani_f64(c, t, k);
        const float a = (float)x;
        rounded_up += (double)a > x;
        for (float thr : {a, std::nextafterf(a, 2.0f), std::nextafterf(a, -1.0f), 0.95f}) {
          const bool kept = x >= (double)superset_threshold(thr);
          if (reps_bad(a, thr)) CHECK(kept);
        }
      }
  CHECK(rounded_up > 1000);  // (the case that needs the lowered threshold occurs)
  {
    const double x = ani_f64(654, 1265, 21);
    const float a = (float)x;
    CHECK((double)a > x && reps_bad(a, a) && !(x >= (double)a) && x >= (double)superset_threshold(a));
    CHECK(!reps_bad(a, std::nextafterf(a, 2.0f)));
  }

  // the member list
  {
    const uint32_t members[] = {7, 3, 9, 3, 7, 2, 5, 2, 1, 9};  // clusters {7: 3 9 3 7}, {2: 5 2 1}, {9}
    const uint32_t offsets[] = {0, 5, 9, 10};
    const std::vector<NamedPair> l = member_pairs(members, offsets, 3);
    const uint32_t exp[][2] = {{2, 1}, {2, 5}, {7, 3}, {7, 3}, {7, 9}};
    CHECK(l.size() == 5);
    for (size_t p = 0; p < l.size(); ++p) CHECK(l[p].rep == exp[p][0] && l[p].member == exp[p][1]);
    CHECK(member_pairs(members, offsets, 0).empty());
  }

  printf("ok %llu\n", (unsigned long long)checks);
  return 0;
}
