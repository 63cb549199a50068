// galah_amd/csrc/cluster_core.hpp on the host: the decision rule and the
// membership key that gg_cluster_pairs_host and the kernels of cluster.hip
// share.  Host only; run by tests/test_cluster_core.py.
//   - decide(): member as soon as a strong lower neighbour is a representative,
//     representative once all are members, undecided otherwise -- whatever the
//     order the neighbours are seen in;
//   - strong(): ani >= threshold in f32, equality included, NaN never;
//   - member_key(): key order == (ANI descending, representative ascending)
//     on random values (ties, +-0, denormals, negatives and infinities
//     included), key_rep() gives the representative back, 0 is below every key;
//   - a small greedy run driven by the rules alone (0 - 1 - 2 strong,
//     ani(1,2) > ani(0,1): representatives 0 and 2, 1 joins 2).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../galah_amd/csrc/cluster_core.hpp"

using namespace gg::cluster;

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

static float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, sizeof f);
  return f;
}

int main() {
  // decide(): every multiset of neighbour states up to 4, in every order
  const uint32_t states[3] = {kUndecided, kRep, kMember};
  for (int len = 0; len <= 4; ++len) {
    int total = 1;
    for (int x = 0; x < len; ++x) total *= 3;
    for (int code = 0; code < total; ++code) {
      Seen s;
      bool any_rep = false, any_und = false;
      for (int x = 0, c = code; x < len; ++x, c /= 3) {
        see(s, states[c % 3]);
        any_rep |= states[c % 3] == kRep;
        any_und |= states[c % 3] == kUndecided;
      }
      const uint32_t want = any_rep ? kMember : any_und ? kUndecided : kRep;
      CHECK(decide(s) == want);
    }
  }
  CHECK(decide(Seen{}) == kRep);  // no strong lower neighbour

  // strong()
  const float t = 0.95f, nan = std::numeric_limits<float>::quiet_NaN();
  CHECK(strong(t, t) && strong(std::nextafter(t, 1.0f), t) && !strong(std::nextafter(t, 0.0f), t));
  CHECK(!strong(nan, t) && !strong(t, nan));

  // member_key(): order on random values
  std::mt19937_64 rng(12345);
  const float pool[] = {0.0f, -0.0f, 0.9f, 0.95f, 0.9808188f, 1.0f, std::nextafter(0.95f, 1.0f), 1e-45f, -1e-45f,
                        -0.5f, std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
  auto random_ani = [&]() -> float {
    switch (rng() % 4) {
      case 0:
        return pool[rng() % (sizeof pool / sizeof pool[0])];
      case 1:
        return (float)((rng() % 1000) / 1000.0);  // ties are common
      default: {
        float f;
        do f = from_bits((uint32_t)rng());
        while (std::isnan(f));
        return f;
      }
    }
  };
  unsigned long checked = 0;
  for (int it = 0; it < 1000000; ++it) {
    const float a = random_ani(), b = rng() % 8 ? random_ani() : a;
    const uint32_t ra = (uint32_t)rng() >> (rng() % 32), rb = rng() % 8 ? (uint32_t)rng() >> (rng() % 32) : ra;
    const uint64_t ka = member_key(a, ra), kb = member_key(b, rb);
    // the reference's scan (src/clusterer.rs:376-399): ascending representatives, strict `>`:
    // a beats b iff ani_a > ani_b, or they are equal and a's representative is smaller
    const bool a_wins = a > b || (a == b && ra < rb);
    const bool b_wins = b > a || (a == b && rb < ra);
    CHECK((ka > kb) == a_wins);
    CHECK((kb > ka) == b_wins);
    CHECK((ka == kb) == (a == b && ra == rb));
    CHECK(key_rep(ka) == ra && key_rep(kb) == rb);
    CHECK(ka != 0 && kb != 0);  // (0 is below every key)
    ++checked;
  }
  // ani >= 0: the key's high word is the bit pattern with the top bit set
  for (float a : {0.0f, 0.5f, 0.9808188f, 1.0f}) {
    uint32_t bits;
    std::memcpy(&bits, &a, sizeof bits);
    CHECK((uint32_t)(member_key(a, 7) >> 32) == (bits | 0x80000000u));
  }

  // the three-genome case by the rules alone
  {
    const float ani01 = 0.96f, ani12 = 0.97f, T = 0.95f;
    uint32_t st[3] = {kUndecided, kUndecided, kUndecided};
    Seen s0;
    st[0] = decide(s0);
    Seen s1;
    if (strong(ani01, T)) see(s1, st[0]);
    st[1] = decide(s1);
    Seen s2;
    if (strong(ani12, T)) see(s2, st[1]);
    st[2] = decide(s2);
    CHECK(st[0] == kRep && st[1] == kMember && st[2] == kRep);
    const uint64_t best = std::max(member_key(ani01, 0), member_key(ani12, 2));
    CHECK(key_rep(best) == 2);
  }

  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok %lu\n", checked);
  return 0;
}
