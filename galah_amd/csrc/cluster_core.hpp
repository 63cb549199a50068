// The rules of the finch + finch clustering step, stated once
// for the host form (cluster.cpp), the kernels (cluster.hip) and a
// stand-alone host test (tests/cpp/test_cluster_core.cpp).
//
//   src/clusterer.rs:155-225  find_dashing_fastani_representatives with
//     skip_clusterer (:29-33, :180-185): genome i is a representative unless
//     a representative j < i has a cached pair with it and ani >= threshold
//     (f32 against f32, :212).
//   src/clusterer.rs:316-406  find_dashing_fastani_memberships: every other
//     genome joins the representative with the largest cached ani, the
//     BTreeSet walked ascending with a strict `>` (:376-399), so ties go to
//     the smallest representative.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_CLUSTER_HD __host__ __device__
#else
#define GG_CLUSTER_HD
#endif

namespace gg {
namespace cluster {

// A vertex's state.  A decision is final: it is taken from final states of
// lower vertices only, so whoever takes it, and when, takes the same one.
enum State : uint32_t { kUndecided = 0, kRep = 1, kMember = 2 };

// rep_of[] of a genome with no decision yet (never left in an output).
constexpr uint32_t kNoRep = 0xFFFFFFFFu;

// :212 -- the pair makes its higher genome a member when its lower one is a representative
GG_CLUSTER_HD inline bool strong(float ani, float threshold) { return ani >= threshold; }

// What a scan of a vertex's strong lower neighbours saw.
struct Seen {
  bool rep = false;        // one of them is a representative
  bool undecided = false;  // one of them has no decision yet
};
GG_CLUSTER_HD inline void see(Seen& s, uint32_t neighbour_state) {
  s.rep |= neighbour_state == kRep;
  s.undecided |= neighbour_state == kUndecided;
}
// The vertex's state after that scan: a member as soon as one strong lower
// neighbour is a representative, a representative once all are members.
GG_CLUSTER_HD inline uint32_t decide(const Seen& s) { return s.rep ? kMember : s.undecided ? kUndecided : kRep; }

// f32 -> u32 whose unsigned order is the order of the values (no NaN; -0.0
// and 0.0, equal as values, map to one word).  For ani >= 0 it is the bit
// pattern with the top bit set.
GG_CLUSTER_HD inline uint32_t ordered_bits(float x) {
  x += 0.0f;  // -0.0 -> 0.0
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// A member's candidate (ani to a representative, that representative): the
// largest key is the largest ani and, among equal ani, the smallest
// representative.  0 is below every key.
GG_CLUSTER_HD inline uint64_t member_key(float ani, uint32_t rep) {
  return ((uint64_t)ordered_bits(ani) << 32) | (uint64_t)(0xFFFFFFFFu - rep);
}
GG_CLUSTER_HD inline uint32_t key_rep(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

}  // namespace cluster
}  // namespace gg
