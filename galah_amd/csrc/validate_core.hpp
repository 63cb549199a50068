// The rules of cluster validation and of the named-pair ANI behind it
// (DESIGN.md 4.6), stated once for the host forms and the kernel
// (ani_pairs.hip) and a stand-alone host test (tests/cpp/test_validate_core.cpp).
//
//   src/finch.rs:57            finch::distance::distance(a, b): the merge of two
//     ascending sketches until either is exhausted -> (common, total).
//   src/cluster_validation.rs:21-45  every member against its cluster's
//     representative: ok iff ani >= threshold.
//   src/cluster_validation.rs:47-77  every pair of representatives: ok iff
//     ani < threshold.
// Both comparisons are f32 against f32: the pair's value is the one galah
// stores, gg_ani_f32(common, total, k), and the threshold the caller's f32.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_VALIDATE_HD __host__ __device__
#else
#define GG_VALIDATE_HD
#endif

namespace gg {
namespace validate {

// finch's merge, literally: rows ascending without repeats.  An empty row
// gives (0, 0).
inline void merge_counts(const uint64_t* A, uint32_t la, const uint64_t* B, uint32_t lb, uint32_t* common,
                         uint32_t* total) {
  uint32_t i = 0, j = 0, c = 0;
  while (i < la && j < lb) {
    const uint64_t va = A[i], vb = B[j];
    if (va < vb) {
      ++i;
    } else if (vb < va) {
      ++j;
    } else {
      ++i;
      ++j;
      ++c;
    }
  }
  *common = c;
  *total = i + j - c;
}

// The same total without the merge.  The row whose last element is the
// smaller (T, len_t entries) is exhausted first, so every element of it is
// visited, and of the other row (S) those <= last T, rank_s of them:
//   total = |T| + #{s in S : s <= last T} - common.
// With equal last elements both rows end together and either is T.
GG_VALIDATE_HD inline uint32_t total_from_rank(uint32_t len_t, uint32_t rank_s, uint32_t common) {
  return len_t + rank_s - common;
}

// #{e < len : S[e] <= v}, S ascending: a fixed number of steps for a given
// len (hibit = the largest power of two <= len, 0 for len == 0).
GG_VALIDATE_HD inline uint32_t hibit_of(uint32_t len) { return len ? 1u << (31 - __builtin_clz(len)) : 0u; }
template <typename Ptr>
GG_VALIDATE_HD inline uint32_t rank_le(Ptr S, uint32_t len, uint32_t hibit, uint64_t v) {
  uint32_t pos = 0;
  for (uint32_t st = hibit; st; st >>= 1) {
    const uint32_t p = pos + st;
    if (p <= len && S[p - 1] <= v) pos = p;
  }
  return pos;
}

// :28-35 -- a member whose value to its representative is below the threshold
GG_VALIDATE_HD inline bool member_bad(float pair_ani, float threshold) { return pair_ani < threshold; }
// :56-66 -- two representatives at or above it
GG_VALIDATE_HD inline bool reps_bad(float pair_ani, float threshold) { return pair_ani >= threshold; }

// The all-pairs path keeps a pair iff its f64 value >= (double)min_ani, the
// rule above is on the f32.  Rounding to f32 is monotone and the f32
// predecessor p of the threshold is itself an f32, so an f64 below p rounds
// to at most p: every pair reps_bad() holds for has its f64 >= p.  The pair
// path run at p returns a superset, filtered by reps_bad().
inline float superset_threshold(float threshold) { return std::nextafterf(threshold, -INFINITY); }

struct NamedPair {
  uint32_t rep, member;
};
// The member side's named pairs: for every cluster (CSR, representative
// first) every listed genome other than the representative, once per listing,
// in (rep, member) order.  The reference also compares the representative
// with itself (:23); that pair is not made.
inline std::vector<NamedPair> member_pairs(const uint32_t* members, const uint32_t* offsets, uint32_t n_clusters) {
  std::vector<NamedPair> out;
  for (uint32_t c = 0; c < n_clusters; ++c) {
    const uint32_t rep = members[offsets[c]];
    for (uint32_t x = offsets[c] + 1; x < offsets[c + 1]; ++x)
      if (members[x] != rep) out.push_back(NamedPair{rep, members[x]});
  }
  // counting sorts would do; the list is N long and the pair work dwarfs it
  struct Less {
    bool operator()(const NamedPair& a, const NamedPair& b) const {
      return a.rep != b.rep ? a.rep < b.rep : a.member < b.member;
    }
  };
  std::stable_sort(out.begin(), out.end(), Less());
  return out;
}

}  // namespace validate
}  // namespace gg
