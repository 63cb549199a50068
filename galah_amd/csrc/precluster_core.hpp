// The rules of the device precluster step, stated once for
// the kernels (precluster.hip) and a stand-alone host test
// (tests/cpp/test_precluster_core.cpp): the sort keys with their bit widths,
// and the hook step of the connected components, written over a small
// atomic-operations policy so that the same function runs on HIP atomics in
// the kernel and on std::atomic in the test.
//
//   src/clusterer.rs:409-431  partition_sketches: single linkage over the
//     pairs the cache contains = the connected components of the pair graph;
//   src/clusterer.rs:45-57    each set ascending, sets by size descending
//     (ties here: by smallest member, as precluster.cpp);
//   src/sorted_pair_genome_distance_cache.rs:47-58  transform_ids: a
//     precluster's pairs keyed (min, max) by position inside it.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_PRECLUSTER_HD __host__ __device__
#else
#define GG_PRECLUSTER_HD
#endif

namespace gg {
namespace precluster {

// ceil(log2 n), at least 1: the bits of an index in [0, n), and of n itself
// when n is not a power of two.
GG_PRECLUSTER_HD inline uint32_t index_bits(uint32_t n) {
  uint32_t bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) < n) ++bits;
  return bits;
}

// ---- the set key: size descending, then root (= smallest member) ascending
GG_PRECLUSTER_HD inline uint64_t set_key(uint32_t n, uint32_t size, uint32_t root) {
  return ((uint64_t)(n - size) << 32) | root;  // 1 <= size <= n
}
GG_PRECLUSTER_HD inline uint32_t set_key_root(uint64_t key) { return (uint32_t)key; }
GG_PRECLUSTER_HD inline uint32_t set_key_size(uint32_t n, uint64_t key) { return n - (uint32_t)(key >> 32); }
// n - size is in [0, n)
GG_PRECLUSTER_HD inline uint32_t set_key_bits(uint32_t n) { return 32 + index_bits(n); }

// ---- the member key: (rank of the genome's set, genome)
GG_PRECLUSTER_HD inline uint64_t member_key(uint32_t rank, uint32_t g) { return ((uint64_t)rank << 32) | g; }
GG_PRECLUSTER_HD inline uint32_t member_key_genome(uint64_t key) { return (uint32_t)key; }
GG_PRECLUSTER_HD inline uint32_t member_key_rank(uint64_t key) { return (uint32_t)(key >> 32); }
GG_PRECLUSTER_HD inline uint32_t member_key_bits(uint32_t n_sets) { return 32 + index_bits(n_sets); }

// ---- the pair key: two positions in members[], a <= b, `bits` =
// index_bits(n) each.  A position is unique across sets, ordered by (set
// rank, position inside the set), so the order of the keys is "grouped by
// precluster, sorted by (i, j) inside it".
GG_PRECLUSTER_HD inline uint64_t pair_key(uint32_t a, uint32_t b, uint32_t bits) {
  return (bits < 32 ? (uint64_t)a << bits : (uint64_t)a << 32) | b;
}
GG_PRECLUSTER_HD inline uint32_t pair_key_a(uint64_t key, uint32_t bits) {
  return bits < 32 ? (uint32_t)(key >> bits) : (uint32_t)(key >> 32);
}
GG_PRECLUSTER_HD inline uint32_t pair_key_b(uint64_t key, uint32_t bits) {
  return bits < 32 ? (uint32_t)(key & (((uint64_t)1 << bits) - 1)) : (uint32_t)key;
}
GG_PRECLUSTER_HD inline uint32_t pair_key_bits(uint32_t n) { return 2 * index_bits(n); }
// The key of a pair that is left out (an index >= n, device form): above
// every key of two positions, which end at (n - 1, n - 1) -- one more bit,
// as position 2^bits - 1 exists when n is a power of two; at 32 bits a side
// n < 2^32 leaves the all-ones key free.
GG_PRECLUSTER_HD inline uint64_t pair_key_none(uint32_t bits) {
  return bits < 32 ? (uint64_t)1 << (2 * bits) : ~(uint64_t)0;
}
GG_PRECLUSTER_HD inline uint32_t pair_sort_bits(uint32_t n) {
  const uint32_t b = pair_key_bits(n) + 1;
  return b < 64 ? b : 64;
}
// The first key of the set whose members begin at position `first` (first =
// n: the end of the last set -- at or below pair_key_none).
GG_PRECLUSTER_HD inline uint64_t pair_key_floor(uint32_t first, uint32_t bits) { return pair_key(first, 0, bits); }

// ---- the hook step ---------------------------------------------------------
// parent[g] = g at the start.  The policy A gives three operations on
// parent[], each of which may be served from an arbitrarily stale copy except
// for what the two read-modify-writes RETURN:
//   uint32_t load(x)               some value parent[x] has held (stale is fine)
//   uint32_t fetch_min(x, v)       parent[x] = min(parent[x], v), atomically
//   uint32_t cas(x, expect, v)     atomic compare-and-swap, returns the value before
//
// Invariants (every write is one of the two atomics):
//   (1) every value ever stored in parent[x] is <= x and lies in x's tree
//       at the time of the store, and trees only ever merge;
//   (2) parent[x] never increases, so a vertex that stopped being a root
//       (parent[x] < x) never becomes one again;
//   (3) hence a stale read of parent[x] is still a vertex of x's tree no
//       greater than x: a walk over stale reads stays inside the tree,
//       strictly descends until it reads parent[r] == r, and ends;
//   (4) a failed cas on a supposed root returns its current parent, which is
//       smaller than the expected value; the retry continues from there.
// Every loop below is bounded by that descent; none waits for another thread.

// Joins the trees of u and v.  The walk steps the LARGER of the two vertices
// towards its root (shortcutting it to its grandparent on the way) until
// both are one vertex -- one tree already -- or the larger is read as a root
// and goes under the smaller with a cas.  The smaller need not be a root: it
// lies in the other tree and below the root hooked, which is all (1) asks.
// Only the larger side is walked, and only as far as needed: a path hooked in
// order costs one cas per pair and leaves a chain for the jump launches,
// where a walk to both roots would cross that chain for every pair.
// max(u, v) strictly decreases from one round to the next.  Returns the
// number of cas attempts (the tests bound it).
template <class A>
GG_PRECLUSTER_HD inline uint32_t hook(A& a, uint32_t u, uint32_t v) {
  uint32_t tries = 0;
  for (;;) {
    if (u == v) return tries;  // one vertex reached from both: one tree
    const uint32_t hi = u > v ? u : v, lo = u > v ? v : u;
    uint32_t p = a.load(hi);
    if (p == hi) {  // a root, as far as this read knows
      ++tries;
      p = a.cas(hi, hi, lo);
      if (p == hi) return tries;  // hi was a root at that instant and is under lo now
      // (4): hi's parent now, p < hi
    }
    const uint32_t gp = a.load(p);  // <= p
    if (gp != p) {
      a.fetch_min(hi, gp);  // an ancestor of hi, below what hi holds or not stored
      p = gp;
    }
    u = p;
    v = lo;
  }
}

// One pointer-jumping step of vertex x: parent[x] = parent[parent[x]].
// Returns whether it wrote.  (The flatten launches; reads of the same launch's
// writes or of older values are both ancestors of x.)
template <class A>
GG_PRECLUSTER_HD inline bool jump(A& a, uint32_t x) {
  const uint32_t p = a.load(x);
  const uint32_t gp = a.load(p);
  if (gp == p) return false;
  a.store(x, gp);
  return true;
}

// ceil(log2 n) + 1: the depth of every vertex at least halves per launch
// (x's new parent is at least two steps up, and has itself at most half its
// depth left), from at most n - 1; the last launch writes nothing.
GG_PRECLUSTER_HD inline uint32_t jump_launch_bound(uint32_t n) {
  uint32_t lg = 0;
  while (lg < 32 && ((uint64_t)1 << lg) < n) ++lg;
  return lg + 1;
}

}  // namespace precluster
}  // namespace gg
