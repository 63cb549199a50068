// The rules of the query of a resident collection, stated
// once for the kernels (query.hip), the host runtime (query.cpp) and a
// stand-alone host test (tests/cpp/test_query_core.cpp).
//
//   table     the distinct hashes of one batch of queries (the columns) in an
//             open-addressing table: slot -> (hash, column id).  An empty slot
//             is marked by its column id, never by a hash: any u64 is a legal
//             hash (0 and 2^64 - 1 included).  All 64 bits of the hash are
//             mixed into the slot: real bottom-s hashes have their high bits
//             zero, the test sketches only their low bits set.  Linear probing
//             wraps; the capacity is a power of two >= 2 x columns, so a probe
//             always ends at an empty slot.
//   best hit  a query's best candidate is cluster_core.hpp's member_key(ani,
//             rank) maximised: the largest f32 ANI, ties to the smallest rank
//             (src/clusterer.rs:376-399).
#pragma once

#include <cstdint>

#include "cluster_core.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_QUERY_HD __host__ __device__
#else
#define GG_QUERY_HD
#endif

namespace gg {
namespace query {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;         // column id of an empty slot
constexpr uint32_t kNoHit = 0xFFFFFFFFu;         // best[q].i of a query no candidate hit
constexpr uint32_t kNotCandidate = 0xFFFFFFFFu;  // rank of a row that is no candidate

// Queries per launch of the stream kernel: its per-wave LDS counters are u16,
// direct-indexed by the query's number in the batch (4 B of LDS per query and
// wave: counter and touched-list entry).
constexpr uint32_t kQueryBatch = 2048;
// ... and no more queries than keep a batch's entries at or below this, so
// that the table (16 B a slot, <= 2^23 slots) stays in the Infinity Cache.
constexpr uint64_t kBatchEntries = 1ull << 22;
constexpr uint64_t kMinCapacity = 64;

struct alignas(16) Slot {
  uint64_t hash;
  uint32_t col;  // kEmpty: nothing here (hash is then not read)
  uint32_t pad;
};

GG_QUERY_HD inline uint32_t batch_queries(uint32_t sketch_size) {
  const uint64_t by_entries = kBatchEntries / (sketch_size ? sketch_size : 1);
  return by_entries < 1 ? 1u : by_entries > kQueryBatch ? kQueryBatch : (uint32_t)by_entries;
}

// The capacity rule: a power of two >= 2 x columns, at least kMinCapacity.
GG_QUERY_HD inline uint64_t capacity(uint64_t columns) {
  uint64_t cap = kMinCapacity;
  while (cap < 2 * columns) cap <<= 1;
  return cap;
}

// The slot function: murmur3's 64-bit finaliser (a bijection of u64 in which
// every input bit reaches every output bit), then the table's mask.
GG_QUERY_HD inline uint64_t mix(uint64_t h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}
GG_QUERY_HD inline uint64_t slot_of(uint64_t hash, uint64_t mask) { return mix(hash) & mask; }
GG_QUERY_HD inline uint64_t next_slot(uint64_t slot, uint64_t mask) { return (slot + 1) & mask; }

// The probe step on what a slot holds: the search of `hash` ends without a
// column, ends with the slot's column, or goes on at next_slot().
enum Probe : uint32_t { kMiss = 0, kHit = 1, kNext = 2 };
GG_QUERY_HD inline Probe probe(uint32_t slot_col, uint64_t slot_hash, uint64_t hash) {
  return slot_col == kEmpty ? kMiss : slot_hash == hash ? kHit : kNext;
}

// The column of `hash` (kEmpty: none); *steps (may be null) the slots read.
GG_QUERY_HD inline uint32_t find(const Slot* table, uint64_t mask, uint64_t hash, uint64_t* steps = nullptr) {
  uint64_t slot = slot_of(hash, mask), n = 0;
  for (;;) {
    const Slot s = table[slot];
    ++n;
    const Probe p = probe(s.col, s.hash, hash);
    if (p != kNext) {
      if (steps) *steps = n;
      return p == kHit ? s.col : kEmpty;
    }
    slot = next_slot(slot, mask);
  }
}

// Column `col` of a hash that is not in the table yet, into the first empty
// slot of its probe chain.  claim(&slot.col, col) takes an empty slot (true)
// or finds it taken: a plain test on the host, an atomicCAS in the kernel.
// The hash is written after the claim; an inserter never reads another
// slot's hash, and the finders run after the build.  Returns the slots tried.
template <typename Claim>
GG_QUERY_HD inline uint64_t insert(Slot* table, uint64_t mask, uint64_t hash, uint32_t col, const Claim& claim) {
  uint64_t slot = slot_of(hash, mask), n = 1;
  while (!claim(&table[slot].col, col)) {
    slot = next_slot(slot, mask);
    ++n;
  }
  table[slot].hash = hash;
  return n;
}
struct HostClaim {
  bool operator()(uint32_t* at, uint32_t col) const {
    if (*at != kEmpty) return false;
    *at = col;
    return true;
  }
};

// The best-hit key: the largest is the largest f32 ANI and, among equal ANI,
// the smallest rank.  0 is below every key.
GG_QUERY_HD inline uint64_t best_key(float ani, uint32_t rank) { return cluster::member_key(ani, rank); }
GG_QUERY_HD inline uint32_t key_rank(uint64_t key) { return cluster::key_rep(key); }

}  // namespace query
}  // namespace gg
