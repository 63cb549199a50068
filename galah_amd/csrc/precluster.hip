// The precluster step on the device: from the pair list of
// distances() to the preclusters (members / offsets, precluster.cpp's order)
// and every precluster's pairs renumbered by position (transform_ids), by the
// rules of precluster_core.hpp.  Single linkage over a sparse pair list is
// connected components:
//
//   1. hook: parent[g] = g, then one launch over the pairs.  A pair walks the
//      larger of its two vertices towards its root until that root goes under
//      the smaller vertex with an agent-scope compare-and-swap, or both walks
//      meet (precluster_core.hpp's hook).  EVERY write to parent[] in this
//      launch is an agent-scope atomic (cas for a hook, min for a shortcut
//      inside the walk); there is no plain store.  Invariants:
//        - every value ever stored in parent[x] is <= x and lies in x's tree,
//          and trees only merge;
//        - parent[x] never increases: a vertex that stopped being a root
//          never becomes one again;
//        - so a stale read (a CU's L1 is never refreshed inside a launch, the
//          per-XCD L2s are not coherent) is still a valid ancestor, and a
//          walk over stale reads strictly descends and ends;
//        - a failed cas returns the current value, smaller than the expected
//          one, and the retry continues from that value.
//      Every loop is bounded by that descent.  No thread waits for another to
//      act: no grid barrier, no spin on a flag, no cooperative launch.
//      Correctness rests on the return values of the atomics only, never on a
//      load being fresh (the loads bypass L1 merely to save retries).
//   2. flatten: pointer-jumping launches, parent[x] = parent[parent[x]] (up
//      to four times per vertex and launch), each setting one "changed" word
//      the host reads back.  A launch in which
//      nobody wrote saw only values of earlier launches, so a 0 word means
//      every vertex points at its root -- its set's smallest member.  The
//      depth at least halves per launch: at most ceil(log2 n) + 1 launches
//      (the hook launch leaves a chain as deep as n for a path hooked in
//      order, which is why no per-vertex walk to the root stands here).
//   3. sets in order: sizes counted per root, the roots compacted with the
//      key ((n - size) << 32) | root and radix-sorted: a set's rank; a scan
//      of the sizes in rank order: offsets.
//   4. members: the genomes sorted by (rank << 32) | g; inv[g] = g's position.
//   5. local pairs: a position in members[] is unique across sets and ordered
//      by (set rank, position inside the set), so ONE stable sort of the
//      pairs by (min(inv[i], inv[j]), max(...)) with src as the payload gives
//      "grouped by precluster, sorted by (i, j) inside it", duplicates in
//      ascending src.  pair_offsets: n_sets + 1 lower-bound searches.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>

#include "context.hpp"
#include "precluster_core.hpp"

namespace gg {
namespace {

namespace pc = precluster;

// parent[] through agent-scope atomics (precluster_core.hpp's policy)
struct DeviceParents {
  uint32_t* parent;
  __device__ uint32_t load(uint32_t x) const {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ void store(uint32_t x, uint32_t v) const {
    __hip_atomic_store(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ uint32_t fetch_min(uint32_t x, uint32_t v) const {
    return __hip_atomic_fetch_min(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ uint32_t cas(uint32_t x, uint32_t expect, uint32_t v) const {
    __hip_atomic_compare_exchange_strong(parent + x, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    return expect;  // the value before, whether it matched or not
  }
};

__device__ inline uint64_t grid_first() { return (uint64_t)blockIdx.x * 256 + threadIdx.x; }
__device__ inline uint64_t grid_step() { return (uint64_t)gridDim.x * 256; }

__global__ __launch_bounds__(256) void pc_init_kernel(uint32_t n, uint32_t* __restrict__ parent,
                                                      uint32_t* __restrict__ size) {
  for (uint64_t g = grid_first(); g < n; g += grid_step()) {
    parent[g] = (uint32_t)g;
    size[g] = 0;
  }
}

// 1. one thread per pair; see the invariants above
__global__ __launch_bounds__(256) void pc_hook_kernel(const gg_pair* __restrict__ pairs, uint64_t n_pairs, uint32_t n,
                                                      uint32_t* parent) {
  DeviceParents a{parent};
  for (uint64_t p = grid_first(); p < n_pairs; p += grid_step()) {
    const uint32_t i = pairs[p].i, j = pairs[p].j;
    if (i >= n || j >= n || i == j) continue;  // (never followed)
    pc::hook(a, i, j);
  }
}

// 2. up to kJumpsPerLaunch jumps of every vertex; *changed = 1 when any thread
// wrote.  (More than one jump per launch only saves launches, each of which
// costs a read-back: whatever a later jump reads is an ancestor as well.)
constexpr int kJumpsPerLaunch = 4;
__global__ __launch_bounds__(256) void pc_jump_kernel(uint32_t n, uint32_t* parent, uint32_t* changed) {
  DeviceParents a{parent};
  bool wrote = false;
  for (uint64_t x = grid_first(); x < n; x += grid_step())
    for (int r = 0; r < kJumpsPerLaunch && pc::jump(a, (uint32_t)x); ++r) wrote = true;
  if (__any(wrote) && (threadIdx.x & 63) == 0) __hip_atomic_store(changed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 3. sizes per root (parent[g] is g's root now).  The lanes of a wave that
// share a root add once: one set of a million genomes is otherwise a million
// atomics on one word.
__global__ __launch_bounds__(256) void pc_count_kernel(uint32_t n, const uint32_t* __restrict__ parent,
                                                       uint32_t* __restrict__ size) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t rounds = ((uint64_t)n + grid_step() - 1) / grid_step();  // (whole waves stay in the loop)
  uint64_t g = grid_first();
  for (uint64_t k = 0; k < rounds; ++k, g += grid_step()) {
    bool live = g < n;
    const uint32_t r = live ? parent[g] : 0;
    unsigned long long todo = __ballot(live);
    while (todo) {  // (uniform over the wave)
      const int leader = __ffsll((long long)todo) - 1;
      const uint32_t first = __shfl(r, leader);
      const unsigned long long same = __ballot(live && r == first);
      if ((int)lane == leader) atomicAdd(&size[first], (uint32_t)__popcll(same));
      if (r == first) live = false;
      todo &= ~same;
    }
  }
}

// the roots' keys appended in any order (one atomic per wave), *n_roots their count
__global__ __launch_bounds__(256) void pc_roots_kernel(uint32_t n, const uint32_t* __restrict__ parent,
                                                       const uint32_t* __restrict__ size, uint64_t* __restrict__ keys,
                                                       uint32_t* __restrict__ n_roots) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t rounds = ((uint64_t)n + grid_step() - 1) / grid_step();  // (whole waves stay in the loop)
  uint64_t g = grid_first();
  for (uint64_t r = 0; r < rounds; ++r, g += grid_step()) {
    const bool root = g < n && parent[g] == (uint32_t)g;
    const unsigned long long mask = __ballot(root);
    if (mask == 0) continue;
    uint32_t base = 0;
    const int leader = __ffsll((long long)mask) - 1;
    if ((int)lane == leader) base = atomicAdd(n_roots, (uint32_t)__popcll(mask));
    base = __shfl(base, leader);
    if (root) keys[base + __popcll(mask & ((1ull << lane) - 1))] = pc::set_key(n, size[g], (uint32_t)g);
  }
}

// sorted set keys -> rank_of[root], the sizes in rank order (and a 0 after them for the scan)
__global__ __launch_bounds__(256) void pc_rank_kernel(uint32_t n, uint32_t n_sets, const uint64_t* __restrict__ keys,
                                                      uint32_t* __restrict__ rank_of, uint32_t* __restrict__ sizes) {
  for (uint64_t r = grid_first(); r <= n_sets; r += grid_step()) {
    if (r == n_sets) {
      sizes[r] = 0;
      continue;
    }
    const uint64_t key = keys[r];
    rank_of[pc::set_key_root(key)] = (uint32_t)r;
    sizes[r] = pc::set_key_size(n, key);
  }
}

// 4. the genomes' member keys; after their sort members[], inv[] and each position's set
__global__ __launch_bounds__(256) void pc_member_keys_kernel(uint32_t n, const uint32_t* __restrict__ parent,
                                                             const uint32_t* __restrict__ rank_of,
                                                             uint64_t* __restrict__ keys) {
  for (uint64_t g = grid_first(); g < n; g += grid_step()) keys[g] = pc::member_key(rank_of[parent[g]], (uint32_t)g);
}

__global__ __launch_bounds__(256) void pc_members_kernel(uint32_t n, const uint64_t* __restrict__ keys,
                                                         uint32_t* __restrict__ members, uint32_t* __restrict__ inv,
                                                         uint32_t* __restrict__ pos_set) {
  for (uint64_t k = grid_first(); k < n; k += grid_step()) {
    const uint64_t key = keys[k];
    const uint32_t g = pc::member_key_genome(key);
    members[k] = g;
    inv[g] = (uint32_t)k;
    pos_set[k] = pc::member_key_rank(key);
  }
}

// 5. a pair's key from the positions of its genomes; src as the payload
__global__ __launch_bounds__(256) void pc_pair_keys_kernel(const gg_pair* __restrict__ pairs, uint64_t n_pairs,
                                                           uint32_t n, uint32_t bits, const uint32_t* __restrict__ inv,
                                                           uint64_t* __restrict__ keys, uint32_t* __restrict__ src) {
  for (uint64_t p = grid_first(); p < n_pairs; p += grid_step()) {
    const uint32_t i = pairs[p].i, j = pairs[p].j;
    uint64_t key = pc::pair_key_none(bits);  // (an index >= n: left out)
    if (i < n && j < n) {
      const uint32_t a = inv[i], b = inv[j];
      key = pc::pair_key(min(a, b), max(a, b), bits);
    }
    keys[p] = key;
    src[p] = (uint32_t)p;
  }
}

__global__ __launch_bounds__(256) void pc_finish_kernel(uint64_t n_pairs, uint32_t bits,
                                                        const uint64_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ src,
                                                        const uint32_t* __restrict__ pos_set,
                                                        const uint32_t* __restrict__ offsets,
                                                        gg_local_pair* __restrict__ local) {
  const uint64_t none = pc::pair_key_none(bits);
  for (uint64_t y = grid_first(); y < n_pairs; y += grid_step()) {
    const uint64_t key = keys[y];
    if (key == none) continue;  // (sorted last: local[] ends before them)
    const uint32_t a = pc::pair_key_a(key, bits), b = pc::pair_key_b(key, bits);
    const uint32_t s = pos_set[a], first = offsets[s];
    local[y] = gg_local_pair{s, a - first, b - first, src[y]};
  }
}

// pair_offsets[s] = the first sorted key at or above set s's first position
// (s = n_sets: above every pair written)
__global__ __launch_bounds__(256) void pc_pair_offsets_kernel(uint32_t n_sets, uint64_t n_pairs, uint32_t bits,
                                                              const uint64_t* __restrict__ keys,
                                                              const uint32_t* __restrict__ offsets,
                                                              uint64_t* __restrict__ pair_offsets) {
  for (uint64_t s = grid_first(); s <= n_sets; s += grid_step()) {
    const uint64_t want = pc::pair_key_floor(offsets[s], bits);
    uint64_t lo = 0, hi = n_pairs;
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (keys[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    pair_offsets[s] = lo;
  }
}

// no pairs: every genome its own set, in index order
__global__ __launch_bounds__(256) void pc_identity_kernel(uint32_t n, uint32_t* __restrict__ members,
                                                          uint32_t* __restrict__ offsets,
                                                          uint64_t* __restrict__ pair_offsets) {
  for (uint64_t g = grid_first(); g <= n; g += grid_step()) {
    if (g < n) members[g] = (uint32_t)g;
    offsets[g] = (uint32_t)g;
    if (pair_offsets) pair_offsets[g] = 0;
  }
}

inline dim3 grid_for(uint64_t items) { return dim3((uint32_t)std::min<uint64_t>(8192, (items + 255) / 256)); }

}  // namespace

gg_status preclusters_device(gg_ctx* c, uint32_t n, const gg_pair* d_pairs, uint64_t n_pairs, uint32_t* d_members,
                             uint32_t* d_offsets, uint32_t* n_sets, gg_local_pair* d_local, uint64_t* d_pair_offsets,
                             hipStream_t st) {
  ++c->precluster_calls;
  c->precluster_jumps = 0;
  *n_sets = 0;
  const bool with_pairs = d_pair_offsets != nullptr;
  if (n == 0 || n_pairs == 0) {
    GG_HIP(c, timed_launch(c, GG_KERNEL_PRECLUSTER, 0, st, [&] {
             hipLaunchKernelGGL(pc_identity_kernel, grid_for((uint64_t)n + 1), dim3(256), 0, st, n, d_members, d_offsets,
                                d_pair_offsets);
             return hipGetLastError();
           }));
    GG_HIP(c, hipStreamSynchronize(st));
    *n_sets = n;
    return GG_OK;
  }
  const uint32_t bits = pc::index_bits(n);
  // scratch, all of it reused by every call
  uint32_t *parent, *size, *rank_of, *sizes, *inv, *pos_set, *words, *h_words, *src = nullptr;
  uint64_t* keys;
  void* tmp;
  const uint64_t n_keys = std::max<uint64_t>(n, with_pairs ? n_pairs : 0);
  size_t tmp_bytes = 0, b = 0;
  GG_HIP(c, hipcub::DeviceRadixSort::SortKeys(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n, 0,
                                              (int)pc::set_key_bits(n)));
  tmp_bytes = std::max(tmp_bytes, b);
  GG_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(n + 1)));
  tmp_bytes = std::max(tmp_bytes, b);
  if (with_pairs) {
    GG_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                 (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n_pairs, 0,
                                                 (int)pc::pair_sort_bits(n)));
    tmp_bytes = std::max(tmp_bytes, b);
  }
  GG_HIP(c, scratch_t(c, "pc_parent", (size_t)n, &parent));
  GG_HIP(c, scratch_t(c, "pc_size", (size_t)n, &size));
  GG_HIP(c, scratch_t(c, "pc_rank", (size_t)n, &rank_of));
  GG_HIP(c, scratch_t(c, "pc_sizes", (size_t)n + 1, &sizes));
  GG_HIP(c, scratch_t(c, "pc_inv", (size_t)n, &inv));
  GG_HIP(c, scratch_t(c, "pc_pos_set", (size_t)n, &pos_set));
  GG_HIP(c, scratch_t(c, "pc_keys", (size_t)(2 * n_keys), &keys));
  if (with_pairs) GG_HIP(c, scratch_t(c, "pc_src", (size_t)(2 * n_pairs), &src));
  GG_HIP(c, scratch_t(c, "pc_words", 2, &words));
  GG_HIP(c, scratch(c, "pc_tmp", tmp_bytes, &tmp));
  GG_HIP(c, host_scratch_t(c, "pc_words", 2, &h_words));
  uint64_t* keys_out = keys + n_keys;
  uint32_t *changed = words, *n_roots = words + 1;
  auto launch = [&](uint64_t work, auto&& f) { return timed_launch(c, GG_KERNEL_PRECLUSTER, work, st, f); };

  // 1. hook
  GG_HIP(c, launch(n_pairs, [&] {
           hipLaunchKernelGGL(pc_init_kernel, grid_for(n), dim3(256), 0, st, n, parent, size);
           return hipGetLastError();
         }));
  GG_HIP(c, launch(0, [&] {
           hipLaunchKernelGGL(pc_hook_kernel, grid_for(n_pairs), dim3(256), 0, st, d_pairs, n_pairs, n, parent);
           return hipGetLastError();
         }));
  // 2. flatten
  const uint32_t bound = pc::jump_launch_bound(n);
  for (;;) {
    if (c->precluster_jumps >= bound)
      return fail(c, GG_ERR_INTERNAL, "gg_preclusters: the jump rounds did not end");
    GG_HIP(c, hipMemsetAsync(words, 0, 2 * sizeof(uint32_t), st));
    GG_HIP(c, launch(0, [&] {
             hipLaunchKernelGGL(pc_jump_kernel, grid_for(n), dim3(256), 0, st, n, parent, changed);
             return hipGetLastError();
           }));
    ++c->precluster_jumps;
    GG_HIP(c, hipMemcpyAsync(h_words, words, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GG_HIP(c, hipStreamSynchronize(st));
    if (h_words[0] == 0) break;
  }
  // 3. sets in order (n_roots is 0: cleared with the changed word of the last round)
  GG_HIP(c, launch(0, [&] {
           hipLaunchKernelGGL(pc_count_kernel, grid_for(n), dim3(256), 0, st, n, parent, size);
           return hipGetLastError();
         }));
  GG_HIP(c, launch(0, [&] {
           hipLaunchKernelGGL(pc_roots_kernel, grid_for(n), dim3(256), 0, st, n, parent, size, keys, n_roots);
           return hipGetLastError();
         }));
  GG_HIP(c, hipMemcpyAsync(h_words + 1, n_roots, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  GG_HIP(c, hipStreamSynchronize(st));
  const uint32_t ns = h_words[1];
  if (ns == 0 || ns > n) return fail(c, GG_ERR_INTERNAL, "gg_preclusters: bad set count " + std::to_string(ns));
  // (bit 0 up: see index_build_buckets on rocPRIM's merge-sort path)
  GG_HIP(c, launch(0, [&] {
           size_t bytes = tmp_bytes;
           return hipcub::DeviceRadixSort::SortKeys(tmp, bytes, keys, keys_out, (int)ns, 0, (int)pc::set_key_bits(n), st);
         }));
  GG_HIP(c, launch(0, [&] {
           hipLaunchKernelGGL(pc_rank_kernel, grid_for((uint64_t)ns + 1), dim3(256), 0, st, n, ns, keys_out, rank_of,
                              sizes);
           return hipGetLastError();
         }));
  GG_HIP(c, launch(0, [&] {
           size_t bytes = tmp_bytes;
           return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, sizes, d_offsets, (int)(ns + 1), st);
         }));
  // 4. members
  GG_HIP(c, launch(0, [&] {
           hipLaunchKernelGGL(pc_member_keys_kernel, grid_for(n), dim3(256), 0, st, n, parent, rank_of, keys);
           return hipGetLastError();
         }));
  GG_HIP(c, launch(0, [&] {
           size_t bytes = tmp_bytes;
           return hipcub::DeviceRadixSort::SortKeys(tmp, bytes, keys, keys_out, (int)n, 0, (int)pc::member_key_bits(ns),
                                                    st);
         }));
  GG_HIP(c, launch(0, [&] {
           hipLaunchKernelGGL(pc_members_kernel, grid_for(n), dim3(256), 0, st, n, keys_out, d_members, inv, pos_set);
           return hipGetLastError();
         }));
  // 5. local pairs
  if (with_pairs) {
    uint32_t* src_out = src + n_pairs;
    GG_HIP(c, launch(0, [&] {
             hipLaunchKernelGGL(pc_pair_keys_kernel, grid_for(n_pairs), dim3(256), 0, st, d_pairs, n_pairs, n, bits, inv,
                                keys, src);
             return hipGetLastError();
           }));
    GG_HIP(c, launch(0, [&] {
             size_t bytes = tmp_bytes;
             return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys, keys_out, src, src_out, (int)n_pairs, 0,
                                                       (int)pc::pair_sort_bits(n), st);
           }));
    GG_HIP(c, launch(0, [&] {
             hipLaunchKernelGGL(pc_finish_kernel, grid_for(n_pairs), dim3(256), 0, st, n_pairs, bits, keys_out, src_out,
                                pos_set, d_offsets, d_local);
             return hipGetLastError();
           }));
    GG_HIP(c, launch(0, [&] {
             hipLaunchKernelGGL(pc_pair_offsets_kernel, grid_for((uint64_t)ns + 1), dim3(256), 0, st, ns, n_pairs, bits,
                                keys_out, d_offsets, d_pair_offsets);
             return hipGetLastError();
           }));
  }
  GG_HIP(c, hipStreamSynchronize(st));
  *n_sets = ns;
  return GG_OK;
}

}  // namespace gg

using namespace gg;

extern "C" {

gg_status gg_preclusters_device(gg_ctx* ctx, uint32_t n_genomes, const gg_pair* d_pairs, uint64_t n_pairs,
                                uint32_t* d_members, uint32_t* d_offsets, uint32_t* n_sets, gg_local_pair* d_local,
                                uint64_t* d_pair_offsets, void* stream) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* m = primary(ctx);
  gg_status st = GG_OK;
  if ((n_pairs && !d_pairs) || !d_offsets || (n_genomes && !d_members) || !n_sets ||
      (d_pair_offsets ? (n_pairs && !d_local) : d_local != nullptr))
    st = fail(m, GG_ERR_INVALID_ARG, "gg_preclusters_device: null argument");
  else if (n_pairs >= (1ull << 31) || n_genomes >= (1u << 31))
    st = fail(m, GG_ERR_INVALID_ARG, "gg_preclusters_device: 2^31 pairs or genomes, or more");
  else if ((st = use_device(m)) == GG_OK)
    st = preclusters_device(m, n_genomes, d_pairs, n_pairs, d_members, d_offsets, n_sets, d_local, d_pair_offsets,
                            (hipStream_t)stream);
  return finish_call(ctx, m, st);
}

// gg_preclusters behind its context lookup
static gg_status preclusters_ctx(gg_ctx* m, uint32_t n_genomes, const gg_pair* pairs, uint64_t n_pairs, uint32_t* members,
                                 uint32_t* offsets, uint32_t* n_sets, gg_local_pair* local, uint64_t* pair_offsets) {
  if ((n_pairs && !pairs) || !offsets || (n_genomes && !members) || !n_sets ||
      (pair_offsets ? (n_pairs && !local) : local != nullptr))
    return fail(m, GG_ERR_INVALID_ARG, "gg_preclusters: null argument");
  if (n_pairs >= (1ull << 31) || n_genomes >= (1u << 31))
    return fail(m, GG_ERR_INVALID_ARG, "gg_preclusters: 2^31 pairs or genomes, or more");
  for (uint64_t p = 0; p < n_pairs; ++p)
    if (pairs[p].i >= n_genomes || pairs[p].j >= n_genomes)
      return fail(m, GG_ERR_INVALID_ARG, "gg_preclusters: pair index out of range");
  gg_status st = use_device(m);
  if (st != GG_OK) return st;
  const uint32_t n = n_genomes;
  gg_pair* d_pairs = nullptr;
  uint32_t *d_members = nullptr, *d_offsets = nullptr;
  gg_local_pair* d_local = nullptr;
  uint64_t* d_poff = nullptr;
  GG_HIP(m, scratch_t(m, "pc_in_pairs", (size_t)n_pairs, &d_pairs));
  GG_HIP(m, scratch_t(m, "pc_out_members", (size_t)n, &d_members));
  GG_HIP(m, scratch_t(m, "pc_out_offsets", (size_t)n + 1, &d_offsets));
  if (pair_offsets) {
    GG_HIP(m, scratch_t(m, "pc_out_local", (size_t)n_pairs, &d_local));
    GG_HIP(m, scratch_t(m, "pc_out_poff", (size_t)n + 1, &d_poff));
  }
  if (n_pairs) GG_HIP(m, hipMemcpyAsync(d_pairs, pairs, n_pairs * sizeof(gg_pair), hipMemcpyHostToDevice, m->stream));
  st = preclusters_device(m, n, d_pairs, n_pairs, d_members, d_offsets, n_sets, d_local, d_poff, m->stream);
  if (st != GG_OK) return st;
  const uint32_t ns = *n_sets;
  if (n) GG_HIP(m, hipMemcpyAsync(members, d_members, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  GG_HIP(m, hipMemcpyAsync(offsets, d_offsets, ((size_t)ns + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  if (pair_offsets) {
    if (n_pairs)
      GG_HIP(m, hipMemcpyAsync(local, d_local, n_pairs * sizeof(gg_local_pair), hipMemcpyDeviceToHost, m->stream));
    GG_HIP(m, hipMemcpyAsync(pair_offsets, d_poff, ((size_t)ns + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                             m->stream));
  }
  GG_HIP(m, hipStreamSynchronize(m->stream));
  return GG_OK;
}

gg_status gg_preclusters(gg_ctx* ctx, uint32_t n_genomes, const gg_pair* pairs, uint64_t n_pairs, uint32_t* members,
                         uint32_t* offsets, uint32_t* n_sets, gg_local_pair* local, uint64_t* pair_offsets) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* m = primary(ctx);
  return finish_call(ctx, m, preclusters_ctx(m, n_genomes, pairs, n_pairs, members, offsets, n_sets, local, pair_offsets));
}

}  // extern "C"
