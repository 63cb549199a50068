// The finch + finch clustering step on the device: from the
// pair cache of gg_precluster_files to rep_of[], by the rules of
// cluster_core.hpp (src/clusterer.rs:155-225 and :316-406 with
// skip_clusterer).
//
//   1. adjacency in CSR from the pair list: degree count, scan, scatter; both
//      directions, each edge with its f32 ANI (order inside a row: as the
//      atomics fall, and no rule depends on it);
//   2. a second CSR of the strong lower neighbours only (j < i, ani >= T),
//      counted and scattered by the same two kernels;
//   3. representative rounds.  A workgroup owns kRange consecutive vertices,
//      their states in LDS, and sweeps them until a sweep decides nothing: a
//      vertex becomes a member as soon as one strong lower neighbour is a
//      representative, a representative once all of them are members.  A
//      decision is final and follows from final states only, so a state read
//      early (another workgroup's, written in the same launch or still
//      "undecided" in a cache) can only delay a decision, never change it.
//      No workgroup waits for another: what a launch leaves undecided the
//      next launch takes up, and the host reads one word per launch.
//      Launch bound: when a launch starts with every vertex below range r
//      decided, range r's sweeps decide all of it (its lowest undecided
//      vertex depends on decided ones only), so launch k leaves ranges
//      0 .. k - 1 decided whatever the graph -- at most ceil(n / kRange)
//      launches, and as many as the ranges the longest chain of
//      dependencies crosses, plus one, when the chains are shorter;
//   4. memberships: one wave per vertex takes the maximum of
//      cluster::member_key over its representative neighbours (either side,
//      strong or not) -- no global atomics.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

#include "cluster_core.hpp"
#include "context.hpp"

namespace gg {
namespace {

constexpr uint32_t kRangeThreads = 256;
constexpr uint32_t kPerThread = 4;  // consecutive vertices of one thread, swept in order
constexpr uint32_t kRange = kRangeThreads * kPerThread;
constexpr uint32_t kHeavyRow = 64;  // more strong lower neighbours: the row is scanned by a wave

__device__ inline bool pair_ok(const gg_pair& p, uint32_t n) { return p.i < n && p.j < n && p.i != p.j; }

// degrees: cnt[v] edges of v (both directions), scnt[v] strong lower neighbours of v
__global__ __launch_bounds__(256) void cluster_count_kernel(const gg_pair* __restrict__ pairs,
                                                            const float* __restrict__ ani, uint64_t n_pairs,
                                                            uint32_t n, float T, uint32_t* __restrict__ cnt,
                                                            uint32_t* __restrict__ scnt) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * 256) {
    const gg_pair x = pairs[p];
    if (!pair_ok(x, n)) continue;
    atomicAdd(&cnt[x.i], 1u);
    atomicAdd(&cnt[x.j], 1u);
    if (cluster::strong(ani[p], T)) atomicAdd(&scnt[max(x.i, x.j)], 1u);
  }
}

// rows filled (fill / sfill: zero on entry, the rows' counts on exit)
__global__ __launch_bounds__(256) void cluster_scatter_kernel(const gg_pair* __restrict__ pairs,
                                                              const float* __restrict__ ani, uint64_t n_pairs,
                                                              uint32_t n, float T, const uint32_t* __restrict__ off,
                                                              const uint32_t* __restrict__ soff,
                                                              uint32_t* __restrict__ fill, uint32_t* __restrict__ sfill,
                                                              uint32_t* __restrict__ nbr, float* __restrict__ nani,
                                                              uint32_t* __restrict__ snbr) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * 256) {
    const gg_pair x = pairs[p];
    if (!pair_ok(x, n)) continue;
    const float a = ani[p];
    const uint32_t ei = off[x.i] + atomicAdd(&fill[x.i], 1u);
    nbr[ei] = x.j;
    nani[ei] = a;
    const uint32_t ej = off[x.j] + atomicAdd(&fill[x.j], 1u);
    nbr[ej] = x.i;
    nani[ej] = a;
    if (cluster::strong(a, T)) {
      const uint32_t hi = max(x.i, x.j);
      snbr[soff[hi] + atomicAdd(&sfill[hi], 1u)] = min(x.i, x.j);
    }
  }
}

// A state of another workgroup's range: from L2, so that a decision of this
// launch may be seen (it need not be: "undecided" is always a safe answer).
__device__ inline uint32_t load_state(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One representative round: workgroup r sweeps vertices [r * kRange, (r + 1) * kRange).
// range_und[r]: undecided vertices the range had after the last launch (a
// range with none returns at once); *und += those it still has.
__global__ __launch_bounds__(kRangeThreads) void cluster_rounds_kernel(uint32_t n, const uint32_t* __restrict__ soff,
                                                                       const uint32_t* __restrict__ snbr,
                                                                       uint32_t* state, uint32_t* __restrict__ range_und,
                                                                       uint32_t* __restrict__ und) {
  __shared__ uint32_t st_lds[kRange];
  __shared__ uint32_t heavy[kRange];
  __shared__ uint32_t n_heavy;
  __shared__ uint32_t part[kRangeThreads / 64];
  const uint32_t r = blockIdx.x, base = r * kRange, tid = threadIdx.x;
  if (range_und[r] == 0) return;
  const uint32_t cnt = min(kRange, n - base);
  volatile uint32_t* st = st_lds;
  for (uint32_t t = tid; t < kRange; t += kRangeThreads) st[t] = t < cnt ? state[base + t] : (uint32_t)cluster::kMember;
  if (tid == 0) n_heavy = 0;
  __syncthreads();
  // this thread's rows; a cursor b past the leading neighbours known to be members
  // (mine: bit x set while vertex x of this thread is undecided and its row
  // is light; heavy rows are left to the waves)
  uint32_t b[kPerThread], e[kPerThread], mine = 0;
#pragma unroll
  for (uint32_t x = 0; x < kPerThread; ++x) {
    const uint32_t v = tid * kPerThread + x;
    b[x] = e[x] = 0;
    if (v < cnt && st[v] == cluster::kUndecided) {
      b[x] = soff[base + v];
      e[x] = soff[base + v + 1];
      if (e[x] - b[x] > kHeavyRow) heavy[atomicAdd(&n_heavy, 1u)] = v;
      else mine |= 1u << x;
    }
  }
  __syncthreads();
  const uint32_t nh = n_heavy, wave = tid >> 6, lane = tid & 63;
  for (;;) {
    int changed = 0;
#pragma unroll
    for (uint32_t x = 0; x < kPerThread; ++x) {
      const uint32_t v = tid * kPerThread + x;
      if (!(mine >> x & 1)) continue;
      cluster::Seen seen;
      bool prefix = true;
      for (uint32_t k = b[x]; k < e[x] && !seen.rep; ++k) {
        const uint32_t u = snbr[k];
        const uint32_t su = u >= base ? st[u - base] : load_state(state + u);
        cluster::see(seen, su);
        if (prefix && su == cluster::kMember) b[x] = k + 1;
        else prefix = false;
      }
      const uint32_t d = cluster::decide(seen);
      if (d != cluster::kUndecided) {
        st[v] = d;
        __hip_atomic_store(state + base + v, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mine &= ~(1u << x);
        changed = 1;
      }
    }
    for (uint32_t h = wave; h < nh; h += kRangeThreads / 64) {
      const uint32_t v = heavy[h];
      if (st[v] != cluster::kUndecided) continue;
      cluster::Seen seen;
      const uint32_t k1 = soff[base + v + 1];
      for (uint32_t k = soff[base + v] + lane; k < k1; k += 64) {
        const uint32_t u = snbr[k];
        cluster::see(seen, u >= base ? st[u - base] : load_state(state + u));
      }
      seen.rep = __ballot(seen.rep) != 0;
      seen.undecided = __ballot(seen.undecided) != 0;
      const uint32_t d = cluster::decide(seen);
      if (d != cluster::kUndecided) {
        if (lane == 0) {
          st[v] = d;
          __hip_atomic_store(state + base + v, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        changed = 1;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  // what the range leaves to the next launch
  uint32_t left = 0;
#pragma unroll
  for (uint32_t x = 0; x < kPerThread; ++x) {
    const uint32_t v = tid * kPerThread + x;
    left += v < cnt && st[v] == cluster::kUndecided;
  }
  for (int o = 32; o > 0; o >>= 1) left += __shfl_xor(left, o);
  if (lane == 0) part[wave] = left;
  __syncthreads();
  if (tid == 0) {
    uint32_t total = 0;
    for (uint32_t w = 0; w < kRangeThreads / 64; ++w) total += part[w];
    range_und[r] = total;
    if (total) atomicAdd(und, total);
  }
}

// one wave per vertex: a representative is its own, a member takes the
// representative neighbour with the largest key
__global__ __launch_bounds__(256) void cluster_members_kernel(uint32_t n, const uint32_t* __restrict__ off,
                                                              const uint32_t* __restrict__ nbr,
                                                              const float* __restrict__ nani,
                                                              const uint32_t* __restrict__ state,
                                                              uint32_t* __restrict__ rep_of) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t waves = (uint64_t)gridDim.x * 4;
  for (uint64_t v = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < n; v += waves) {
    if (state[v] == cluster::kRep) {
      if (lane == 0) rep_of[v] = (uint32_t)v;
      continue;
    }
    unsigned long long key = 0;
    const uint32_t k1 = off[v + 1];
    for (uint32_t k = off[v] + lane; k < k1; k += 64) {
      const uint32_t u = nbr[k];
      if (state[u] == cluster::kRep) key = max(key, (unsigned long long)cluster::member_key(nani[k], u));
    }
    for (int o = 32; o > 0; o >>= 1) key = max(key, (unsigned long long)__shfl_xor(key, o));
    if (lane == 0) rep_of[v] = key ? cluster::key_rep(key) : cluster::kNoRep;
  }
}

// no pairs: every genome is its own representative
__global__ __launch_bounds__(256) void cluster_identity_kernel(uint32_t n, uint32_t* __restrict__ rep_of) {
  for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (uint64_t)gridDim.x * 256)
    rep_of[v] = (uint32_t)v;
}

}  // namespace

gg_status cluster_device(gg_ctx* c, uint32_t n, const gg_pair* d_pairs, const float* d_ani, uint64_t n_pairs, float T,
                         uint32_t* d_rep_of, hipStream_t st) {
  ++c->cluster_calls;
  c->cluster_rounds = 0;
  if (n == 0) return GG_OK;
  if (n_pairs == 0) {
    GG_HIP(c, timed_launch(c, GG_KERNEL_CLUSTER, 0, st, [&] {
             hipLaunchKernelGGL(cluster_identity_kernel, dim3(std::min<uint32_t>(4096, (n + 255) / 256)), dim3(256), 0,
                                st, n, d_rep_of);
             return hipGetLastError();
           }));
    GG_HIP(c, hipStreamSynchronize(st));
    return GG_OK;
  }
  const uint32_t n_ranges = (n + kRange - 1) / kRange;
  // scratch, all of it reused by every call; cnt / scnt: counts, then (after
  // the scans) the scatter's fill cursors
  uint32_t *cnt, *scnt, *off, *soff, *nbr, *snbr, *state, *range_und, *und, *h_und;
  float* nani;
  void* tmp;
  size_t tmp_bytes = 0;
  GG_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (int)(n + 1)));
  GG_HIP(c, scratch_t(c, "cl_cnt", 2 * ((size_t)n + 1), &cnt));
  scnt = cnt + n + 1;
  GG_HIP(c, scratch_t(c, "cl_off", 2 * ((size_t)n + 1), &off));
  soff = off + n + 1;
  GG_HIP(c, scratch_t(c, "cl_nbr", 2 * n_pairs, &nbr));
  GG_HIP(c, scratch_t(c, "cl_nani", 2 * n_pairs, &nani));
  GG_HIP(c, scratch_t(c, "cl_snbr", n_pairs, &snbr));
  GG_HIP(c, scratch_t(c, "cl_state", (size_t)n + n_ranges + 1, &state));
  range_und = state + n;
  und = range_und + n_ranges;
  GG_HIP(c, scratch(c, "cl_tmp", tmp_bytes, &tmp));
  GG_HIP(c, host_scratch_t(c, "cl_und", 1, &h_und));

  const uint32_t pair_grid = (uint32_t)std::min<uint64_t>(8192, (n_pairs + 255) / 256);
  GG_HIP(c, hipMemsetAsync(cnt, 0, 2 * ((size_t)n + 1) * sizeof(uint32_t), st));
  GG_HIP(c, timed_launch(c, GG_KERNEL_CLUSTER, n_pairs, st, [&] {
           hipLaunchKernelGGL(cluster_count_kernel, dim3(pair_grid), dim3(256), 0, st, d_pairs, d_ani, n_pairs, n, T,
                              cnt, scnt);
           return hipGetLastError();
         }));
  for (int which = 0; which < 2; ++which) {
    GG_HIP(c, timed_launch(c, GG_KERNEL_CLUSTER, 0, st, [&] {
             size_t bytes = tmp_bytes;
             return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, which ? scnt : cnt, which ? soff : off, (int)(n + 1),
                                                     st);
           }));
  }
  GG_HIP(c, hipMemsetAsync(cnt, 0, 2 * ((size_t)n + 1) * sizeof(uint32_t), st));
  GG_HIP(c, timed_launch(c, GG_KERNEL_CLUSTER, 0, st, [&] {
           hipLaunchKernelGGL(cluster_scatter_kernel, dim3(pair_grid), dim3(256), 0, st, d_pairs, d_ani, n_pairs, n, T,
                              off, soff, cnt, scnt, nbr, nani, snbr);
           return hipGetLastError();
         }));
  // rounds: every vertex undecided (state 0), every range marked as having some
  static_assert(cluster::kUndecided == 0, "the states are cleared with a memset");
  GG_HIP(c, hipMemsetAsync(state, 0, (size_t)n * sizeof(uint32_t), st));
  GG_HIP(c, hipMemsetAsync(range_und, 0xFF, (size_t)n_ranges * sizeof(uint32_t), st));
  for (;;) {
    if (c->cluster_rounds > (uint64_t)n_ranges)  // (launch k leaves ranges 0 .. k - 1 decided)
      return fail(c, GG_ERR_INTERNAL, "gg_cluster_pairs: the representative rounds did not end");
    GG_HIP(c, hipMemsetAsync(und, 0, sizeof(uint32_t), st));
    GG_HIP(c, timed_launch(c, GG_KERNEL_CLUSTER, 0, st, [&] {
             hipLaunchKernelGGL(cluster_rounds_kernel, dim3(n_ranges), dim3(kRangeThreads), 0, st, n, soff, snbr, state,
                                range_und, und);
             return hipGetLastError();
           }));
    ++c->cluster_rounds;
    GG_HIP(c, hipMemcpyAsync(h_und, und, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GG_HIP(c, hipStreamSynchronize(st));
    if (*h_und == 0) break;
  }
  GG_HIP(c, timed_launch(c, GG_KERNEL_CLUSTER, 0, st, [&] {
           hipLaunchKernelGGL(cluster_members_kernel, dim3(std::min<uint32_t>(8192, (n + 3) / 4)), dim3(256), 0, st, n,
                              off, nbr, nani, state, d_rep_of);
           return hipGetLastError();
         }));
  GG_HIP(c, hipStreamSynchronize(st));
  return GG_OK;
}

}  // namespace gg

using namespace gg;

extern "C" {

gg_status gg_cluster_pairs_device(gg_ctx* ctx, uint32_t n_genomes, const gg_pair* d_pairs, const float* d_ani,
                                  uint64_t n_pairs, float cluster_ani, uint32_t* d_rep_of, void* stream) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* m = primary(ctx);
  gg_status st = GG_OK;
  if ((n_pairs && (!d_pairs || !d_ani)) || (n_genomes && !d_rep_of))
    st = fail(m, GG_ERR_INVALID_ARG, "gg_cluster_pairs_device: null buffer");
  else if (std::isnan(cluster_ani))
    st = fail(m, GG_ERR_INVALID_ARG, "gg_cluster_pairs_device: cluster_ani is NaN");
  else if (n_pairs >= (1ull << 31) || n_genomes >= (1u << 31))
    st = fail(m, GG_ERR_INVALID_ARG, "gg_cluster_pairs_device: 2^31 pairs or genomes, or more");
  else if ((st = use_device(m)) == GG_OK)
    st = cluster_device(m, n_genomes, d_pairs, d_ani, n_pairs, cluster_ani, d_rep_of, (hipStream_t)stream);
  return finish_call(ctx, m, st);
}

// gg_cluster_pairs behind its context lookup
static gg_status cluster_pairs_ctx(gg_ctx* m, uint32_t n_genomes, const gg_pair* pairs, const float* ani, uint64_t n_pairs,
                                   float cluster_ani, uint32_t* rep_of) {
  const gg_status chk = cluster_check_input("gg_cluster_pairs", n_genomes, pairs, ani, n_pairs, cluster_ani, rep_of);
  if (chk != GG_OK) return fail(m, chk, gg_thread_last_error());
  if (n_genomes >= (1u << 31)) return fail(m, GG_ERR_INVALID_ARG, "gg_cluster_pairs: 2^31 genomes or more");
  if (n_genomes == 0) return GG_OK;
  gg_status st = use_device(m);
  if (st != GG_OK) return st;
  gg_pair* d_pairs = nullptr;
  float* d_ani = nullptr;
  uint32_t* d_rep = nullptr;
  GG_HIP(m, scratch_t(m, "cl_in_pairs", (size_t)n_pairs, &d_pairs));
  GG_HIP(m, scratch_t(m, "cl_in_ani", (size_t)n_pairs, &d_ani));
  GG_HIP(m, scratch_t(m, "cl_rep", (size_t)n_genomes, &d_rep));
  if (n_pairs) {
    GG_HIP(m, hipMemcpyAsync(d_pairs, pairs, n_pairs * sizeof(gg_pair), hipMemcpyHostToDevice, m->stream));
    GG_HIP(m, hipMemcpyAsync(d_ani, ani, n_pairs * sizeof(float), hipMemcpyHostToDevice, m->stream));
  }
  st = cluster_device(m, n_genomes, d_pairs, d_ani, n_pairs, cluster_ani, d_rep, m->stream);
  if (st != GG_OK) return st;
  GG_HIP(m, hipMemcpyAsync(rep_of, d_rep, (size_t)n_genomes * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  GG_HIP(m, hipStreamSynchronize(m->stream));
  return GG_OK;
}

gg_status gg_cluster_pairs(gg_ctx* ctx, uint32_t n_genomes, const gg_pair* pairs, const float* ani, uint64_t n_pairs,
                           float cluster_ani, uint32_t* rep_of) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* m = primary(ctx);
  return finish_call(ctx, m, cluster_pairs_ctx(m, n_genomes, pairs, ani, n_pairs, cluster_ani, rep_of));
}

gg_status gg_cluster_files(gg_ctx* ctx, const char* const* paths, uint32_t n_paths, float min_ani, float cluster_ani,
                           const char* cache_dir, uint32_t* rep_of, gg_pair** pairs, float** ani, uint64_t* n_out) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  if (pairs) *pairs = nullptr;
  if (ani) *ani = nullptr;
  if (n_out) *n_out = 0;
  if ((n_paths && !rep_of) || std::isnan(cluster_ani))
    return fail(ctx, GG_ERR_INVALID_ARG, "gg_cluster_files: null rep_of or NaN cluster_ani");
  gg_pair* p = nullptr;
  float* a = nullptr;
  uint64_t n = 0;
  gg_status st = gg_precluster_files_cached(ctx, paths, n_paths, min_ani, cache_dir, &p, &a, &n, nullptr);
  if (st == GG_OK) st = gg_cluster_pairs(ctx, n_paths, p, a, n, cluster_ani, rep_of);
  if (st == GG_OK && pairs && ani && n_out) {
    *pairs = p;
    *ani = a;
    *n_out = n;
  } else {
    gg_free(p);
    gg_free(a);
  }
  return st;
}

}  // extern "C"
