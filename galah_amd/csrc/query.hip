// Querying a set of resident rows: every cell (row i, query
// q) that passes gg_pairs' test, with the small side indexed and the large
// side streamed once.
//
//   query table     per batch of queries: their (hash, q) entries radix-sorted
//                   by hash (hipcub, stable: q ascending inside a hash), equal
//                   hashes one column (col_off / col_q), and an open-addressing
//                   table slot -> (hash, column) filled with atomicCAS by the
//                   rules of query_core.hpp;
//   query_rows_kernel  one wave per collection row, grid-stride: the lanes
//                   read the row coalesced and probe the table, four probes in
//                   flight per lane.  A row without a hit leaves there.  A hit
//                   adds 1 to the u16 LDS counter of every query of the column
//                   (the wave's own counters, indexed by the query's number in
//                   the batch); the first touch appends the query to the
//                   wave's touched list.  After the row each touched query's
//                   counter is its `common`: reset, dropped on sufmin, total
//                   by validate_core.hpp's rank form, tested on cmin, appended
//                   by gg_pairs_device's contract (one atomicAdd per wave and
//                   round of 64 touched queries);
//   query_rect_kernel / query_append_kernel   min_ani <= 0 (every cell
//                   passes, without a shared hash too): the rectangle listed
//                   for the named-pair kernel (ani_pairs.hip), its result
//                   appended;
//   query_best_*    the best candidate of every query: atomicMax of
//                   query_core.hpp's key, then the pair that holds the
//                   winning key writes itself.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "context.hpp"
#include "device_util.hpp"
#include "gg_internal.hpp"
#include "query_core.hpp"
#include "validate_core.hpp"

namespace gg {
namespace {

constexpr int kQueryBlock = 256;
constexpr int kQueryWaves = kQueryBlock / 64;
constexpr int kProbes = 4;                  // table reads in flight per lane
constexpr uint32_t kQueryGridMax = 256 * 8;  // workgroups of the stream kernel

// Orders a wave's own LDS writes before its reads of other lanes' entries.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the query table ----------------------------------------------------------
constexpr int kScanItems = (query::kQueryBatch + kQueryBlock - 1) / kQueryBlock;

// off[b] = the entries of the batch's queries before b (off[nb] = all of them)
__global__ __launch_bounds__(kQueryBlock) void query_offsets_kernel(const uint32_t* __restrict__ q_lens, uint32_t nb,
                                                                    uint32_t s, uint32_t* __restrict__ off) {
  using Scan = hipcub::BlockScan<uint32_t, kQueryBlock>;
  __shared__ typename Scan::TempStorage tmp;
  uint32_t v[kScanItems], o[kScanItems], total;
#pragma unroll
  for (int x = 0; x < kScanItems; ++x) {
    const uint32_t b = threadIdx.x * kScanItems + x;
    v[x] = b < nb ? min(q_lens[b], s) : 0u;
  }
  Scan(tmp).ExclusiveSum(v, o, total);
#pragma unroll
  for (int x = 0; x < kScanItems; ++x) {
    const uint32_t b = threadIdx.x * kScanItems + x;
    if (b < nb) off[b] = o[x];
  }
  if (threadIdx.x == 0) off[nb] = total;
}

// (hash, q) of every entry, query after query
__global__ __launch_bounds__(kQueryBlock) void query_entries_kernel(const uint64_t* __restrict__ q_sk,
                                                                    const uint32_t* __restrict__ q_lens, uint32_t s,
                                                                    const uint32_t* __restrict__ off,
                                                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t q = blockIdx.y, e = blockIdx.x * kQueryBlock + threadIdx.x;
  if (e >= min(q_lens[q], s)) return;
  keys[off[q] + e] = q_sk[(uint64_t)q * s + e];
  vals[off[q] + e] = q;
}

// 1 at the first entry of every run of equal hashes
__global__ __launch_bounds__(kQueryBlock) void query_heads_kernel(const uint64_t* __restrict__ keys, uint32_t n_entries,
                                                                  uint32_t* __restrict__ head) {
  const uint32_t e = blockIdx.x * kQueryBlock + threadIdx.x;
  if (e < n_entries) head[e] = (e == 0 || keys[e] != keys[e - 1]) ? 1u : 0u;
}

struct DeviceClaim {
  __device__ bool operator()(uint32_t* at, uint32_t col) const { return atomicCAS(at, query::kEmpty, col) == query::kEmpty; }
};

// id[e] = the heads up to and including e: entry e belongs to column id[e] - 1
__global__ __launch_bounds__(kQueryBlock) void query_columns_kernel(const uint64_t* __restrict__ keys,
                                                                    const uint32_t* __restrict__ head,
                                                                    const uint32_t* __restrict__ id, uint32_t n_entries,
                                                                    uint32_t* __restrict__ col_off, query::Slot* table,
                                                                    uint64_t mask) {
  const uint32_t e = blockIdx.x * kQueryBlock + threadIdx.x;
  if (e >= n_entries) return;
  if (head[e]) {
    const uint32_t c = id[e] - 1;
    col_off[c] = e;
    query::insert(table, mask, keys[e], c, DeviceClaim());
  }
  if (e == n_entries - 1) col_off[id[e]] = n_entries;
}

// ---- the stream kernel --------------------------------------------------------
struct QueryRows {
  const uint64_t* sk;
  const uint32_t* lens;
  uint32_t n;
  const uint64_t* q_sk;  // the batch's first query
  const uint32_t* q_lens;
  uint32_t j0;           // j of the batch's first query
  uint32_t nb_pad;       // the batch's queries, rounded up to a multiple of 64
  uint32_t s;
  const query::Slot* table;
  uint64_t mask;
  const uint32_t* col_off;
  const uint32_t* col_q;
  const uint32_t* cmin;
  const uint32_t* sufmin;
  gg_pair* out;
  uint64_t cap;
  unsigned long long* count;
};

__global__ __launch_bounds__(kQueryBlock) void query_rows_kernel(QueryRows a) {
  // per wave: nb_pad / 2 words of u16 counters, nb_pad u16 of touched list; then the lists' lengths
  extern __shared__ __align__(16) uint8_t query_smem[];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t* cnt = reinterpret_cast<uint32_t*>(query_smem + (size_t)wave * a.nb_pad * 4);
  uint16_t* touched = reinterpret_cast<uint16_t*>(cnt + a.nb_pad / 2);
  uint32_t* n_touched = reinterpret_cast<uint32_t*>(query_smem + (size_t)kQueryWaves * a.nb_pad * 4) + wave;
  for (uint32_t w = lane; w < a.nb_pad / 2; w += 64) cnt[w] = 0;
  if (lane == 0) *n_touched = 0;
  wave_lds_sync();
  const uint64_t waves = (uint64_t)gridDim.x * kQueryWaves;
  for (uint64_t i = (uint64_t)blockIdx.x * kQueryWaves + wave; i < a.n; i += waves) {
    const uint32_t len = min(uni32(a.lens[i]), a.s);
    const uint64_t* __restrict__ row = a.sk + i * a.s;
    bool hit = false;
    for (uint32_t e0 = 0; e0 < len; e0 += 64 * kProbes) {
      uint64_t h[kProbes], at[kProbes];
      query::Slot sl[kProbes];
#pragma unroll
      for (int u = 0; u < kProbes; ++u) {
        const uint32_t e = e0 + u * 64 + lane;
        h[u] = e < len ? row[e] : 0;  // (a lane past the row probes hash 0 and ignores what it finds)
      }
#pragma unroll
      for (int u = 0; u < kProbes; ++u) {
        at[u] = query::slot_of(h[u], a.mask);
        sl[u] = a.table[at[u]];
      }
#pragma unroll
      for (int u = 0; u < kProbes; ++u) {
        if (e0 + u * 64 + lane >= len) continue;
        query::Probe p;
        while ((p = query::probe(sl[u].col, sl[u].hash, h[u])) == query::kNext) {
          at[u] = query::next_slot(at[u], a.mask);
          sl[u] = a.table[at[u]];
        }
        if (p != query::kHit) continue;
        hit = true;
        const uint32_t c = sl[u].col;
        for (uint32_t x = a.col_off[c], x1 = a.col_off[c + 1]; x < x1; ++x) {
          const uint32_t q = a.col_q[x], sh = (q & 1u) * 16u;
          const uint32_t old = atomicAdd(&cnt[q >> 1], 1u << sh);
          if (((old >> sh) & 0xFFFFu) == 0) touched[atomicAdd(n_touched, 1u)] = (uint16_t)q;
        }
      }
    }
    if (__ballot(hit) == 0) continue;  // the common case: nothing shared with any query
    wave_lds_sync();
    const uint32_t nt = uni32(*n_touched);
    const uint64_t last_row = uni64(row[len - 1]);  // (a hit: the row is not empty)
    const uint32_t hibit_row = validate::hibit_of(len);
    for (uint32_t t0 = 0; t0 < nt; t0 += 64) {
      const uint32_t t = t0 + lane;
      bool pass = false;
      gg_pair p{0, 0, 0, 0};
      if (t < nt) {
        const uint32_t q = touched[t], sh = (q & 1u) * 16u;
        const uint32_t common = (atomicAnd(&cnt[q >> 1], ~(0xFFFFu << sh)) >> sh) & 0xFFFFu;  // read and reset
        const uint32_t qlen = min(a.q_lens[q], a.s);
        if (common >= a.sufmin[min(len, qlen)]) {
          const uint64_t* __restrict__ qrow = a.q_sk + (uint64_t)q * a.s;
          const uint64_t last_q = qrow[qlen - 1];
          // the row whose last element is the smaller is exhausted first (equal: either)
          const bool row_ends = last_row <= last_q;
          const uint32_t rank = row_ends ? validate::rank_le(qrow, qlen, validate::hibit_of(qlen), last_row)
                                         : validate::rank_le(row, len, hibit_row, last_q);
          const uint32_t total = validate::total_from_rank(row_ends ? len : qlen, rank, common);
          if (total <= 2 * a.s && common >= a.cmin[total]) {  // (rows that are not ascending: no table entry)
            pass = true;
            p = gg_pair{(uint32_t)i, a.j0 + q, common, total};
          }
        }
      }
      const uint64_t m = __ballot(pass);
      if (m) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.count, (unsigned long long)__popcll(m));
        base = uni64(base);
        const uint64_t pos = base + lanes_below(m);
        if (pass && pos < a.cap) a.out[pos] = p;  // past the capacity: counted, not written
      }
    }
    wave_lds_sync();
    if (lane == 0) *n_touched = 0;
    wave_lds_sync();
  }
}

// ---- min_ani <= 0: the rectangle ------------------------------------------------
// cell p of rows [i0, i0 + ...) x nq queries: the pair (i, n + q) of the rows followed by the queries
__global__ __launch_bounds__(kQueryBlock) void query_rect_kernel(gg_pair* __restrict__ list, uint64_t m, uint32_t i0,
                                                                 uint32_t n, uint32_t nq) {
  for (uint64_t p = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x; p < m; p += (uint64_t)gridDim.x * kQueryBlock)
    list[p] = gg_pair{i0 + (uint32_t)(p / nq), n + (uint32_t)(p % nq), 0, 0};
}
// list[0 .. m) appended at *count (read, not written: query_count_kernel adds m afterwards)
__global__ __launch_bounds__(kQueryBlock) void query_append_kernel(const gg_pair* __restrict__ list, uint64_t m,
                                                                   gg_pair* __restrict__ out, uint64_t cap,
                                                                   const unsigned long long* __restrict__ count) {
  const uint64_t base = *count;
  for (uint64_t p = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x; p < m; p += (uint64_t)gridDim.x * kQueryBlock)
    if (base + p < cap) out[base + p] = list[p];
}
__global__ void query_count_kernel(unsigned long long* count, uint64_t m) { *count += m; }

// ---- the best hit ------------------------------------------------------------------
__global__ __launch_bounds__(kQueryBlock) void query_best_init_kernel(uint32_t n, uint32_t nq, unsigned long long* key,
                                                                      gg_pair* best, float* best_ani) {
  const uint32_t q = blockIdx.x * kQueryBlock + threadIdx.x;
  if (q >= nq) return;
  key[q] = 0;
  best[q] = gg_pair{query::kNoHit, n + q, 0, 0};
  best_ani[q] = 0.0f;
}
// the key of pair p for its query (false: the pair names no candidate row of a query)
__device__ __forceinline__ bool best_key_of(const gg_pair& p, float ani, uint32_t n, uint32_t nq,
                                            const uint32_t* __restrict__ rank, uint32_t* q, uint64_t* key) {
  if (p.i >= n || p.j < n || p.j - n >= nq) return false;
  const uint32_t r = rank ? rank[p.i] : p.i;
  if (r == query::kNotCandidate) return false;
  *q = p.j - n;
  *key = query::best_key(ani, r);
  return true;
}
__global__ __launch_bounds__(kQueryBlock) void query_best_kernel(uint32_t n, uint32_t nq, const gg_pair* __restrict__ pairs,
                                                                 const float* __restrict__ ani, uint64_t n_pairs,
                                                                 const uint32_t* __restrict__ rank,
                                                                 unsigned long long* key) {
  for (uint64_t p = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * kQueryBlock) {
    uint32_t q;
    uint64_t k;
    if (best_key_of(pairs[p], ani[p], n, nq, rank, &q, &k)) atomicMax(&key[q], (unsigned long long)k);
  }
}
// the candidates' ranks are distinct: one pair of a query holds its winning key
__global__ __launch_bounds__(kQueryBlock) void query_best_write_kernel(uint32_t n, uint32_t nq,
                                                                       const gg_pair* __restrict__ pairs,
                                                                       const float* __restrict__ ani, uint64_t n_pairs,
                                                                       const uint32_t* __restrict__ rank,
                                                                       const unsigned long long* __restrict__ key,
                                                                       gg_pair* best, float* best_ani) {
  for (uint64_t p = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * kQueryBlock) {
    uint32_t q;
    uint64_t k;
    const gg_pair x = pairs[p];
    if (best_key_of(x, ani[p], n, nq, rank, &q, &k) && key[q] == k) {
      best[q] = x;
      best_ani[q] = ani[p];
    }
  }
}

uint32_t grid_for(uint64_t items) {
  return (uint32_t)std::min<uint64_t>(kQueryGridMax, std::max<uint64_t>(1, (items + kQueryBlock - 1) / kQueryBlock));
}

// One batch: queries [0, nb) at q_sk / q_lens, j0 = the first one's j.
gg_status query_batch_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n, const uint64_t* q_sk,
                             const uint32_t* q_lens, uint32_t nb, uint32_t j0, const uint32_t* d_cmin,
                             const uint32_t* d_sufmin, gg_pair* d_out, uint64_t cap, uint64_t* d_count, hipStream_t st) {
  const uint32_t s = c->s;
  const uint64_t max_entries = (uint64_t)nb * s;  // < 2^32: nb <= kQueryBatch, s <= kMaxSketch
  uint32_t *d_off, *d_vals, *d_colq, *d_head, *d_id, *d_coloff, *h_entries;
  uint64_t *d_keys, *d_keys2;
  GG_HIP(c, scratch_t(c, "qy_off", (size_t)nb + 1, &d_off));
  GG_HIP(c, host_scratch_t(c, "qy_entries", 1, &h_entries));
  GG_HIP(c, scratch_t(c, "qy_keys", (size_t)max_entries * 2, &d_keys));
  d_keys2 = d_keys + max_entries;
  GG_HIP(c, scratch_t(c, "qy_vals", (size_t)max_entries * 4 + 2, &d_vals));
  d_colq = d_vals + max_entries;
  d_head = d_colq + max_entries;
  d_id = d_head + max_entries;
  GG_HIP(c, scratch_t(c, "qy_coloff", (size_t)max_entries + 1, &d_coloff));
  hipLaunchKernelGGL(query_offsets_kernel, dim3(1), dim3(kQueryBlock), 0, st, q_lens, nb, s, d_off);
  GG_HIP(c, hipGetLastError());
  // the one count the host needs: the sort's and the table's size
  GG_HIP(c, hipMemcpyAsync(h_entries, d_off + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  GG_HIP(c, hipStreamSynchronize(st));
  const uint32_t E = *h_entries;
  if (E > max_entries) return fail(c, GG_ERR_INTERNAL, "query: bad entry count");
  if (E == 0) return GG_OK;  // no column: nothing is built and nothing found
  // sized from the entries, an upper bound of the columns: no second count comes back
  const uint64_t slots = query::capacity(E);
  query::Slot* d_table;
  GG_HIP(c, scratch_t(c, "qy_table", (size_t)slots, &d_table));
  size_t sort_bytes = 0, scan_bytes = 0;
  GG_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                               (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)E, 0, 64, st));
  GG_HIP(c, hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)E, st));
  void* d_tmp;
  const size_t tmp_bytes = std::max<size_t>(std::max(sort_bytes, scan_bytes), 16);
  GG_HIP(c, scratch(c, "qy_tmp", tmp_bytes, &d_tmp));
  GG_HIP(c, timed_launch(c, GG_KERNEL_PAIRS_INDEX, E, st, [&]() -> hipError_t {
    hipLaunchKernelGGL(query_entries_kernel, dim3((s + kQueryBlock - 1) / kQueryBlock, nb), dim3(kQueryBlock), 0, st, q_sk,
                       q_lens, s, d_off, d_keys, d_vals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t b = sort_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(d_tmp, b, (const uint64_t*)d_keys, d_keys2, (const uint32_t*)d_vals, d_colq,
                                           (int)E, 0, 64, st);
    if (e != hipSuccess) return e;
    const uint32_t g = (E + kQueryBlock - 1) / kQueryBlock;
    hipLaunchKernelGGL(query_heads_kernel, dim3(g), dim3(kQueryBlock), 0, st, d_keys2, E, d_head);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    b = scan_bytes;
    e = hipcub::DeviceScan::InclusiveSum(d_tmp, b, (const uint32_t*)d_head, d_id, (int)E, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(d_table, 0xFF, (size_t)slots * sizeof(query::Slot), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(query_columns_kernel, dim3(g), dim3(kQueryBlock), 0, st, d_keys2, d_head, d_id, E, d_coloff,
                       d_table, slots - 1);
    return hipGetLastError();
  }));
  QueryRows a;
  a.sk = d_sk;
  a.lens = d_lens;
  a.n = n;
  a.q_sk = q_sk;
  a.q_lens = q_lens;
  a.j0 = j0;
  a.nb_pad = (nb + 63u) & ~63u;
  a.s = s;
  a.table = d_table;
  a.mask = slots - 1;
  a.col_off = d_coloff;
  a.col_q = d_colq;
  a.cmin = d_cmin;
  a.sufmin = d_sufmin;
  a.out = d_out;
  a.cap = cap;
  a.count = reinterpret_cast<unsigned long long*>(d_count);
  const size_t lds = (size_t)kQueryWaves * a.nb_pad * 4 + kQueryWaves * sizeof(uint32_t);
  const uint32_t grid = (uint32_t)std::min<uint64_t>(kQueryGridMax, ((uint64_t)n + kQueryWaves - 1) / kQueryWaves);
  GG_HIP(c, timed_launch(c, GG_KERNEL_PAIRS, (uint64_t)n * nb, st, [&]() -> hipError_t {
    hipLaunchKernelGGL(query_rows_kernel, dim3(grid), dim3(kQueryBlock), lds, st, a);
    return hipGetLastError();
  }));
  return GG_OK;
}

}  // namespace

gg_status query_append_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n, const uint64_t* d_q_sk,
                              const uint32_t* d_q_lens, uint32_t nq, uint32_t batch, const uint32_t* d_cmin,
                              const uint32_t* d_sufmin, gg_pair* d_out, uint64_t cap, uint64_t* d_count, hipStream_t st) {
  batch = std::max(1u, std::min(batch, query::batch_queries(c->s)));
  for (uint32_t q0 = 0; q0 < nq; q0 += batch) {
    const uint32_t nb = std::min(batch, nq - q0);
    const gg_status r = query_batch_device(c, d_sk, d_lens, n, d_q_sk + (uint64_t)q0 * c->s, d_q_lens + q0, nb, n + q0,
                                           d_cmin, d_sufmin, d_out, cap, d_count, st);
    if (r != GG_OK) return r;
  }
  return GG_OK;
}

gg_status query_rect_append_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                                   const uint64_t* d_q_sk, const uint32_t* d_q_lens, uint32_t nq, gg_pair* d_out,
                                   uint64_t cap, uint64_t* d_count, hipStream_t st) {
  // the named-pair kernel reads one matrix: the rows followed by the queries
  const uint32_t s = c->s, all = n + nq;
  uint64_t* d_cat;
  uint32_t* d_cat_len;
  gg_pair* d_list;
  const uint32_t rows_per_pass = (uint32_t)std::max<uint64_t>(1, (1ull << 24) / nq);
  GG_HIP(c, scratch_t(c, "qy_cat_sk", (size_t)all * s, &d_cat));
  GG_HIP(c, scratch_t(c, "qy_cat_len", (size_t)all, &d_cat_len));
  GG_HIP(c, scratch_t(c, "qy_list", (size_t)std::min(rows_per_pass, n) * nq, &d_list));
  GG_HIP(c, hipMemcpyAsync(d_cat, d_sk, (size_t)n * s * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  GG_HIP(c, hipMemcpyAsync(d_cat + (size_t)n * s, d_q_sk, (size_t)nq * s * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  GG_HIP(c, hipMemcpyAsync(d_cat_len, d_lens, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  GG_HIP(c, hipMemcpyAsync(d_cat_len + n, d_q_lens, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  unsigned long long* count = reinterpret_cast<unsigned long long*>(d_count);
  for (uint32_t i0 = 0; i0 < n; i0 += rows_per_pass) {
    const uint64_t m = (uint64_t)std::min(rows_per_pass, n - i0) * nq;
    hipLaunchKernelGGL(query_rect_kernel, dim3(grid_for(m)), dim3(kQueryBlock), 0, st, d_list, m, i0, n, nq);
    GG_HIP(c, hipGetLastError());
    const gg_status r = gg_ani_pairs_device(c, d_cat, d_cat_len, all, d_list, m, st);
    if (r != GG_OK) return r;
    hipLaunchKernelGGL(query_append_kernel, dim3(grid_for(m)), dim3(kQueryBlock), 0, st, (const gg_pair*)d_list, m, d_out,
                       cap, (const unsigned long long*)count);
    GG_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(query_count_kernel, dim3(1), dim3(1), 0, st, count, m);
    GG_HIP(c, hipGetLastError());
  }
  return GG_OK;
}

gg_status query_best_device(gg_ctx* c, uint32_t n, uint32_t nq, const gg_pair* d_pairs, const float* d_ani,
                            uint64_t n_pairs, const uint32_t* d_rank, gg_pair* d_best, float* d_best_ani, hipStream_t st) {
  if (nq == 0) return GG_OK;
  unsigned long long* d_key;
  GG_HIP(c, scratch_t(c, "qy_key", (size_t)nq, &d_key));
  GG_HIP(c, timed_launch(c, GG_KERNEL_CLUSTER, n_pairs, st, [&]() -> hipError_t {
    hipLaunchKernelGGL(query_best_init_kernel, dim3((nq + kQueryBlock - 1) / kQueryBlock), dim3(kQueryBlock), 0, st, n, nq,
                       d_key, d_best, d_best_ani);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n_pairs == 0) return e;
    hipLaunchKernelGGL(query_best_kernel, dim3(grid_for(n_pairs)), dim3(kQueryBlock), 0, st, n, nq, d_pairs, d_ani, n_pairs,
                       d_rank, d_key);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(query_best_write_kernel, dim3(grid_for(n_pairs)), dim3(kQueryBlock), 0, st, n, nq, d_pairs, d_ani,
                       n_pairs, d_rank, (const unsigned long long*)d_key, d_best, d_best_ani);
    return hipGetLastError();
  }));
  return GG_OK;
}

}  // namespace gg
