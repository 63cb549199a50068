// Clustering from resident sketches: the rows of a sketch
// matrix in device memory to rep_of in device memory, the pair list never
// leaving it.  What gg_pairs + gg_ani_f32 + gg_cluster_pairs give, chained
// from their device forms:
//
//   1. K2 (pairs_core) over every tile into context scratch, sized as
//      pairs_range_to_host sizes it: max(2^20, 16 n) pairs clipped to
//      n (n - 1) / 2, the count word read back, one retry at the exact count;
//   2. no sort: neither the clustering rules nor the partition depend on the
//      order of the pairs;
//   3. the f32 ANI of every pair (ani_f32_device), then cluster_device;
//   4. for the summary, the partition of preclusters_device (no local pairs):
//      the number of sets and the size of the first, which is the largest.
#include <algorithm>
#include <cmath>

#include "context.hpp"

namespace gg {

gg_status pairs_rows_device(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                            float min_ani, gg_pair** d_pairs, uint64_t* n_pairs, uint32_t* n_passes, hipStream_t st) {
  gg_pair* d_out = nullptr;
  uint64_t cnt = 0;
  uint32_t passes = 0;
  *d_pairs = nullptr;
  *n_pairs = 0;
  *n_passes = 0;
  if (n < 2) return GG_OK;
  uint64_t *d_count, *h_count;
  GG_HIP(c, scratch_t(c, "rs_count", 1, &d_count));
  GG_HIP(c, host_scratch_t(c, "rs_count", 1, &h_count));
  const uint64_t all = (uint64_t)n * (n - 1) / 2;
  uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(1 << 20, (uint64_t)n * 16), all);
  for (;;) {
    if (passes == 2) return fail(c, GG_ERR_INTERNAL, std::string(who) + ": pair output sizing failed");
    GG_HIP(c, scratch_t(c, "rs_pairs", (size_t)cap, &d_out));
    GG_HIP(c, hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
    const gg_status ps = pairs_core(c, d_sk, d_lens, n, 0, gg_pair_tiles(n), min_ani, d_out, cap, d_count, st);
    if (ps != GG_OK) return ps;
    ++passes;
    GG_HIP(c, hipMemcpyAsync(h_count, d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    GG_HIP(c, hipStreamSynchronize(st));
    cnt = *h_count;
    if (cnt > all) return fail(c, GG_ERR_INTERNAL, std::string(who) + ": bad pair count");
    if (cnt <= cap) break;
    cap = cnt;
  }
  if (cnt >= (1ull << 31)) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": 2^31 pairs or more");
  *d_pairs = d_out;
  *n_pairs = cnt;
  *n_passes = passes;
  return GG_OK;
}

gg_status cluster_rows_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n, float min_ani,
                              float T, uint32_t* d_rep_of, gg_cluster_summary* sum, const gg_pair** d_pairs,
                              const float** d_ani, hipStream_t st) {
  if (sum) *sum = gg_cluster_summary{};
  if (d_pairs) *d_pairs = nullptr;
  if (d_ani) *d_ani = nullptr;
  if (n == 0) return GG_OK;
  gg_pair* d_out = nullptr;
  float* d_val = nullptr;
  uint64_t cnt = 0;
  uint32_t passes = 0;
  gg_status s = pairs_rows_device(c, "gg_cluster_rows_device", d_sk, d_lens, n, min_ani, &d_out, &cnt, &passes, st);
  if (s != GG_OK) return s;
  uint64_t rechecked = 0;
  GG_HIP(c, scratch_t(c, "rs_ani", (size_t)std::max<uint64_t>(cnt, 1), &d_val));
  s = ani_f32_device(c, d_out, cnt, d_val, nullptr, &rechecked, st);
  if (s != GG_OK) return s;
  s = cluster_device(c, n, d_out, d_val, cnt, T, d_rep_of, st);
  if (s != GG_OK) return s;
  if (sum) {
    uint32_t *d_members, *d_offsets, *h_off, n_sets = 0;
    GG_HIP(c, scratch_t(c, "rs_members", (size_t)n, &d_members));
    GG_HIP(c, scratch_t(c, "rs_offsets", (size_t)n + 1, &d_offsets));
    GG_HIP(c, host_scratch_t(c, "rs_offsets", 2, &h_off));
    s = preclusters_device(c, n, d_out, cnt, d_members, d_offsets, &n_sets, nullptr, nullptr, st);
    if (s != GG_OK) return s;
    GG_HIP(c, hipMemcpyAsync(h_off, d_offsets, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GG_HIP(c, hipStreamSynchronize(st));
    sum->n_pairs = cnt;
    sum->ani_rechecked = rechecked;
    sum->n_preclusters = n_sets;
    sum->largest_precluster = h_off[1] - h_off[0];
    sum->pair_passes = passes;
  }
  if (d_pairs) *d_pairs = d_out;
  if (d_ani) *d_ani = d_val;
  return GG_OK;
}

}  // namespace gg

using namespace gg;

extern "C" {

gg_status gg_cluster_rows_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                                 float min_ani, float cluster_ani, uint32_t* d_rep_of, gg_cluster_summary* summary,
                                 const gg_pair** d_pairs, const float** d_ani, void* stream) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* m = primary(ctx);
  gg_status st = GG_OK;
  if (n && (!d_sketches || !d_lens || !d_rep_of))
    st = fail(m, GG_ERR_INVALID_ARG, "gg_cluster_rows_device: null buffer");
  else if (std::isnan(min_ani) || std::isnan(cluster_ani))
    st = fail(m, GG_ERR_INVALID_ARG, "gg_cluster_rows_device: min_ani or cluster_ani is NaN");
  else if (n >= (1u << 31))
    st = fail(m, GG_ERR_INVALID_ARG, "gg_cluster_rows_device: 2^31 genomes or more");
  else if (hipSetDevice(m->device) != hipSuccess)
    st = fail(m, GG_ERR_HIP, "hipSetDevice failed");
  else
    st = cluster_rows_device(m, d_sketches, d_lens, n, min_ani, cluster_ani, d_rep_of, summary, d_pairs, d_ani,
                             (hipStream_t)stream);
  if (st != GG_OK) {
    if (summary) *summary = gg_cluster_summary{};
    if (d_pairs) *d_pairs = nullptr;
    if (d_ani) *d_ani = nullptr;
    if (m != ctx) ctx->err = m->err;
  }
  return st;
}

}  // extern "C"
