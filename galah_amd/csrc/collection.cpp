// A collection resident on the device (include/galahgpu.h):
// the sketch matrix, the passing pairs in (i, j) order and their f32 ANI stay
// in device memory between calls; genomes are added (the border of the new
// rows, merged into the list without a sort), removed (the pair list filtered
// and renumbered, the rows compacted in place) and clustered in any order
// (one relabel gather, then cluster_device).
//
// The collection owns its buffers (hipMalloc): the matrix, the lens, two pair
// buffers and two ANI buffers.  A new pair list is always built in the buffer
// that does not hold the current one and the two are swapped last; new rows
// are written past n and n is raised last: a call that fails leaves the
// collection as it was.  Everything that lives for one call (the border, its
// sort, flags, scans, the bounce buffer) is context scratch.  Every entry
// point acts on the context's first device and synchronises.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "collection_core.hpp"
#include "context.hpp"

using namespace gg;

namespace {

constexpr uint64_t kBounceBytes = 64ull << 20;

gg_ctx* first(gg_collection* c) { return primary(c->ctx); }

// the tail of every entry point: the message of a failure goes to the context given
gg_status finish(gg_collection* c, gg_status st) { return finish_call(c->ctx, first(c), st); }

// the rows' capacity raised to hold `need`: allocate new, copy, free old
gg_status reserve_rows(gg_collection* c, uint64_t need, hipStream_t st) {
  if (need <= c->row_cap) return GG_OK;
  gg_ctx* m = first(c);
  const bool growth = c->row_cap != 0;
  const uint64_t cap = std::min<uint64_t>(collection::grown(c->row_cap, need), (1ull << 31) - 1);
  uint64_t* sk = nullptr;
  uint32_t* lens = nullptr;
  hipError_t e = hipMalloc(&sk, (size_t)cap * m->s * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc(&lens, (size_t)cap * sizeof(uint32_t));
  if (e == hipSuccess && c->n) e = hipMemcpyAsync(sk, c->sk, (size_t)c->n * m->s * sizeof(uint64_t), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && c->n) e = hipMemcpyAsync(lens, c->lens, (size_t)c->n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    (void)hipFree(sk);
    (void)hipFree(lens);
    (void)hipGetLastError();
    return hip_fail(m, e, "gg_collection: growing the sketch matrix");
  }
  (void)hipFree(c->sk);
  (void)hipFree(c->lens);
  c->sk = sk;
  c->lens = lens;
  c->row_cap = (uint32_t)cap;
  if (growth) ++c->grows;
  return GG_OK;
}

// buffer `b` (not the current one unless the list is empty) raised to hold
// `need` pairs; its contents are not kept
gg_status reserve_pairs(gg_collection* c, int b, uint64_t need) {
  if (need <= c->pair_cap[b]) return GG_OK;
  gg_ctx* m = first(c);
  const bool growth = c->pair_cap[b] != 0;
  const uint64_t cap = collection::grown(c->pair_cap[b], need);
  (void)hipFree(c->pairs[b]);
  (void)hipFree(c->ani[b]);
  c->pairs[b] = nullptr;
  c->ani[b] = nullptr;
  c->pair_cap[b] = 0;
  hipError_t e = hipMalloc(&c->pairs[b], (size_t)cap * sizeof(gg_pair));
  if (e == hipSuccess) e = hipMalloc(&c->ani[b], (size_t)cap * sizeof(float));
  if (e != hipSuccess) {
    (void)hipFree(c->pairs[b]);
    c->pairs[b] = nullptr;
    (void)hipGetLastError();
    return hip_fail(m, e, "gg_collection: growing the pair list");
  }
  c->pair_cap[b] = cap;
  if (growth) ++c->grows;
  return GG_OK;
}

void release(gg_collection* c) {
  if (!c) return;
  if (hipSetDevice(first(c)->device) == hipSuccess) {
    (void)hipFree(c->sk);
    (void)hipFree(c->lens);
    for (int b = 0; b < 2; ++b) {
      (void)hipFree(c->pairs[b]);
      (void)hipFree(c->ani[b]);
    }
  }
  delete c;
}

gg_status create(gg_ctx* ctx, float min_ani, uint32_t reserve_r, uint64_t reserve_p, gg_collection** out) {
  gg_ctx* m = primary(ctx);
  if (std::isnan(min_ani)) return fail(m, GG_ERR_INVALID_ARG, "gg_collection_create: min_ani is NaN");
  if (reserve_r >= (1u << 31) || reserve_p >= (1ull << 31))
    return fail(m, GG_ERR_INVALID_ARG, "gg_collection_create: 2^31 genomes or pairs, or more");
  gg_status st = use_device(m);
  if (st != GG_OK) return st;
  gg_collection* c = new gg_collection;
  c->ctx = ctx;
  c->min_ani = min_ani;
  st = reserve_rows(c, reserve_r, m->stream);
  for (int b = 0; st == GG_OK && b < 2; ++b) st = reserve_pairs(c, b, reserve_p);
  if (st != GG_OK) {
    release(c);
    return st;
  }
  *out = c;
  return GG_OK;
}

// The rows d_sk / d_len (device, n_new of them) appended, and their border
// merged into the pair list.
gg_status add_rows_device(gg_collection* c, const char* who, const uint64_t* d_sk, const uint32_t* d_len, uint32_t n_new,
                          uint64_t* n_border, hipStream_t st) {
  gg_ctx* m = first(c);
  const uint32_t s = m->s, n_old = c->n;
  if ((uint64_t)n_old + n_new >= (1ull << 31)) return fail(m, GG_ERR_INVALID_ARG, std::string(who) + ": 2^31 genomes or more");
  const uint32_t n = n_old + n_new;
  gg_status r = reserve_rows(c, n, st);
  if (r != GG_OK) return r;
  // past n: not part of the collection until n is raised
  GG_HIP(m, hipMemcpyAsync(c->sk + (size_t)n_old * s, d_sk, (size_t)n_new * s * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  GG_HIP(m, hipMemcpyAsync(c->lens + n_old, d_len, (size_t)n_new * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  uint64_t cnt = 0;
  if (n >= 2) {
    // the border, routed as gg_pairs_border_device routes it, in sized passes
    const uint64_t all = (uint64_t)n_new * n_old + (uint64_t)n_new * (n_new - 1) / 2;
    const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(1 << 20, (uint64_t)n * 16), all);
    gg_pair* d_border = nullptr;
    uint32_t passes = 0;
    bool matrix = false;
    r = sized_pair_passes(
        m, who, "co_border", all, cap,
        [&](gg_pair* d_out, uint64_t pcap, uint64_t* d_count) {
          gg_status b = border_routed_append(m, who, c->sk, c->lens, n, n_old, c->min_ani, d_out, pcap, d_count, &matrix, st);
          if (b == GG_OK && !matrix)
            b = pairs_core(m, c->sk, c->lens, n, 0, gg_pair_tiles(n), c->min_ani, d_out, pcap, d_count, st, n_old);
          return b;
        },
        &d_border, &cnt, &passes, st);
    if (r != GG_OK) return r;
    if (cnt >= (1ull << 31)) return fail(m, GG_ERR_INVALID_ARG, std::string(who) + ": 2^31 pairs or more");
    count_pairs_path(m, matrix);
    if (c->n_pairs + cnt >= (1ull << 31)) return fail(m, GG_ERR_INVALID_ARG, std::string(who) + ": 2^31 pairs or more");
    if (cnt) {
      const uint32_t n_op = (uint32_t)c->n_pairs, n_bp = (uint32_t)cnt;
      gg_pair* d_sorted = nullptr;
      r = sorted_pairs_device(m, d_border, cnt, n, &d_sorted, st);
      if (r != GG_OK) return r;
      float* d_bani = nullptr;
      uint32_t* d_start = nullptr;  // [2 (n + 1)]: old boundaries, border boundaries
      GG_HIP(m, scratch_t(m, "co_bani", (size_t)cnt, &d_bani));
      GG_HIP(m, scratch_t(m, "co_start", 2 * ((size_t)n + 1), &d_start));
      r = ani_f32_device(m, d_sorted, cnt, d_bani, nullptr, nullptr, st);
      if (r != GG_OK) return r;
      const int to = c->n_pairs ? 1 - c->cur : c->cur;
      r = reserve_pairs(c, to, c->n_pairs + cnt);
      if (r != GG_OK) return r;
      GG_HIP(m, launch_collection_row_bounds(c->pairs[c->cur], n_op, d_start, d_sorted, n_bp, d_start + n + 1, n, st));
      GG_HIP(m, launch_collection_merge(c->pairs[c->cur], c->ani[c->cur], n_op, d_sorted, d_bani, n_bp, d_start,
                                        d_start + n + 1, n, c->pairs[to], c->ani[to], st));
      GG_HIP(m, hipStreamSynchronize(st));
      c->cur = to;
      c->n_pairs += cnt;
    }
  }
  GG_HIP(m, hipStreamSynchronize(st));
  c->n = n;
  if (n_border) *n_border = cnt;
  return GG_OK;
}

// GALAHGPU_TEST_COLLECTION_BATCH, read per call: source rows per batch of the
// row compaction (tests: many batches on small inputs)
uint32_t compaction_batch_rows(uint32_t s) {
  const uint32_t dflt = collection::batch_rows(kBounceBytes, s);
  const char* e = getenv("GALAHGPU_TEST_COLLECTION_BATCH");
  if (!e || !*e) return dflt;
  const unsigned long long v = strtoull(e, nullptr, 10);
  return v < 1 ? dflt : (uint32_t)std::min<unsigned long long>(v, dflt);
}

gg_status remove_rows(gg_collection* c, const uint32_t* rows, uint32_t cnt_rows, uint32_t* new_index_out) {
  gg_ctx* m = first(c);
  const uint32_t n = c->n, s = m->s;
  std::vector<uint8_t> keep(n, 1);
  for (uint32_t x = 0; x < cnt_rows; ++x) {
    if (rows[x] >= n) return fail(m, GG_ERR_INVALID_ARG, "gg_collection_remove: row index out of range");
    keep[rows[x]] = 0;
  }
  std::vector<uint32_t> below((size_t)n + 1), new_index(std::max(n, 1u));
  const uint32_t first_removed = collection::relabel_rows(keep.data(), n, below.data(), new_index.data());
  const uint32_t n_keep = below[n];
  if (first_removed < n) {
    gg_status r = use_device(m);
    if (r != GG_OK) return r;
    hipStream_t st = m->stream;
    // every allocation of the call, before anything changes
    const uint32_t B = compaction_batch_rows(s);
    const uint32_t bounce_rows = std::min(B, n - first_removed);
    const uint32_t n_op = (uint32_t)c->n_pairs;
    uint32_t *d_new, *d_flags = nullptr, *d_at = nullptr, *d_blens, *h_kept;
    uint64_t* d_bounce;
    void* d_tmp = nullptr;
    const size_t tmp_bytes = n_op ? collection_scan_tmp_bytes(n_op) : 0;
    GG_HIP(m, scratch_t(m, "co_new", (size_t)n, &d_new));
    GG_HIP(m, scratch_t(m, "co_bounce", (size_t)bounce_rows * s, &d_bounce));
    GG_HIP(m, scratch_t(m, "co_blens", (size_t)bounce_rows, &d_blens));
    GG_HIP(m, host_scratch_t(m, "co_kept", 1, &h_kept));
    GG_HIP(m, hipMemcpyAsync(d_new, new_index.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    // the pair list: filtered and renumbered into the other buffer
    uint32_t kept_pairs = 0;
    const int to = 1 - c->cur;
    if (n_op) {
      GG_HIP(m, scratch_t(m, "co_flags", (size_t)n_op + 1, &d_flags));
      GG_HIP(m, scratch_t(m, "co_at", (size_t)n_op + 1, &d_at));
      GG_HIP(m, scratch(m, "co_tmp", std::max<size_t>(tmp_bytes, 16), &d_tmp));
      GG_HIP(m, launch_collection_pair_scan(c->pairs[c->cur], n_op, n, d_new, d_flags, d_at, d_tmp, tmp_bytes, st));
      GG_HIP(m, hipMemcpyAsync(h_kept, d_at + n_op, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      GG_HIP(m, hipStreamSynchronize(st));
      kept_pairs = *h_kept;
      if (kept_pairs > n_op) return fail(m, GG_ERR_INTERNAL, "gg_collection_remove: bad survivor count");
      r = reserve_pairs(c, to, kept_pairs);
      if (r != GG_OK) return r;
      GG_HIP(m, launch_collection_pair_compact(c->pairs[c->cur], c->ani[c->cur], n_op, d_new, d_flags, d_at, kept_pairs,
                                               c->pairs[to], c->ani[to], st));
      GG_HIP(m, hipStreamSynchronize(st));
    }
    // the rows, in place: stream-ordered batches through the bounce buffer
    const uint32_t nb = collection::batch_count(first_removed, n, B);
    for (uint32_t b = 0; b < nb; ++b) {
      const collection::Batch x = collection::batch_of(b, first_removed, n, B, below.data());
      const uint32_t kept = x.dst1 - x.dst0;
      if (kept == 0) continue;
      GG_HIP(m, launch_collection_rows_gather(c->sk, c->lens, s, x.src0, x.src1, x.dst0, bounce_rows, d_new, d_bounce,
                                              d_blens, st));
      GG_HIP(m, hipMemcpyAsync(c->sk + (size_t)x.dst0 * s, d_bounce, (size_t)kept * s * sizeof(uint64_t),
                               hipMemcpyDeviceToDevice, st));
      GG_HIP(m, hipMemcpyAsync(c->lens + x.dst0, d_blens, (size_t)kept * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    }
    GG_HIP(m, hipStreamSynchronize(st));
    if (n_op) c->cur = to;
    c->n_pairs = kept_pairs;
    c->n = n_keep;
  }
  c->rows_moved = first_removed < n ? n_keep - first_removed : 0;
  if (new_index_out && n) memcpy(new_index_out, new_index.data(), (size_t)n * sizeof(uint32_t));
  return GG_OK;
}

gg_status cluster_rows(gg_collection* c, const uint32_t* order, float cluster_ani, uint32_t* rep_of) {
  gg_ctx* m = first(c);
  const uint32_t n = c->n;
  if (std::isnan(cluster_ani)) return fail(m, GG_ERR_INVALID_ARG, "gg_collection_cluster: cluster_ani is NaN");
  if (n && !rep_of) return fail(m, GG_ERR_INVALID_ARG, "gg_collection_cluster: null argument");
  if (order) {
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t x = 0; x < n; ++x) {
      if (order[x] >= n || seen[order[x]]) return fail(m, GG_ERR_INVALID_ARG, "gg_collection_cluster: order is not a permutation");
      seen[order[x]] = 1;
    }
  }
  if (n == 0) return GG_OK;
  gg_status r = use_device(m);
  if (r != GG_OK) return r;
  hipStream_t st = m->stream;
  const uint32_t n_op = (uint32_t)c->n_pairs;
  const gg_pair* d_pairs = c->pairs[c->cur];
  uint32_t* d_rep;
  GG_HIP(m, scratch_t(m, "co_rep", (size_t)n, &d_rep));
  if (order) {
    uint32_t *d_order, *d_pos;
    gg_pair* d_rel;
    GG_HIP(m, scratch_t(m, "co_order", 2 * (size_t)n, &d_order));
    d_pos = d_order + n;
    GG_HIP(m, scratch_t(m, "co_rel", (size_t)std::max(n_op, 1u), &d_rel));
    GG_HIP(m, hipMemcpyAsync(d_order, order, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    GG_HIP(m, launch_collection_relabel(d_order, n, d_pos, d_pairs, n_op, d_rel, st));
    d_pairs = d_rel;
  }
  r = cluster_device(m, n, d_pairs, c->ani[c->cur], n_op, cluster_ani, d_rep, st);
  if (r != GG_OK) return r;
  GG_HIP(m, hipMemcpyAsync(rep_of, d_rep, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  GG_HIP(m, hipStreamSynchronize(st));
  return GG_OK;
}

// host rows (checked) into context scratch, then add_rows_device
gg_status add_rows_host(gg_collection* c, const uint64_t* sketches, const uint32_t* lens, uint32_t n_new,
                        uint64_t* n_border) {
  gg_ctx* m = first(c);
  if (!sketches || !lens) return fail(m, GG_ERR_INVALID_ARG, "gg_collection_add_rows: null buffer");
  for (uint32_t g = 0; g < n_new; ++g)
    if (lens[g] > m->s) return fail(m, GG_ERR_INVALID_ARG, "gg_collection_add_rows: sketch longer than sketch_size");
  gg_status st = use_device(m);
  if (st != GG_OK) return st;
  uint64_t* d_sk;
  uint32_t* d_len;
  GG_HIP(m, scratch_t(m, "co_up_sk", (size_t)n_new * m->s, &d_sk));
  GG_HIP(m, scratch_t(m, "co_up_len", (size_t)n_new, &d_len));
  GG_HIP(m, hipMemcpyAsync(d_sk, sketches, (size_t)n_new * m->s * sizeof(uint64_t), hipMemcpyHostToDevice, m->stream));
  GG_HIP(m, hipMemcpyAsync(d_len, lens, (size_t)n_new * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
  return add_rows_device(c, "gg_collection_add_rows", d_sk, d_len, n_new, n_border, m->stream);
}

// a saved state into the buffers of a collection just created for it
gg_status load_state(gg_collection* c, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const gg_pair* pairs,
                     const float* ani, uint64_t n_pairs) {
  gg_ctx* m = first(c);
  hipStream_t s = m->stream;
  if (n) {
    GG_HIP(m, hipMemcpyAsync(c->sk, sketches, (size_t)n * m->s * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    GG_HIP(m, hipMemcpyAsync(c->lens, lens, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  }
  if (n_pairs) {
    GG_HIP(m, hipMemcpyAsync(c->pairs[0], pairs, (size_t)n_pairs * sizeof(gg_pair), hipMemcpyHostToDevice, s));
    GG_HIP(m, hipMemcpyAsync(c->ani[0], ani, (size_t)n_pairs * sizeof(float), hipMemcpyHostToDevice, s));
  }
  GG_HIP(m, hipStreamSynchronize(s));
  c->n = n;
  c->n_pairs = n_pairs;
  return GG_OK;
}

gg_status pairs_to_host(gg_collection* c, gg_pair** pairs, float** ani, uint64_t* n_out) {
  gg_ctx* m = first(c);
  gg_status st = use_device(m);
  if (st == GG_OK) st = copy_out(m, c->pairs[c->cur], c->n_pairs, pairs, m->stream);
  if (st == GG_OK) st = copy_out(m, c->ani[c->cur], c->n_pairs, ani, m->stream);
  if (st != GG_OK) return st;
  GG_HIP(m, hipStreamSynchronize(m->stream));
  *n_out = c->n_pairs;
  return GG_OK;
}

gg_status rows_to_host(gg_collection* c, uint64_t* sketches, uint32_t* lens) {
  gg_ctx* m = first(c);
  if (!sketches || !lens) return fail(m, GG_ERR_INVALID_ARG, "gg_collection_rows: null argument");
  const gg_status st = use_device(m);
  if (st != GG_OK) return st;
  GG_HIP(m, hipMemcpyAsync(sketches, c->sk, (size_t)c->n * m->s * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
  GG_HIP(m, hipMemcpyAsync(lens, c->lens, (size_t)c->n * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  GG_HIP(m, hipStreamSynchronize(m->stream));
  return GG_OK;
}

}  // namespace

extern "C" {

gg_status gg_collection_create(gg_ctx* ctx, float min_ani, uint32_t reserve_rows_, uint64_t reserve_pairs_,
                               gg_collection** out) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  if (!out) return fail(ctx, GG_ERR_INVALID_ARG, "gg_collection_create: null argument");
  *out = nullptr;
  return finish_call(ctx, primary(ctx), create(ctx, min_ani, reserve_rows_, reserve_pairs_, out));
}

void gg_collection_destroy(gg_collection* c) { release(c); }

gg_status gg_collection_stat(const gg_collection* c, gg_collection_info* info, float* min_ani) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  if (info) {
    const uint32_t s = primary(c->ctx)->s;
    info->n_pairs = c->n_pairs;
    info->pair_capacity = c->pair_cap[c->cur];
    info->device_bytes = (uint64_t)c->row_cap * ((uint64_t)s * sizeof(uint64_t) + sizeof(uint32_t)) +
                         (c->pair_cap[0] + c->pair_cap[1]) * (sizeof(gg_pair) + sizeof(float));
    info->n_rows = c->n;
    info->row_capacity = c->row_cap;
    info->grows = c->grows;
    info->rows_moved = c->rows_moved;
  }
  if (min_ani) *min_ani = c->min_ani;
  return GG_OK;
}

gg_status gg_collection_load(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const gg_pair* pairs,
                             const float* ani, uint64_t n_pairs, float min_ani, gg_collection** out) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  const std::string who = "gg_collection_load";
  if (!out || (n && (!sketches || !lens)) || (n_pairs && (!pairs || !ani)))
    return fail(ctx, GG_ERR_INVALID_ARG, who + ": null argument");
  *out = nullptr;
  gg_ctx* m = primary(ctx);
  if (n >= (1u << 31) || n_pairs >= (1ull << 31)) return fail(ctx, GG_ERR_INVALID_ARG, who + ": 2^31 genomes or pairs, or more");
  for (uint32_t g = 0; g < n; ++g)
    if (lens[g] > m->s) return fail(ctx, GG_ERR_INVALID_ARG, who + ": sketch longer than sketch_size");
  for (uint64_t p = 0; p < n_pairs; ++p) {
    const gg_pair& x = pairs[p];
    if (!(x.i < x.j && x.j < n)) return fail(ctx, GG_ERR_INVALID_ARG, who + ": a pair is not i < j < n");
    if (p && !(pairs[p - 1].i < x.i || (pairs[p - 1].i == x.i && pairs[p - 1].j < x.j)))
      return fail(ctx, GG_ERR_INVALID_ARG, who + ": the pairs are not strictly ascending by (i, j)");
    if (std::isnan(ani[p])) return fail(ctx, GG_ERR_INVALID_ARG, who + ": NaN ANI");
  }
  gg_collection* c = nullptr;
  gg_status st = create(ctx, min_ani, n, n_pairs, &c);
  if (st == GG_OK) st = load_state(c, sketches, lens, n, pairs, ani, n_pairs);
  if (st == GG_OK) *out = c;
  return finish_call(ctx, m, st, [&] { release(c); });
}

gg_status gg_collection_add_rows_device(gg_collection* c, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n_new,
                                        uint64_t* n_border, void* stream) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  if (n_border) *n_border = 0;
  if (n_new == 0) return GG_OK;
  gg_ctx* m = first(c);
  if (!d_sketches || !d_lens) return finish(c, fail(m, GG_ERR_INVALID_ARG, "gg_collection_add_rows_device: null buffer"));
  gg_status st = use_device(m);
  if (st == GG_OK) st = add_rows_device(c, "gg_collection_add_rows_device", d_sketches, d_lens, n_new, n_border, (hipStream_t)stream);
  return finish(c, st);
}

gg_status gg_collection_add_rows(gg_collection* c, const uint64_t* sketches, const uint32_t* lens, uint32_t n_new,
                                 uint64_t* n_border) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  if (n_border) *n_border = 0;
  if (n_new == 0) return GG_OK;
  return finish(c, add_rows_host(c, sketches, lens, n_new, n_border));
}

gg_status gg_collection_add_files(gg_collection* c, const char* const* paths, uint32_t n_new, const char* cache_dir,
                                  uint64_t* n_border) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  if (n_border) *n_border = 0;
  if (n_new == 0) return GG_OK;
  gg_ctx* m = first(c);
  if (!paths) return finish(c, fail(m, GG_ERR_INVALID_ARG, "gg_collection_add_files: null argument"));
  if ((uint64_t)c->n + n_new >= (1ull << 31))
    return finish(c, fail(m, GG_ERR_INVALID_ARG, "gg_collection_add_files: 2^31 genomes or more"));
  // only file bytes go up: the rows are sketched into context scratch on the
  // device and copied from there into the matrix
  const uint64_t* d_sk = nullptr;
  const uint32_t* d_len = nullptr;
  const gg_status st = sketch_files_first(c->ctx, paths, n_new, cache_dir, &d_sk, &d_len);
  if (st != GG_OK) return st;  // (reported on the context given)
  return finish(c, add_rows_device(c, "gg_collection_add_files", d_sk, d_len, n_new, n_border, m->stream));
}

gg_status gg_collection_remove(gg_collection* c, const uint32_t* rows, uint32_t m_rows, uint32_t* new_index) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  if (m_rows && !rows) return finish(c, fail(first(c), GG_ERR_INVALID_ARG, "gg_collection_remove: null argument"));
  return finish(c, remove_rows(c, rows, m_rows, new_index));
}

gg_status gg_collection_cluster(gg_collection* c, const uint32_t* order, float cluster_ani, uint32_t* rep_of) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  return finish(c, cluster_rows(c, order, cluster_ani, rep_of));
}

gg_status gg_collection_pairs(gg_collection* c, gg_pair** pairs, float** ani, uint64_t* n_out) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  gg_ctx* m = first(c);
  if (!pairs || !ani || !n_out) return finish(c, fail(m, GG_ERR_INVALID_ARG, "gg_collection_pairs: null argument"));
  *pairs = nullptr;
  *ani = nullptr;
  *n_out = 0;
  const gg_status st = pairs_to_host(c, pairs, ani, n_out);
  if (st != GG_OK) free_out(pairs, ani);
  return finish(c, st);
}

gg_status gg_collection_rows(gg_collection* c, uint64_t* sketches, uint32_t* lens) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  if (c->n == 0) return GG_OK;
  return finish(c, rows_to_host(c, sketches, lens));
}

gg_status gg_collection_view(gg_collection* c, const uint64_t** d_sketches, const uint32_t** d_lens, const gg_pair** d_pairs,
                             const float** d_ani) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  if (d_sketches) *d_sketches = c->sk;
  if (d_lens) *d_lens = c->lens;
  if (d_pairs) *d_pairs = c->pairs[c->cur];
  if (d_ani) *d_ani = c->ani[c->cur];
  return GG_OK;
}

}  // extern "C"
