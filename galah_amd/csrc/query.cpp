// Querying resident rows and a resident collection (include/galahgpu.h, "the
// query"): the passing cells (row i, query q) of n rows and nq
// queries that are not to be added, so that
//   gg_query(rows, queries, min_ani)
//     == [p for p in gg_pairs_border(rows ++ queries, n_old = n, min_ani) if p.i < n]
// in content and order, and the best candidate of every query by
// query_core.hpp's key.  No query x query cell is evaluated, min_ani is the
// call's own, and a collection is only read: everything that lives for the
// call is context scratch.  Every entry point acts on the context's first
// device.  gg_pair_paths, gg_pairs_paths_taken and gg_fallbacks do not count a
// query: it is not a pair-kernel call over tiles.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "context.hpp"
#include "query_core.hpp"
#include "validate_core.hpp"

using namespace gg;

namespace {

constexpr uint64_t kLimit = 1ull << 31;

// GALAHGPU_TEST_QUERY_BATCH, read per call: queries per table and launch of
// the stream kernel (tests: many batches on small inputs); never above the default
uint32_t query_batch(uint32_t s) {
  const uint32_t dflt = query::batch_queries(s);
  const char* e = getenv("GALAHGPU_TEST_QUERY_BATCH");
  if (!e || !*e) return dflt;
  const unsigned long long v = strtoull(e, nullptr, 10);
  return v < 1 ? dflt : (uint32_t)std::min<unsigned long long>(v, dflt);
}

// the cells appended to d_out by gg_pairs_device's contract (n, nq >= 1)
gg_status query_append(gg_ctx* m, const uint64_t* d_sk, const uint32_t* d_len, uint32_t n, const uint64_t* d_q,
                       const uint32_t* d_qlen, uint32_t nq, float min_ani, gg_pair* d_out, uint64_t cap, uint64_t* d_count,
                       hipStream_t st) {
  uint32_t *d_cmin, *d_sufmin;
  const gg_status t = pairs_tables(m, min_ani, &d_cmin, &d_sufmin, st);
  if (t != GG_OK) return t;
  if (m->sufmin_host[0] == 0)  // a pair without a shared hash passes: min_ani <= 0, every cell does
    return query_rect_append_device(m, d_sk, d_len, n, d_q, d_qlen, nq, d_out, cap, d_count, st);
  return query_append_device(m, d_sk, d_len, n, d_q, d_qlen, nq, query_batch(m->s), d_cmin, d_sufmin, d_out, cap, d_count,
                             st);
}

// The hits in context scratch with their f32 ANI: sized passes as
// add_rows_device sizes the border; sorted by (i, j) when asked.  Synchronises st.
gg_status query_hits(gg_ctx* m, const std::string& who, const uint64_t* d_sk, const uint32_t* d_len, uint32_t n,
                     const uint64_t* d_q, const uint32_t* d_qlen, uint32_t nq, float min_ani, bool sorted,
                     const gg_pair** d_hits, const float** d_ani, uint64_t* cnt, hipStream_t st) {
  *d_hits = nullptr;
  *d_ani = nullptr;
  *cnt = 0;
  if (n == 0 || nq == 0) return GG_OK;
  const uint64_t all = (uint64_t)n * nq;
  const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(1 << 20, ((uint64_t)n + nq) * 16), all);
  gg_pair* d_out = nullptr;
  uint32_t passes = 0;
  gg_status r = sized_pair_passes(
      m, who, "qy_hits", all, cap,
      [&](gg_pair* d_o, uint64_t pcap, uint64_t* d_count) {
        return query_append(m, d_sk, d_len, n, d_q, d_qlen, nq, min_ani, d_o, pcap, d_count, st);
      },
      &d_out, cnt, &passes, st);
  if (r != GG_OK) return r;
  if (*cnt >= kLimit) return fail(m, GG_ERR_INVALID_ARG, who + ": 2^31 pairs or more");
  if (*cnt == 0) return GG_OK;
  if (sorted) {
    gg_pair* d_sorted = nullptr;
    r = sorted_pairs_device(m, d_out, *cnt, n + nq, &d_sorted, st);
    if (r != GG_OK) return r;
    d_out = d_sorted;
  }
  float* d_a = nullptr;
  GG_HIP(m, scratch_t(m, "qy_ani", (size_t)*cnt, &d_a));
  r = ani_f32_device(m, d_out, *cnt, d_a, nullptr, nullptr, st);
  if (r != GG_OK) return r;
  *d_hits = d_out;
  *d_ani = d_a;
  return GG_OK;
}

// host rows into context scratch
gg_status upload_rows(gg_ctx* m, const char* key_sk, const char* key_len, const uint64_t* sketches, const uint32_t* lens,
                      uint32_t n, const uint64_t** d_sk, const uint32_t** d_len, hipStream_t st) {
  uint64_t* sk = nullptr;
  uint32_t* ln = nullptr;
  GG_HIP(m, scratch_t(m, key_sk, (size_t)std::max(n, 1u) * m->s, &sk));
  GG_HIP(m, scratch_t(m, key_len, (size_t)std::max(n, 1u), &ln));
  if (n) {
    GG_HIP(m, hipMemcpyAsync(sk, sketches, (size_t)n * m->s * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    GG_HIP(m, hipMemcpyAsync(ln, lens, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  *d_sk = sk;
  *d_len = ln;
  return GG_OK;
}

// pairs and ANI to library-owned host arrays
gg_status hits_to_host(gg_ctx* m, const gg_pair* d_hits, const float* d_ani, uint64_t cnt, gg_pair** pairs, float** ani,
                       uint64_t* n_out, hipStream_t st) {
  gg_status r = copy_out(m, d_hits, cnt, pairs, st);
  if (r == GG_OK) r = copy_out(m, d_ani, cnt, ani, st);
  if (r != GG_OK) return r;
  GG_HIP(m, hipStreamSynchronize(st));
  *n_out = cnt;
  return GG_OK;
}

gg_status check_lens(gg_ctx* m, const std::string& who, const uint32_t* lens, uint32_t n) {
  for (uint32_t g = 0; g < n; ++g)
    if (lens[g] > m->s) return fail(m, GG_ERR_INVALID_ARG, who + ": sketch longer than sketch_size");
  return GG_OK;
}

// rank [n] (null: every row, by its index): the candidates' ranks are distinct
bool ranks_distinct(const uint32_t* rank, uint32_t n) {
  if (!rank) return true;
  std::vector<uint32_t> r;
  for (uint32_t i = 0; i < n; ++i)
    if (rank[i] != query::kNotCandidate) r.push_back(rank[i]);
  std::sort(r.begin(), r.end());
  return std::adjacent_find(r.begin(), r.end()) == r.end();
}

gg_status query_rows_ctx(gg_ctx* m, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint64_t* q_sketches,
                         const uint32_t* q_lens, uint32_t nq, float min_ani, gg_pair** pairs, float** ani,
                         uint64_t* n_out) {
  const std::string who = "gg_query_rows";
  gg_status r = check_lens(m, who, lens, n);
  if (r == GG_OK) r = check_lens(m, who, q_lens, nq);
  if (r == GG_OK) r = use_device(m);
  if (r != GG_OK) return r;
  hipStream_t st = m->stream;
  const uint64_t *d_sk, *d_q;
  const uint32_t *d_len, *d_qlen;
  const gg_pair* d_hits;
  const float* d_ani;
  uint64_t cnt = 0;
  r = upload_rows(m, "qy_up_sk", "qy_up_len", sketches, lens, n, &d_sk, &d_len, st);
  if (r == GG_OK) r = upload_rows(m, "qy_up_q", "qy_up_qlen", q_sketches, q_lens, nq, &d_q, &d_qlen, st);
  if (r == GG_OK) r = query_hits(m, who, d_sk, d_len, n, d_q, d_qlen, nq, min_ani, true, &d_hits, &d_ani, &cnt, st);
  if (r == GG_OK) r = hits_to_host(m, d_hits, d_ani, cnt, pairs, ani, n_out, st);
  return r;
}

// the queries (device rows of the collection's first member) against the collection
gg_status collection_query(gg_collection* c, const std::string& who, const uint64_t* d_q, const uint32_t* d_qlen,
                           uint32_t nq, float min_ani, gg_pair** pairs, float** ani, uint64_t* n_out) {
  gg_ctx* m = primary(c->ctx);
  const gg_pair* d_hits;
  const float* d_ani;
  uint64_t cnt = 0;
  gg_status r = query_hits(m, who, c->sk, c->lens, c->n, d_q, d_qlen, nq, min_ani, true, &d_hits, &d_ani, &cnt, m->stream);
  if (r == GG_OK) r = hits_to_host(m, d_hits, d_ani, cnt, pairs, ani, n_out, m->stream);
  return r;
}

// ... at the collection's min_ani: only best / best_ani come down
gg_status collection_classify(gg_collection* c, const std::string& who, const uint64_t* d_q, const uint32_t* d_qlen,
                              uint32_t nq, const uint32_t* rank, gg_pair* best, float* best_ani) {
  gg_ctx* m = primary(c->ctx);
  hipStream_t st = m->stream;
  const uint32_t n = c->n;
  const gg_pair* d_hits;
  const float* d_ani;
  uint64_t cnt = 0;
  gg_status r = query_hits(m, who, c->sk, c->lens, n, d_q, d_qlen, nq, c->min_ani, false, &d_hits, &d_ani, &cnt, st);
  if (r != GG_OK) return r;
  uint32_t* d_rank = nullptr;
  gg_pair* d_best;
  float* d_best_ani;
  if (rank && n) {
    GG_HIP(m, scratch_t(m, "qy_rank", (size_t)n, &d_rank));
    GG_HIP(m, hipMemcpyAsync(d_rank, rank, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  GG_HIP(m, scratch_t(m, "qy_best", (size_t)nq, &d_best));
  GG_HIP(m, scratch_t(m, "qy_best_ani", (size_t)nq, &d_best_ani));
  r = query_best_device(m, n, nq, d_hits, d_ani, cnt, d_rank, d_best, d_best_ani, st);
  if (r != GG_OK) return r;
  GG_HIP(m, hipMemcpyAsync(best, d_best, (size_t)nq * sizeof(gg_pair), hipMemcpyDeviceToHost, st));
  GG_HIP(m, hipMemcpyAsync(best_ani, d_best_ani, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost, st));
  GG_HIP(m, hipStreamSynchronize(st));
  return GG_OK;
}

gg_status finish(gg_collection* c, gg_status st) { return finish_call(c->ctx, primary(c->ctx), st); }

// what every collection query checks before any work (the message on the first member)
gg_status check_collection_query(gg_collection* c, const std::string& who, uint32_t nq, bool nulls, float min_ani) {
  gg_ctx* m = primary(c->ctx);
  if (nulls) return fail(m, GG_ERR_INVALID_ARG, who + ": null argument");
  if (std::isnan(min_ani)) return fail(m, GG_ERR_INVALID_ARG, who + ": min_ani is NaN");
  if ((uint64_t)c->n + nq >= kLimit) return fail(m, GG_ERR_INVALID_ARG, who + ": 2^31 genomes or more");
  return GG_OK;
}

}  // namespace

extern "C" {

gg_status gg_query_host(const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint64_t* q_sketches,
                        const uint32_t* q_lens, uint32_t nq, uint32_t sketch_size, int kmer_length, float min_ani,
                        gg_pair** out, uint64_t* n_out) {
  std::string err;
  if (!out || !n_out || (n && (!sketches || !lens)) || (nq && (!q_sketches || !q_lens)))
    err = "gg_query_host: null buffer";
  else if (std::isnan(min_ani))
    err = "min_ani is NaN";
  else if (kmer_length < 1 || kmer_length > 32 || sketch_size < 1)
    err = "gg_query_host: kmer_length must be 1..32 and sketch_size at least 1";
  else if ((uint64_t)n + nq >= kLimit)
    err = "gg_query_host: 2^31 genomes or more";
  for (uint32_t g = 0; err.empty() && g < n; ++g)
    if (lens[g] > sketch_size) err = "gg_query_host: sketch longer than sketch_size";
  for (uint32_t g = 0; err.empty() && g < nq; ++g)
    if (q_lens[g] > sketch_size) err = "gg_query_host: sketch longer than sketch_size";
  if (!err.empty()) {
    set_thread_error(err);
    return GG_ERR_INVALID_ARG;
  }
  *out = nullptr;
  *n_out = 0;
  const std::vector<uint32_t> cmin = build_cmin(sketch_size, kmer_length, min_ani);
  std::vector<gg_pair> res;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t q = 0; q < nq; ++q) {
      uint32_t common, total;
      validate::merge_counts(sketches + (size_t)i * sketch_size, lens[i], q_sketches + (size_t)q * sketch_size, q_lens[q],
                             &common, &total);
      if (total < cmin.size() && common >= cmin[total]) res.push_back(gg_pair{i, n + q, common, total});
    }
  if (res.size() >= kLimit) {
    set_thread_error("gg_query_host: 2^31 pairs or more");
    return GG_ERR_INVALID_ARG;
  }
  *out = copy_out(res);
  if (!*out) {
    set_thread_error("out of host memory");
    return GG_ERR_OUT_OF_MEMORY;
  }
  *n_out = res.size();
  return GG_OK;
}

gg_status gg_query_rows(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint64_t* q_sketches,
                        const uint32_t* q_lens, uint32_t nq, float min_ani, gg_pair** pairs, float** ani, uint64_t* n_out) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  if (!pairs || !ani || !n_out || (n && (!sketches || !lens)) || (nq && (!q_sketches || !q_lens)))
    return fail(ctx, GG_ERR_INVALID_ARG, "gg_query_rows: null buffer");
  if (std::isnan(min_ani)) return fail(ctx, GG_ERR_INVALID_ARG, "min_ani is NaN");
  if ((uint64_t)n + nq >= kLimit) return fail(ctx, GG_ERR_INVALID_ARG, "gg_query_rows: 2^31 genomes or more");
  *pairs = nullptr;
  *ani = nullptr;
  *n_out = 0;
  gg_ctx* m = primary(ctx);
  const gg_status st = query_rows_ctx(m, sketches, lens, n, q_sketches, q_lens, nq, min_ani, pairs, ani, n_out);
  return finish_call(ctx, m, st, [&] { free_out(pairs, ani); });
}

gg_status gg_query_rows_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                               const uint64_t* d_q_sketches, const uint32_t* d_q_lens, uint32_t nq, float min_ani,
                               gg_pair* d_out, uint64_t out_cap, uint64_t* d_count, void* stream) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  if (std::isnan(min_ani)) return fail(ctx, GG_ERR_INVALID_ARG, "min_ani is NaN");
  if ((uint64_t)n + nq >= kLimit) return fail(ctx, GG_ERR_INVALID_ARG, "gg_query_rows_device: 2^31 genomes or more");
  if (n == 0 || nq == 0) return GG_OK;
  if (!d_sketches || !d_lens || !d_q_sketches || !d_q_lens || !d_count || (out_cap && !d_out))
    return fail(ctx, GG_ERR_INVALID_ARG, "gg_query_rows_device: null buffer");
  gg_ctx* m = primary(ctx);
  gg_status st = use_device(m);
  if (st == GG_OK)
    st = query_append(m, d_sketches, d_lens, n, d_q_sketches, d_q_lens, nq, min_ani, d_out, out_cap, d_count,
                      (hipStream_t)stream);
  return finish_call(ctx, m, st);
}

gg_status gg_query_best_host(uint32_t n, uint32_t nq, const gg_pair* pairs, const float* ani, uint64_t n_pairs,
                             const uint32_t* rank, gg_pair* best, float* best_ani) {
  std::string err;
  if ((n_pairs && (!pairs || !ani)) || (nq && (!best || !best_ani)))
    err = "gg_query_best_host: null argument";
  else if ((uint64_t)n + nq >= kLimit)
    err = "gg_query_best_host: 2^31 genomes or more";
  else if (!ranks_distinct(rank, n))
    err = "gg_query_best_host: two candidates of one rank";
  for (uint64_t p = 0; err.empty() && p < n_pairs; ++p) {
    if (pairs[p].i >= n || pairs[p].j < n || pairs[p].j - n >= nq)
      err = "gg_query_best_host: pair index out of range";
    else if (std::isnan(ani[p]))
      err = "gg_query_best_host: NaN ani";
  }
  if (!err.empty()) {
    set_thread_error(err);
    return GG_ERR_INVALID_ARG;
  }
  std::vector<uint64_t> key(nq, 0);
  for (uint32_t q = 0; q < nq; ++q) {
    best[q] = gg_pair{query::kNoHit, n + q, 0, 0};
    best_ani[q] = 0.0f;
  }
  for (uint64_t p = 0; p < n_pairs; ++p) {
    const uint32_t r = rank ? rank[pairs[p].i] : pairs[p].i;
    if (r == query::kNotCandidate) continue;
    const uint32_t q = pairs[p].j - n;
    const uint64_t k = query::best_key(ani[p], r);
    if (k > key[q]) {
      key[q] = k;
      best[q] = pairs[p];
      best_ani[q] = ani[p];
    }
  }
  return GG_OK;
}

gg_status gg_query_best_device(gg_ctx* ctx, uint32_t n, uint32_t nq, const gg_pair* d_pairs, const float* d_ani,
                               uint64_t n_pairs, const uint32_t* d_rank, gg_pair* d_best, float* d_best_ani, void* stream) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  if ((n_pairs && (!d_pairs || !d_ani)) || (nq && (!d_best || !d_best_ani)))
    return fail(ctx, GG_ERR_INVALID_ARG, "gg_query_best_device: null buffer");
  if ((uint64_t)n + nq >= kLimit) return fail(ctx, GG_ERR_INVALID_ARG, "gg_query_best_device: 2^31 genomes or more");
  gg_ctx* m = primary(ctx);
  gg_status st = use_device(m);
  if (st == GG_OK) st = query_best_device(m, n, nq, d_pairs, d_ani, n_pairs, d_rank, d_best, d_best_ani, (hipStream_t)stream);
  return finish_call(ctx, m, st);
}

gg_status gg_collection_query_rows(gg_collection* c, const uint64_t* q_sketches, const uint32_t* q_lens, uint32_t nq,
                                   float min_ani, gg_pair** pairs, float** ani, uint64_t* n_out) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  const std::string who = "gg_collection_query_rows";
  gg_ctx* m = primary(c->ctx);
  gg_status st = check_collection_query(c, who, nq, !pairs || !ani || !n_out || (nq && (!q_sketches || !q_lens)), min_ani);
  if (st == GG_OK) st = check_lens(m, who, q_lens, nq);
  if (st != GG_OK) return finish(c, st);
  *pairs = nullptr;
  *ani = nullptr;
  *n_out = 0;
  const uint64_t* d_q;
  const uint32_t* d_qlen;
  st = use_device(m);
  if (st == GG_OK) st = upload_rows(m, "qy_up_q", "qy_up_qlen", q_sketches, q_lens, nq, &d_q, &d_qlen, m->stream);
  if (st == GG_OK) st = collection_query(c, who, d_q, d_qlen, nq, min_ani, pairs, ani, n_out);
  if (st != GG_OK) free_out(pairs, ani);
  return finish(c, st);
}

gg_status gg_collection_query_files(gg_collection* c, const char* const* paths, uint32_t nq, const char* cache_dir,
                                    float min_ani, uint64_t* q_hashes, uint32_t* q_lens, gg_pair** pairs, float** ani,
                                    uint64_t* n_out) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  const std::string who = "gg_collection_query_files";
  gg_ctx* m = primary(c->ctx);
  gg_status st = check_collection_query(c, who, nq, !pairs || !ani || !n_out || (nq && !paths), min_ani);
  if (st != GG_OK) return finish(c, st);
  *pairs = nullptr;
  *ani = nullptr;
  *n_out = 0;
  if (nq == 0) return GG_OK;
  // the files sketched as gg_collection_add_files sketches them, into context scratch
  const uint64_t* d_q = nullptr;
  const uint32_t* d_qlen = nullptr;
  st = sketch_files_first(c->ctx, paths, nq, cache_dir, &d_q, &d_qlen);
  if (st != GG_OK) return st;  // (reported on the context given)
  st = collection_query(c, who, d_q, d_qlen, nq, min_ani, pairs, ani, n_out);
  // the hashes visit the host only when the caller asks for them
  if (st == GG_OK && q_hashes)
    st = hipMemcpy(q_hashes, d_q, (size_t)nq * m->s * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess
             ? GG_OK
             : fail(m, GG_ERR_HIP, who + ": copying the hashes");
  if (st == GG_OK && q_lens)
    st = hipMemcpy(q_lens, d_qlen, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess
             ? GG_OK
             : fail(m, GG_ERR_HIP, who + ": copying the lens");
  if (st != GG_OK) {
    free_out(pairs, ani);
    *n_out = 0;
  }
  return finish(c, st);
}

gg_status gg_collection_classify_rows(gg_collection* c, const uint64_t* q_sketches, const uint32_t* q_lens, uint32_t nq,
                                      const uint32_t* rank, gg_pair* best, float* best_ani) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  const std::string who = "gg_collection_classify_rows";
  gg_ctx* m = primary(c->ctx);
  gg_status st = check_collection_query(c, who, nq, nq && (!q_sketches || !q_lens || !best || !best_ani), c->min_ani);
  if (st == GG_OK) st = check_lens(m, who, q_lens, nq);
  if (st == GG_OK && !ranks_distinct(rank, c->n)) st = fail(m, GG_ERR_INVALID_ARG, who + ": two candidates of one rank");
  if (st != GG_OK || nq == 0) return finish(c, st);
  const uint64_t* d_q;
  const uint32_t* d_qlen;
  st = use_device(m);
  if (st == GG_OK) st = upload_rows(m, "qy_up_q", "qy_up_qlen", q_sketches, q_lens, nq, &d_q, &d_qlen, m->stream);
  if (st == GG_OK) st = collection_classify(c, who, d_q, d_qlen, nq, rank, best, best_ani);
  return finish(c, st);
}

gg_status gg_collection_classify_files(gg_collection* c, const char* const* paths, uint32_t nq, const char* cache_dir,
                                       const uint32_t* rank, gg_pair* best, float* best_ani) {
  if (!c) return fail(nullptr, GG_ERR_INVALID_ARG, "null collection");
  const std::string who = "gg_collection_classify_files";
  gg_ctx* m = primary(c->ctx);
  gg_status st = check_collection_query(c, who, nq, nq && (!paths || !best || !best_ani), c->min_ani);
  if (st == GG_OK && !ranks_distinct(rank, c->n)) st = fail(m, GG_ERR_INVALID_ARG, who + ": two candidates of one rank");
  if (st != GG_OK || nq == 0) return finish(c, st);
  const uint64_t* d_q = nullptr;
  const uint32_t* d_qlen = nullptr;
  st = sketch_files_first(c->ctx, paths, nq, cache_dir, &d_q, &d_qlen);
  if (st != GG_OK) return st;  // (reported on the context given)
  return finish(c, collection_classify(c, who, d_q, d_qlen, nq, rank, best, best_ani));
}

}  // extern "C"
