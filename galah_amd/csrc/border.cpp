// Adding genomes to a finished run (include/galahgpu.h, "the border"): the
// pairs (i < j) of rows 0 .. n-1 with j >= n_old, so that
//   gg_pairs(rows[0:n]) == gg_pairs(rows[0:n_old]) U gg_pairs_border(rows[0:n], n_old)
// with the sketch matrix left where it is (old rows first, new rows after
// them).  K2 evaluates only the new rows (pairs_core with n_old: the border
// forms of pairs_index.hip and pairs_gate.hip), or, by the context's pairs path
// (gg_set_pairs_path), the border form of the matrix product
// gives them.  Every entry point here acts on the context's first device.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.hpp"
#include "validate_core.hpp"

using namespace gg;

namespace {

gg_status check_border_args(const char* who, const void* sketches, const uint32_t* lens, uint32_t n, uint32_t n_old,
                            float min_ani, const void* out, const void* n_out, std::string& err) {
  if (!out || !n_out || (n && (!sketches || !lens))) {
    err = std::string(who) + ": null buffer";
    return GG_ERR_INVALID_ARG;
  }
  if (std::isnan(min_ani)) {
    err = "min_ani is NaN";
    return GG_ERR_INVALID_ARG;
  }
  if (n_old > n) {
    err = std::string(who) + ": n_old exceeds n";
    return GG_ERR_INVALID_ARG;
  }
  return GG_OK;
}

// The border of n rows resident on m's device, in (i, j) order: by the
// context's pairs path the border form of the matrix product, else K2.
gg_status border_to_host(gg_ctx* m, const char* who, const uint64_t* d_sk, const uint32_t* d_len, uint32_t n,
                         uint32_t n_old, float min_ani, std::vector<gg_pair>& res) {
  if (n < 2 || n_old >= n) return GG_OK;
  bool matrix = false;
  gg_status st = border_routed_to_host(m, who, d_sk, d_len, n, n_old, min_ani, res, &matrix, m->stream);
  if (st == GG_OK && !matrix)
    st = pairs_range_to_host(m, d_sk, d_len, n, 0, gg_pair_tiles(n), min_ani, res, m->stream, n_old);
  if (st == GG_OK) count_pairs_path(m, matrix);
  return st;
}

gg_status pairs_border_ctx(gg_ctx* m, const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t n_old,
                           float min_ani, std::vector<gg_pair>& res) {
  for (uint32_t i = 0; i < n; ++i)
    if (lens[i] > m->s) return fail(m, GG_ERR_INVALID_ARG, "sketch longer than sketch_size");
  if (n < 2 || n_old >= n) return GG_OK;
  const gg_status ds = use_device(m);
  if (ds != GG_OK) return ds;
  uint64_t* d_sk = nullptr;
  uint32_t* d_len = nullptr;
  GG_HIP(m, scratch_t(m, "bd_sk", (size_t)n * m->s, &d_sk));
  GG_HIP(m, scratch_t(m, "bd_len", (size_t)n, &d_len));
  GG_HIP(m, hipMemcpyAsync(d_sk, sketches, (size_t)n * m->s * sizeof(uint64_t), hipMemcpyHostToDevice, m->stream));
  GG_HIP(m, hipMemcpyAsync(d_len, lens, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
  return border_to_host(m, "gg_pairs_border", d_sk, d_len, n, n_old, min_ani, res);
}

gg_status update_files_ctx(gg_ctx* m, const uint64_t* old_sketches, const uint32_t* old_lens, uint32_t n_old,
                           const char* const* new_paths, uint32_t n_new, float min_ani, const char* cache_dir,
                           uint64_t* new_hashes, uint32_t* new_lens, std::vector<gg_pair>& res) {
  for (uint32_t i = 0; i < n_old; ++i)
    if (old_lens[i] > m->s) return fail(m, GG_ERR_INVALID_ARG, "sketch longer than sketch_size");
  if (n_new == 0) return GG_OK;
  // only the new files are read and sketched (cached ones come from the cache)
  gg_status st = gg_sketch_files(m, new_paths, n_new, cache_dir, new_hashes, new_lens, nullptr);
  if (st != GG_OK) return st;
  const uint32_t n = n_old + n_new;
  st = use_device(m);
  if (st != GG_OK) return st;
  uint64_t* d_sk = nullptr;
  uint32_t* d_len = nullptr;
  GG_HIP(m, scratch_t(m, "bd_sk", (size_t)n * m->s, &d_sk));
  GG_HIP(m, scratch_t(m, "bd_len", (size_t)n, &d_len));
  const size_t row = (size_t)m->s * sizeof(uint64_t);
  if (n_old) {
    GG_HIP(m, hipMemcpyAsync(d_sk, old_sketches, n_old * row, hipMemcpyHostToDevice, m->stream));
    GG_HIP(m, hipMemcpyAsync(d_len, old_lens, (size_t)n_old * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
  }
  GG_HIP(m, hipMemcpyAsync(d_sk + (size_t)n_old * m->s, new_hashes, n_new * row, hipMemcpyHostToDevice, m->stream));
  GG_HIP(m, hipMemcpyAsync(d_len + n_old, new_lens, (size_t)n_new * sizeof(uint32_t), hipMemcpyHostToDevice,
                           m->stream));
  return border_to_host(m, "gg_update_files", d_sk, d_len, n, n_old, min_ani, res);
}

}  // namespace

extern "C" {

gg_status gg_pairs_border_host(const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t n_old,
                               uint32_t sketch_size, int kmer_length, float min_ani, gg_pair** out, uint64_t* n_out) {
  std::string err;
  gg_status st = check_border_args("gg_pairs_border_host", sketches, lens, n, n_old, min_ani, out, n_out, err);
  if (st == GG_OK && (kmer_length < 1 || kmer_length > 32 || sketch_size < 1)) {
    err = "gg_pairs_border_host: kmer_length must be 1..32 and sketch_size at least 1";
    st = GG_ERR_INVALID_ARG;
  }
  for (uint32_t g = 0; st == GG_OK && g < n; ++g)
    if (lens[g] > sketch_size) {
      err = "gg_pairs_border_host: sketch longer than sketch_size";
      st = GG_ERR_INVALID_ARG;
    }
  if (st != GG_OK) {
    set_thread_error(err);
    return st;
  }
  *out = nullptr;
  *n_out = 0;
  // the kernels' rule: common >= cmin[total] (build_cmin inverts the f64 test once)
  const std::vector<uint32_t> cmin = build_cmin(sketch_size, kmer_length, min_ani);
  std::vector<gg_pair> res;
  for (uint32_t i = 0; i + 1 < n; ++i)
    for (uint32_t j = std::max(i + 1, n_old); j < n; ++j) {
      uint32_t common, total;
      validate::merge_counts(sketches + (size_t)i * sketch_size, lens[i], sketches + (size_t)j * sketch_size, lens[j],
                             &common, &total);
      if (total < cmin.size() && common >= cmin[total]) res.push_back(gg_pair{i, j, common, total});
    }
  *out = copy_out(res);
  if (!*out) {
    set_thread_error("out of host memory");
    return GG_ERR_OUT_OF_MEMORY;
  }
  *n_out = res.size();
  return GG_OK;
}

gg_status gg_pairs_border(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t n_old,
                          float min_ani, gg_pair** out, uint64_t* n_out) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  std::string err;
  gg_status st = check_border_args("gg_pairs_border", sketches, lens, n, n_old, min_ani, out, n_out, err);
  if (st != GG_OK) return fail(ctx, st, err);
  *out = nullptr;
  *n_out = 0;
  gg_ctx* m = primary(ctx);
  std::vector<gg_pair> res;
  st = pairs_border_ctx(m, sketches, lens, n, n_old, min_ani, res);
  if (st == GG_OK && !(*out = copy_out(res))) st = fail(m, GG_ERR_OUT_OF_MEMORY, "out of host memory");
  if (st == GG_OK) *n_out = res.size();
  return finish_call(ctx, m, st);
}

gg_status gg_pairs_border_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                                 uint32_t n_old, float min_ani, gg_pair* d_out, uint64_t out_cap, uint64_t* d_count,
                                 void* stream) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  if (n && (!d_sketches || !d_lens || !d_count || (out_cap && !d_out)))
    return fail(ctx, GG_ERR_INVALID_ARG, "gg_pairs_border_device: null buffer");
  if (std::isnan(min_ani)) return fail(ctx, GG_ERR_INVALID_ARG, "min_ani is NaN");
  if (n_old > n) return fail(ctx, GG_ERR_INVALID_ARG, "gg_pairs_border_device: n_old exceeds n");
  if (n < 2 || n_old == n) return GG_OK;
  gg_ctx* m = primary(ctx);
  bool matrix = false;
  gg_status st = use_device(m);
  if (st == GG_OK)
    st = border_routed_append(m, "gg_pairs_border_device", d_sketches, d_lens, n, n_old, min_ani, d_out, out_cap, d_count,
                              &matrix, (hipStream_t)stream);
  if (st == GG_OK && !matrix)
    st = pairs_core(m, d_sketches, d_lens, n, 0, gg_pair_tiles(n), min_ani, d_out, out_cap, d_count, (hipStream_t)stream,
                    n_old);
  if (st == GG_OK) count_pairs_path(m, matrix);
  return finish_call(ctx, m, st);
}

gg_status gg_update_files(gg_ctx* ctx, const uint64_t* old_sketches, const uint32_t* old_lens, uint32_t n_old,
                          const char* const* new_paths, uint32_t n_new, float min_ani, const char* cache_dir,
                          uint64_t* new_hashes, uint32_t* new_lens, gg_pair** pairs, float** ani, uint64_t* n_out) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  if (!pairs || !ani || !n_out || (n_old && (!old_sketches || !old_lens)) ||
      (n_new && (!new_paths || !new_hashes || !new_lens)))
    return fail(ctx, GG_ERR_INVALID_ARG, "gg_update_files: null argument");
  if (std::isnan(min_ani)) return fail(ctx, GG_ERR_INVALID_ARG, "min_ani is NaN");
  if ((uint64_t)n_old + n_new > 0xFFFFFFFFull) return fail(ctx, GG_ERR_INVALID_ARG, "gg_update_files: too many genomes");
  *pairs = nullptr;
  *ani = nullptr;
  *n_out = 0;
  gg_ctx* m = primary(ctx);
  std::vector<gg_pair> res;
  gg_status st =
      update_files_ctx(m, old_sketches, old_lens, n_old, new_paths, n_new, min_ani, cache_dir, new_hashes, new_lens, res);
  if (st == GG_OK) {
    *pairs = copy_out(res);
    *ani = (float*)malloc(std::max<size_t>(res.size(), 1) * sizeof(float));
    if (!*pairs || !*ani) st = fail(m, GG_ERR_OUT_OF_MEMORY, "out of host memory");
  }
  if (st == GG_OK) {
    for (size_t p = 0; p < res.size(); ++p) (*ani)[p] = gg_ani_f32(res[p].common, res[p].total, m->k);  // src/finch.rs:70
    *n_out = res.size();
  }
  return finish_call(ctx, m, st, [&] { free_out(pairs, ani); });
}

}  // extern "C"
