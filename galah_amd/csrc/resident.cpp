// Clustering from resident sketches: the rows of a sketch
// matrix in device memory to rep_of in device memory, the pair list never
// leaving it.  What gg_pairs + gg_ani_f32 + gg_cluster_pairs give, chained
// from their device forms:
//
//   1. K2 (pairs_core) over every tile into context scratch, sized as
//      pairs_range_to_host sizes it: max(2^20, 16 n) pairs clipped to
//      n (n - 1) / 2, the count word read back, one retry at the exact count;
//      or, by the context's pairs path (gg_set_pairs_path),
//      the pair form of the matrix product, sized the same way;
//   2. no sort: neither the clustering rules nor the partition depend on the
//      order of the pairs;
//   3. the f32 ANI of every pair (ani_f32_device), then cluster_device;
//   4. for the summary, the partition of preclusters_device (no local pairs):
//      the number of sets and the size of the first, which is the largest.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "context.hpp"
#include "matrix_core.hpp"

namespace gg {

namespace {

// GALAHGPU_PAIRS_MATRIX_RATIO, read per call: AUTO takes the product when the
// index's member reads exceed R chunk rounds (changes no result)
constexpr double kPairsMatrixRatio = 3675.0;  // (measured)
constexpr double kBorderMatrixRatio = 1000.0;  // a border call's (measured)
double pairs_matrix_ratio(double dflt = kPairsMatrixRatio) {
  const char* e = getenv("GALAHGPU_PAIRS_MATRIX_RATIO");
  if (!e || !*e) return dflt;
  char* end = nullptr;
  const double v = strtod(e, &end);
  return end == e || std::isnan(v) ? dflt : v;
}

// GALAHGPU_TEST_PAIRS_CAP, read per call: lowers gg_pairs_matrix's first capacity (tests of the retry)
uint64_t test_pairs_cap(uint64_t cap) {
  const char* e = getenv("GALAHGPU_TEST_PAIRS_CAP");
  if (!e || !*e) return cap;
  return std::min<uint64_t>(cap, std::max<uint64_t>(1, strtoull(e, nullptr, 10)));
}

void fill_matrix_summary(gg_pairs_matrix_summary* sum, const MatrixPrep& p) {
  sum->n_entries = p.n_entries;
  sum->n_columns = p.n_columns;
  sum->column_entries = p.column_entries;
  sum->chunk_rounds = matrix::pair_chunk_rounds(p.m, p.n_columns);
  sum->index_reads = matrix::pair_index_reads(p.n_columns, p.column_entries);
}

// The sized passes of a pair producer into scratch `key`: the first at `cap`,
// one retry at the exact count.  run(d_out, cap, d_count) enqueues it on st.
template <typename Run>
gg_status sized_pair_passes(gg_ctx* c, const std::string& who, const char* key, uint64_t all, uint64_t cap,
                            const Run& run, gg_pair** d_pairs, uint64_t* n_pairs, uint32_t* n_passes, hipStream_t st) {
  gg_pair* d_out = nullptr;
  uint64_t cnt = 0;
  uint32_t passes = 0;
  uint64_t *d_count, *h_count;
  GG_HIP(c, scratch_t(c, "rs_count", 1, &d_count));
  GG_HIP(c, host_scratch_t(c, "rs_count", 1, &h_count));
  for (;;) {
    if (passes == 2) return fail(c, GG_ERR_INTERNAL, who + ": pair output sizing failed");
    GG_HIP(c, scratch_t(c, key, (size_t)std::max<uint64_t>(cap, 1), &d_out));
    GG_HIP(c, hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
    const gg_status ps = run(d_out, cap, d_count);
    if (ps != GG_OK) return ps;
    ++passes;
    GG_HIP(c, hipMemcpyAsync(h_count, d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    GG_HIP(c, hipStreamSynchronize(st));
    cnt = *h_count;
    if (cnt > all) return fail(c, GG_ERR_INTERNAL, who + ": bad pair count");
    if (cnt <= cap) break;
    cap = cnt;
  }
  if (cnt >= (1ull << 31)) return fail(c, GG_ERR_INVALID_ARG, who + ": 2^31 pairs or more");
  *d_pairs = d_out;
  *n_pairs = cnt;
  *n_passes = passes;
  return GG_OK;
}

}  // namespace

gg_status pairs_rows_device(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                            float min_ani, gg_pair** d_pairs, uint64_t* n_pairs, uint32_t* n_passes, hipStream_t st,
                            gg_pairs_matrix_summary* msum) {
  *d_pairs = nullptr;
  *n_pairs = 0;
  *n_passes = 0;
  if (msum) *msum = gg_pairs_matrix_summary{};
  if (n < 2) return GG_OK;
  const uint64_t all = (uint64_t)n * (n - 1) / 2;
  const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(1 << 20, (uint64_t)n * 16), all);
  // the matrix: by request, or by AUTO's rule from the counts of the positions part
  bool matrix = false;
  MatrixPrep prep{};
  gg_pairs_matrix_summary ms{};
  if (c->pairs_path != GG_PAIRS_PATH_DEFAULT) {
    const bool fits = matrix::pair_limits_ok(n, c->s);
    if (c->pairs_path == GG_PAIRS_PATH_MATRIX && !fits)
      return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": 2^31 sketch slots or tile pairs, or more, on the matrix path");
    if (fits) {
      const gg_status r = matrix_prepare(c, who, d_sk, d_lens, n, nullptr, n, &prep, st);
      if (r != GG_OK) return r;
      fill_matrix_summary(&ms, prep);
      matrix = c->pairs_path == GG_PAIRS_PATH_MATRIX ||
               (prep.n_columns > 0 && (double)ms.index_reads > pairs_matrix_ratio() * (double)ms.chunk_rounds);
    }
  }
  gg_status r;
  if (matrix) {
    uint32_t *d_cmin, *d_sufmin;
    r = sized_pair_passes(
        c, who, "rs_pairs", all, cap,
        [&](gg_pair* d_out, uint64_t pcap, uint64_t* d_count) {
          const gg_status t = pairs_tables(c, min_ani, &d_cmin, &d_sufmin, st);
          return t != GG_OK ? t : pairs_matrix_launch(c, d_sk, prep, d_cmin, d_sufmin, d_out, pcap, d_count, st);
        },
        d_pairs, n_pairs, n_passes, st);
  } else {
    r = sized_pair_passes(
        c, who, "rs_pairs", all, cap,
        [&](gg_pair* d_out, uint64_t pcap, uint64_t* d_count) {
          return pairs_core(c, d_sk, d_lens, n, 0, gg_pair_tiles(n), min_ani, d_out, pcap, d_count, st);
        },
        d_pairs, n_pairs, n_passes, st);
  }
  if (r != GG_OK) return r;
  ++c->pairs_paths_taken[!matrix ? 0 : c->pairs_path == GG_PAIRS_PATH_MATRIX ? 1 : 2];
  if (msum) {
    *msum = ms;
    msum->n_pairs = *n_pairs;
    msum->path = matrix ? GG_PAIRS_PATH_MATRIX : GG_PAIRS_PATH_DEFAULT;
    msum->pair_passes = *n_passes;
  }
  return GG_OK;
}

// gg_pairs_matrix_device behind its argument checks
gg_status pairs_matrix_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n, const uint32_t* d_rows,
                              uint32_t m, float min_ani, gg_pair* d_out, uint64_t cap, uint64_t* d_count,
                              gg_pairs_matrix_summary* sum, hipStream_t st) {
  if (m < 2) {  // no pair: nothing is run
    if (sum) sum->path = GG_PAIRS_PATH_MATRIX;
    return GG_OK;
  }
  uint64_t* h_count = nullptr;
  if (sum) {  // the count before, read with the positions part's read-back
    GG_HIP(c, host_scratch_t(c, "pm_count", 2, &h_count));
    GG_HIP(c, hipMemcpyAsync(&h_count[0], d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  }
  MatrixPrep prep;
  gg_status r = matrix_prepare(c, "gg_pairs_matrix", d_sk, d_lens, n, d_rows, m, &prep, st);
  if (r != GG_OK) return r;
  uint32_t *d_cmin, *d_sufmin;
  r = pairs_tables(c, min_ani, &d_cmin, &d_sufmin, st);
  if (r != GG_OK) return r;
  r = pairs_matrix_launch(c, d_sk, prep, d_cmin, d_sufmin, d_out, cap, d_count, st);
  if (r != GG_OK) return r;
  if (sum) {
    GG_HIP(c, hipMemcpyAsync(&h_count[1], d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    GG_HIP(c, hipStreamSynchronize(st));
    fill_matrix_summary(sum, prep);
    sum->n_pairs = h_count[1] - h_count[0];
    sum->path = GG_PAIRS_PATH_MATRIX;
    sum->pair_passes = 1;
  }
  return GG_OK;
}

// gg_pairs_matrix behind its context lookup: host arrays in, the sorted list out
gg_status pairs_matrix_ctx(gg_ctx* c, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint32_t* rows,
                           uint32_t m, float min_ani, gg_pair** out, uint64_t* n_out, gg_pairs_matrix_summary* sum) {
  const char* who = "gg_pairs_matrix";
  if (!out || !n_out) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": null argument");
  *out = nullptr;
  *n_out = 0;
  if (std::isnan(min_ani)) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": min_ani is NaN");
  if (n && (!sketches || !lens)) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": null argument");
  if (!rows && m > n) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": more positions than rows");
  if (!matrix::pair_limits_ok(m, c->s) || !matrix::pair_limits_ok(n, c->s))
    return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": 2^31 sketch slots or tile pairs, or more");
  for (uint32_t g = 0; g < n; ++g)
    if (lens[g] > c->s) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": sketch longer than sketch_size");
  if (rows) {
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t a = 0; a < m; ++a) {
      if (rows[a] >= n) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": row index out of range");
      if (seen[rows[a]]) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": row index listed twice");
      seen[rows[a]] = 1;
    }
  }
  if (m < 2) {  // no pair: nothing is run
    if (sum) sum->path = GG_PAIRS_PATH_MATRIX;
    *out = (gg_pair*)malloc(sizeof(gg_pair));
    return *out ? GG_OK : fail(c, GG_ERR_OUT_OF_MEMORY, "out of host memory");
  }
  if (hipSetDevice(c->device) != hipSuccess) return fail(c, GG_ERR_HIP, "hipSetDevice failed");
  hipStream_t st = c->stream;
  uint64_t* d_sk = nullptr;
  uint32_t *d_len = nullptr, *d_rows = nullptr;
  GG_HIP(c, scratch_t(c, "mx_h_sk", (size_t)n * c->s, &d_sk));
  GG_HIP(c, scratch_t(c, "mx_h_len", (size_t)n, &d_len));
  GG_HIP(c, hipMemcpyAsync(d_sk, sketches, (size_t)n * c->s * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  GG_HIP(c, hipMemcpyAsync(d_len, lens, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (rows) {
    GG_HIP(c, scratch_t(c, "mx_h_rows", (size_t)m, &d_rows));
    GG_HIP(c, hipMemcpyAsync(d_rows, rows, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  MatrixPrep prep;
  gg_status r = matrix_prepare(c, who, d_sk, d_len, n, d_rows, m, &prep, st);
  if (r != GG_OK) return r;
  const uint64_t all = (uint64_t)m * (m - 1) / 2;
  const uint64_t cap = test_pairs_cap(std::min<uint64_t>(std::max<uint64_t>(1 << 20, (uint64_t)m * 16), all));
  gg_pair *d_pairs = nullptr, *d_sorted = nullptr;
  uint64_t cnt = 0;
  uint32_t passes = 0, *d_cmin, *d_sufmin;
  r = sized_pair_passes(
      c, who, "pm_pairs", all, cap,
      [&](gg_pair* d_out, uint64_t pcap, uint64_t* d_count) {
        const gg_status t = pairs_tables(c, min_ani, &d_cmin, &d_sufmin, st);
        return t != GG_OK ? t : pairs_matrix_launch(c, d_sk, prep, d_cmin, d_sufmin, d_out, pcap, d_count, st);
      },
      &d_pairs, &cnt, &passes, st);
  if (r != GG_OK) return r;
  r = sorted_pairs_device(c, d_pairs, cnt, n, &d_sorted, st);
  if (r != GG_OK) return r;
  *out = (gg_pair*)malloc(std::max<uint64_t>(cnt, 1) * sizeof(gg_pair));
  if (!*out) return fail(c, GG_ERR_OUT_OF_MEMORY, "out of host memory");
  if (cnt) GG_HIP(c, hipMemcpyAsync(*out, d_sorted, cnt * sizeof(gg_pair), hipMemcpyDeviceToHost, st));
  GG_HIP(c, hipStreamSynchronize(st));
  *n_out = cnt;
  if (sum) {
    fill_matrix_summary(sum, prep);
    sum->n_pairs = cnt;
    sum->path = GG_PAIRS_PATH_MATRIX;
    sum->pair_passes = passes;
  }
  return GG_OK;
}

// ---- the border form ------------------------------------------
namespace {

uint64_t border_all_pairs(uint32_t n, uint32_t n_old) {
  const uint64_t n_new = n - n_old;
  return n_new * n_old + n_new * (n_new - 1) / 2;
}

void fill_border_summary(gg_pairs_matrix_summary* sum, const MatrixPrep& p, uint32_t n_old) {
  sum->n_entries = p.n_entries;
  sum->n_columns = p.n_columns;
  sum->column_entries = p.column_entries;
  sum->chunk_rounds = matrix::border_chunk_rounds(p.m, n_old, p.n_columns);
  sum->index_reads = matrix::border_index_reads(p.n_columns, p.column_entries, p.new_entries);
}

// gg_pairs_border_matrix_device behind its argument checks (n >= 2, n_old < n)
gg_status pairs_border_matrix_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n, uint32_t n_old,
                                     float min_ani, gg_pair* d_out, uint64_t cap, uint64_t* d_count,
                                     gg_pairs_matrix_summary* sum, hipStream_t st) {
  const char* who = "gg_pairs_border_matrix";
  uint64_t* h_count = nullptr;
  if (sum) {  // the count before, read with the positions part's read-back
    GG_HIP(c, host_scratch_t(c, "pm_count", 2, &h_count));
    GG_HIP(c, hipMemcpyAsync(&h_count[0], d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  }
  MatrixPrep prep;
  gg_status r = matrix_prepare(c, who, d_sk, d_lens, n, nullptr, n, &prep, st, n_old);
  if (r != GG_OK) return r;
  uint32_t *d_cmin, *d_sufmin;
  r = pairs_tables(c, min_ani, &d_cmin, &d_sufmin, st);
  if (r != GG_OK) return r;
  r = pairs_border_matrix_launch(c, d_sk, prep, n - n_old, d_cmin, d_sufmin, d_out, cap, d_count, st);
  if (r != GG_OK) return r;
  if (sum) {
    GG_HIP(c, hipMemcpyAsync(&h_count[1], d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    GG_HIP(c, hipStreamSynchronize(st));
    fill_border_summary(sum, prep, n_old);
    sum->n_pairs = h_count[1] - h_count[0];
    sum->path = GG_PAIRS_PATH_MATRIX;
    sum->pair_passes = 1;
  }
  return GG_OK;
}

// The border of prepared positions into context scratch, sorted by (i, j):
// the first capacity min(all border pairs, max(2^20, 16 n)), one retry at the
// exact count.
gg_status border_matrix_sorted(gg_ctx* c, const char* who, const uint64_t* d_sk, const MatrixPrep& prep, uint32_t n,
                               uint32_t n_old, float min_ani, gg_pair** d_sorted, uint64_t* cnt, uint32_t* passes,
                               hipStream_t st) {
  const uint64_t all = border_all_pairs(n, n_old);
  const uint64_t cap = test_pairs_cap(std::min<uint64_t>(std::max<uint64_t>(1 << 20, (uint64_t)n * 16), all));
  gg_pair* d_pairs = nullptr;
  uint32_t *d_cmin, *d_sufmin;
  const gg_status r = sized_pair_passes(
      c, who, "pm_pairs", all, cap,
      [&](gg_pair* d_out, uint64_t pcap, uint64_t* d_count) {
        const gg_status t = pairs_tables(c, min_ani, &d_cmin, &d_sufmin, st);
        return t != GG_OK ? t
                          : pairs_border_matrix_launch(c, d_sk, prep, n - n_old, d_cmin, d_sufmin, d_out, pcap, d_count, st);
      },
      &d_pairs, cnt, passes, st);
  if (r != GG_OK) return r;
  return sorted_pairs_device(c, d_pairs, *cnt, n, d_sorted, st);
}

// gg_pairs_border_matrix behind its context lookup: host arrays in, the sorted list out
gg_status pairs_border_matrix_ctx(gg_ctx* c, const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t n_old,
                                  float min_ani, gg_pair** out, uint64_t* n_out, gg_pairs_matrix_summary* sum) {
  const char* who = "gg_pairs_border_matrix";
  if (!out || !n_out) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": null argument");
  *out = nullptr;
  *n_out = 0;
  if (std::isnan(min_ani)) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": min_ani is NaN");
  if (n_old > n) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": n_old exceeds n");
  if (!matrix::border_limits_ok(n, n_old, c->s))
    return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": 2^31 sketch slots or tile pairs, or more");
  if (n && (!sketches || !lens)) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": null argument");
  for (uint32_t g = 0; g < n; ++g)
    if (lens[g] > c->s) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": sketch longer than sketch_size");
  if (n < 2 || n_old == n) {  // no pair: nothing is run
    if (sum) sum->path = GG_PAIRS_PATH_MATRIX;
    *out = (gg_pair*)malloc(sizeof(gg_pair));
    return *out ? GG_OK : fail(c, GG_ERR_OUT_OF_MEMORY, "out of host memory");
  }
  if (hipSetDevice(c->device) != hipSuccess) return fail(c, GG_ERR_HIP, "hipSetDevice failed");
  hipStream_t st = c->stream;
  uint64_t* d_sk = nullptr;
  uint32_t* d_len = nullptr;
  GG_HIP(c, scratch_t(c, "mx_h_sk", (size_t)n * c->s, &d_sk));
  GG_HIP(c, scratch_t(c, "mx_h_len", (size_t)n, &d_len));
  GG_HIP(c, hipMemcpyAsync(d_sk, sketches, (size_t)n * c->s * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  GG_HIP(c, hipMemcpyAsync(d_len, lens, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  MatrixPrep prep;
  gg_status r = matrix_prepare(c, who, d_sk, d_len, n, nullptr, n, &prep, st, n_old);
  if (r != GG_OK) return r;
  gg_pair* d_sorted = nullptr;
  uint64_t cnt = 0;
  uint32_t passes = 0;
  r = border_matrix_sorted(c, who, d_sk, prep, n, n_old, min_ani, &d_sorted, &cnt, &passes, st);
  if (r != GG_OK) return r;
  *out = (gg_pair*)malloc(std::max<uint64_t>(cnt, 1) * sizeof(gg_pair));
  if (!*out) return fail(c, GG_ERR_OUT_OF_MEMORY, "out of host memory");
  if (cnt) GG_HIP(c, hipMemcpyAsync(*out, d_sorted, cnt * sizeof(gg_pair), hipMemcpyDeviceToHost, st));
  GG_HIP(c, hipStreamSynchronize(st));
  *n_out = cnt;
  if (sum) {
    fill_border_summary(sum, prep, n_old);
    sum->n_pairs = cnt;
    sum->path = GG_PAIRS_PATH_MATRIX;
    sum->pair_passes = passes;
  }
  return GG_OK;
}

// The route of a border call of n >= 2 rows, n_old < n, by the context's pairs
// path.  DEFAULT: nothing is run.  MATRIX: the border positions part, or
// GG_ERR_INVALID_ARG when the limits fail.  AUTO: the positions part when the
// limits hold, and the product iff there is a column and index_reads > R *
// chunk_rounds (R: GALAHGPU_PAIRS_MATRIX_RATIO, by default a border's own
// 1,000).
gg_status border_route(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                       uint32_t n_old, hipStream_t st, bool* matrix, MatrixPrep* prep) {
  *matrix = false;
  if (c->pairs_path == GG_PAIRS_PATH_DEFAULT) return GG_OK;
  const bool fits = matrix::border_limits_ok(n, n_old, c->s);
  if (c->pairs_path == GG_PAIRS_PATH_MATRIX && !fits)
    return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": 2^31 sketch slots or tile pairs, or more, on the matrix path");
  if (!fits) return GG_OK;
  const gg_status r = matrix_prepare(c, who, d_sk, d_lens, n, nullptr, n, prep, st, n_old);
  if (r != GG_OK) return r;
  gg_pairs_matrix_summary ms{};
  fill_border_summary(&ms, *prep, n_old);
  *matrix = c->pairs_path == GG_PAIRS_PATH_MATRIX ||
            (prep->n_columns > 0 && (double)ms.index_reads > pairs_matrix_ratio(kBorderMatrixRatio) * (double)ms.chunk_rounds);
  return GG_OK;
}

}  // namespace

void count_pairs_path(gg_ctx* c, bool matrix) {
  ++c->pairs_paths_taken[!matrix ? 0 : c->pairs_path == GG_PAIRS_PATH_MATRIX ? 1 : 2];
}

gg_status border_routed_to_host(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                                uint32_t n_old, float min_ani, std::vector<gg_pair>& res, bool* ran, hipStream_t st) {
  MatrixPrep prep{};
  gg_status r = border_route(c, who, d_sk, d_lens, n, n_old, st, ran, &prep);
  if (r != GG_OK || !*ran) return r;
  gg_pair* d_sorted = nullptr;
  uint64_t cnt = 0;
  uint32_t passes = 0;
  r = border_matrix_sorted(c, who, d_sk, prep, n, n_old, min_ani, &d_sorted, &cnt, &passes, st);
  if (r != GG_OK) return r;
  const size_t at = res.size();
  res.resize(at + cnt);
  if (cnt) GG_HIP(c, hipMemcpyAsync(res.data() + at, d_sorted, cnt * sizeof(gg_pair), hipMemcpyDeviceToHost, st));
  GG_HIP(c, hipStreamSynchronize(st));
  return GG_OK;
}

gg_status border_routed_append(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                               uint32_t n_old, float min_ani, gg_pair* d_out, uint64_t cap, uint64_t* d_count, bool* ran,
                               hipStream_t st) {
  MatrixPrep prep{};
  gg_status r = border_route(c, who, d_sk, d_lens, n, n_old, st, ran, &prep);
  if (r != GG_OK || !*ran) return r;
  uint32_t *d_cmin, *d_sufmin;
  r = pairs_tables(c, min_ani, &d_cmin, &d_sufmin, st);
  if (r != GG_OK) return r;
  return pairs_border_matrix_launch(c, d_sk, prep, n - n_old, d_cmin, d_sufmin, d_out, cap, d_count, st);
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

gg_status gg_pairs_matrix_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                                 const uint32_t* d_rows, uint32_t m, float min_ani, gg_pair* d_out, uint64_t out_cap,
                                 uint64_t* d_count, gg_pairs_matrix_summary* summary, void* stream) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  gg_status st = GG_OK;
  if (summary) *summary = gg_pairs_matrix_summary{};
  if (std::isnan(min_ani))
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_pairs_matrix_device: min_ani is NaN");
  else if (!matrix::pair_limits_ok(m, pm->s))  // (before any buffer is looked at)
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_pairs_matrix_device: 2^31 sketch slots or tile pairs, or more");
  else if (m >= 2 && (!d_count || (out_cap && !d_out) || (n && (!d_sketches || !d_lens))))
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_pairs_matrix_device: null buffer");
  else if (hipSetDevice(pm->device) != hipSuccess)
    st = fail(pm, GG_ERR_HIP, "hipSetDevice failed");
  else
    st = pairs_matrix_device(pm, d_sketches, d_lens, n, d_rows, m, min_ani, d_out, out_cap, d_count, summary,
                             (hipStream_t)stream);
  if (st != GG_OK) {
    if (summary) *summary = gg_pairs_matrix_summary{};
    if (pm != ctx) ctx->err = pm->err;
  }
  return st;
}

gg_status gg_pairs_matrix(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint32_t* rows,
                          uint32_t m, float min_ani, gg_pair** out, uint64_t* n_out, gg_pairs_matrix_summary* summary) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  if (summary) *summary = gg_pairs_matrix_summary{};
  const gg_status st = pairs_matrix_ctx(pm, sketches, lens, n, rows, m, min_ani, out, n_out, summary);
  if (st != GG_OK) {
    if (out) {
      free(*out);
      *out = nullptr;
    }
    if (n_out) *n_out = 0;
    if (summary) *summary = gg_pairs_matrix_summary{};
    if (pm != ctx) ctx->err = pm->err;
  }
  return st;
}

gg_status gg_pairs_border_matrix_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                                        uint32_t n_old, float min_ani, gg_pair* d_out, uint64_t out_cap,
                                        uint64_t* d_count, gg_pairs_matrix_summary* summary, void* stream) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  gg_status st = GG_OK;
  if (summary) *summary = gg_pairs_matrix_summary{};
  const bool work = n >= 2 && n_old < n;
  if (std::isnan(min_ani))
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_pairs_border_matrix_device: min_ani is NaN");
  else if (n_old > n)  // (the limits: before any buffer is looked at)
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_pairs_border_matrix_device: n_old exceeds n");
  else if (!matrix::border_limits_ok(n, n_old, pm->s))
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_pairs_border_matrix_device: 2^31 sketch slots or tile pairs, or more");
  else if (work && (!d_sketches || !d_lens || !d_count || (out_cap && !d_out)))
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_pairs_border_matrix_device: null buffer");
  else if (!work) {  // no pair: nothing is run, the count is left as it is
    if (summary) summary->path = GG_PAIRS_PATH_MATRIX;
  } else if (hipSetDevice(pm->device) != hipSuccess)
    st = fail(pm, GG_ERR_HIP, "hipSetDevice failed");
  else
    st = pairs_border_matrix_device(pm, d_sketches, d_lens, n, n_old, min_ani, d_out, out_cap, d_count, summary,
                                    (hipStream_t)stream);
  if (st != GG_OK) {
    if (summary) *summary = gg_pairs_matrix_summary{};
    if (pm != ctx) ctx->err = pm->err;
  }
  return st;
}

gg_status gg_pairs_border_matrix(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t n_old,
                                 float min_ani, gg_pair** out, uint64_t* n_out, gg_pairs_matrix_summary* summary) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  if (summary) *summary = gg_pairs_matrix_summary{};
  const gg_status st = pairs_border_matrix_ctx(pm, sketches, lens, n, n_old, min_ani, out, n_out, summary);
  if (st != GG_OK) {
    if (out) {
      free(*out);
      *out = nullptr;
    }
    if (n_out) *n_out = 0;
    if (summary) *summary = gg_pairs_matrix_summary{};
    if (pm != ctx) ctx->err = pm->err;
  }
  return st;
}

gg_status gg_set_pairs_path(gg_ctx* ctx, int path) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  if (path != GG_PAIRS_PATH_DEFAULT && path != GG_PAIRS_PATH_MATRIX && path != GG_PAIRS_PATH_AUTO)
    return fail(ctx, GG_ERR_INVALID_ARG, "gg_set_pairs_path: unknown path");
  primary(ctx)->pairs_path = path;
  return GG_OK;
}

int gg_pairs_path(const gg_ctx* ctx) { return ctx ? primary(const_cast<gg_ctx*>(ctx))->pairs_path : -1; }

gg_status gg_pairs_paths_taken(const gg_ctx* ctx, uint64_t* counts) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  if (!counts) return fail(const_cast<gg_ctx*>(ctx), GG_ERR_INVALID_ARG, "gg_pairs_paths_taken: null argument");
  const gg_ctx* pm = primary(const_cast<gg_ctx*>(ctx));
  for (int i = 0; i < 3; ++i) counts[i] = pm->pairs_paths_taken[i];
  return GG_OK;
}

}  // extern "C"
