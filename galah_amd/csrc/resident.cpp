// Clustering from resident sketches: the rows of a sketch
// matrix in device memory to rep_of in device memory, the pair list never
// leaving it.  What gg_pairs + gg_ani_f32 + gg_cluster_pairs give, chained
// from their device forms:
//
//   1. K2 (pairs_core) over every tile into context scratch, in the sized
//      passes every caller shares (sized_pair_passes): max(2^20, 16 n) pairs
//      clipped to n (n - 1) / 2, the count word read back, one retry at the
//      exact count;
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
double pairs_matrix_ratio(double dflt) {
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

// What differs between the two forms of the product that give pairs: the pair
// form over m positions, and the border form (4.13) over all
// m == n rows of which the first n_old are old.
struct PairsForm {
  uint32_t m;
  bool border;
  uint32_t n_old;
  bool work() const { return m >= 2 && !(border && n_old == m); }  // there is a pair to evaluate
  bool limits_ok(uint32_t s) const { return border ? matrix::border_limits_ok(m, n_old, s) : matrix::pair_limits_ok(m, s); }
  uint64_t all() const {
    const uint64_t n_new = border ? m - n_old : m, old = m - n_new;
    return n_new * old + n_new * (n_new - 1) / 2;
  }
  double ratio() const { return border ? kBorderMatrixRatio : kPairsMatrixRatio; }
  gg_status prepare(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                    const uint32_t* d_rows, MatrixPrep* prep, hipStream_t st) const {
    return matrix_prepare(c, who, d_sk, d_lens, n, d_rows, m, border ? MatrixForm{MatrixForm::kBorder, n_old} : MatrixForm{},
                          prep, st);
  }
  // the tables of min_ani and the launch: asynchronous
  gg_status run(gg_ctx* c, const uint64_t* d_sk, const MatrixPrep& p, float min_ani, gg_pair* d_out, uint64_t cap,
                uint64_t* d_count, hipStream_t st) const {
    uint32_t *d_cmin, *d_sufmin;
    const gg_status t = pairs_tables(c, min_ani, &d_cmin, &d_sufmin, st);
    if (t != GG_OK) return t;
    return border ? pairs_border_matrix_launch(c, d_sk, p, m - n_old, d_cmin, d_sufmin, d_out, cap, d_count, st)
                  : pairs_matrix_launch(c, d_sk, p, d_cmin, d_sufmin, d_out, cap, d_count, st);
  }
  void fill(gg_pairs_matrix_summary* sum, const MatrixPrep& p) const {
    sum->n_entries = p.n_entries;
    sum->n_columns = p.n_columns;
    sum->column_entries = p.column_entries;
    sum->chunk_rounds = border ? matrix::border_chunk_rounds(p.m, n_old, p.n_columns) : matrix::pair_chunk_rounds(p.m, p.n_columns);
    sum->index_reads = border ? matrix::border_index_reads(p.n_columns, p.column_entries, p.new_entries)
                              : matrix::pair_index_reads(p.n_columns, p.column_entries);
  }
  void fill(gg_pairs_matrix_summary* sum, const MatrixPrep& p, uint64_t n_pairs, uint32_t passes) const {
    fill(sum, p);
    sum->n_pairs = n_pairs;
    sum->path = GG_PAIRS_PATH_MATRIX;
    sum->pair_passes = passes;
  }
};

// The route of a call over resident rows by the context's pairs path.
// DEFAULT: nothing is run.  MATRIX: the positions part, or GG_ERR_INVALID_ARG
// when the limits fail.  AUTO: the positions part when the limits hold, and
// the product iff there is a column and index_reads > R * chunk_rounds (R:
// GALAHGPU_PAIRS_MATRIX_RATIO, by default the form's own: 3,675, or a
// border's 1,000).  *ms: the counts whenever the positions part ran.
gg_status matrix_route(gg_ctx* c, const char* who, const PairsForm& form, const uint64_t* d_sk, const uint32_t* d_lens,
                       uint32_t n, hipStream_t st, bool* matrix, MatrixPrep* prep, gg_pairs_matrix_summary* ms) {
  *matrix = false;
  if (c->pairs_path == GG_PAIRS_PATH_DEFAULT) return GG_OK;
  const bool fits = form.limits_ok(c->s);
  if (c->pairs_path == GG_PAIRS_PATH_MATRIX && !fits)
    return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": 2^31 sketch slots or tile pairs, or more, on the matrix path");
  if (!fits) return GG_OK;
  const gg_status r = form.prepare(c, who, d_sk, d_lens, n, nullptr, prep, st);
  if (r != GG_OK) return r;
  form.fill(ms, *prep);
  *matrix = c->pairs_path == GG_PAIRS_PATH_MATRIX ||
            (prep->n_columns > 0 && (double)ms->index_reads > pairs_matrix_ratio(form.ratio()) * (double)ms->chunk_rounds);
  return GG_OK;
}

// The middle of the host frame: the pairs of prepared positions into context
// scratch, sorted by (i, j) -- the first capacity min(all pairs of the form,
// max(2^20, 16 m)), one retry at the exact count.
gg_status pairs_form_sorted(gg_ctx* c, const char* who, const PairsForm& form, const uint64_t* d_sk, const MatrixPrep& prep,
                            uint32_t n, float min_ani, gg_pair** d_sorted, uint64_t* cnt, uint32_t* passes,
                            hipStream_t st) {
  const uint64_t all = form.all();
  const uint64_t cap = test_pairs_cap(std::min<uint64_t>(std::max<uint64_t>(1 << 20, (uint64_t)form.m * 16), all));
  gg_pair* d_pairs = nullptr;
  const gg_status r = sized_pair_passes(
      c, who, "pm_pairs", all, cap,
      [&](gg_pair* d_out, uint64_t pcap, uint64_t* d_count) { return form.run(c, d_sk, prep, min_ani, d_out, pcap, d_count, st); },
      &d_pairs, cnt, passes, st);
  if (r != GG_OK) return r;
  if (*cnt >= (1ull << 31)) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": 2^31 pairs or more");
  return sorted_pairs_device(c, d_pairs, *cnt, n, d_sorted, st);
}

// The device frame (gg_pairs_matrix_device, gg_pairs_border_matrix_device
// behind their argument checks): the count before, the positions part, the
// tables, the launch, the count after, the summary.
gg_status pairs_form_device(gg_ctx* c, const char* who, const PairsForm& form, const uint64_t* d_sk, const uint32_t* d_lens,
                            uint32_t n, const uint32_t* d_rows, float min_ani, gg_pair* d_out, uint64_t cap,
                            uint64_t* d_count, gg_pairs_matrix_summary* sum, hipStream_t st) {
  if (!form.work()) {  // no pair: nothing is run, the count is left as it is
    if (sum) sum->path = GG_PAIRS_PATH_MATRIX;
    return GG_OK;
  }
  uint64_t* h_count = nullptr;
  if (sum) {  // the count before, read with the positions part's read-back
    GG_HIP(c, host_scratch_t(c, "pm_count", 2, &h_count));
    GG_HIP(c, hipMemcpyAsync(&h_count[0], d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  }
  MatrixPrep prep;
  gg_status r = form.prepare(c, who, d_sk, d_lens, n, d_rows, &prep, st);
  if (r != GG_OK) return r;
  r = form.run(c, d_sk, prep, min_ani, d_out, cap, d_count, st);
  if (r != GG_OK) return r;
  if (sum) {
    GG_HIP(c, hipMemcpyAsync(&h_count[1], d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    GG_HIP(c, hipStreamSynchronize(st));
    form.fill(sum, prep, h_count[1] - h_count[0], 1);
  }
  return GG_OK;
}

// The host frame (gg_pairs_matrix, gg_pairs_border_matrix behind their
// argument checks): host arrays in, the sorted list out.
gg_status pairs_form_host(gg_ctx* c, const char* who, const PairsForm& form, const uint64_t* sketches, const uint32_t* lens,
                          uint32_t n, const uint32_t* rows, float min_ani, gg_pair** out, uint64_t* n_out,
                          gg_pairs_matrix_summary* sum) {
  if (!form.work()) {  // no pair: nothing is run
    if (sum) sum->path = GG_PAIRS_PATH_MATRIX;
    *out = (gg_pair*)malloc(sizeof(gg_pair));
    return *out ? GG_OK : fail(c, GG_ERR_OUT_OF_MEMORY, "out of host memory");
  }
  gg_status r = use_device(c);
  if (r != GG_OK) return r;
  hipStream_t st = c->stream;
  uint64_t* d_sk = nullptr;
  uint32_t *d_len = nullptr, *d_rows = nullptr;
  r = upload_sketch_rows(c, sketches, lens, n, rows, form.m, &d_sk, &d_len, &d_rows, st);
  if (r != GG_OK) return r;
  MatrixPrep prep;
  r = form.prepare(c, who, d_sk, d_len, n, d_rows, &prep, st);
  if (r != GG_OK) return r;
  gg_pair* d_sorted = nullptr;
  uint64_t cnt = 0;
  uint32_t passes = 0;
  r = pairs_form_sorted(c, who, form, d_sk, prep, n, min_ani, &d_sorted, &cnt, &passes, st);
  if (r != GG_OK) return r;
  r = copy_out(c, d_sorted, cnt, out, st);
  if (r != GG_OK) return r;
  GG_HIP(c, hipStreamSynchronize(st));
  *n_out = cnt;
  if (sum) form.fill(sum, prep, cnt, passes);
  return GG_OK;
}

// gg_pairs_matrix behind its context lookup
gg_status pairs_matrix_ctx(gg_ctx* c, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint32_t* rows,
                           uint32_t m, float min_ani, gg_pair** out, uint64_t* n_out, gg_pairs_matrix_summary* sum) {
  const std::string who = "gg_pairs_matrix";
  if (!out || !n_out) return fail(c, GG_ERR_INVALID_ARG, who + ": null argument");
  *out = nullptr;
  *n_out = 0;
  if (std::isnan(min_ani)) return fail(c, GG_ERR_INVALID_ARG, who + ": min_ani is NaN");
  std::string err;
  gg_status st = check_sketch_arrays(who, sketches, lens, n, rows, false, m, err);
  if (st != GG_OK) return fail(c, st, err);
  if (!matrix::pair_limits_ok(m, c->s) || !matrix::pair_limits_ok(n, c->s))
    return fail(c, GG_ERR_INVALID_ARG, who + ": 2^31 sketch slots or tile pairs, or more");
  st = check_sketch_rows(who, lens, n, c->s, rows, m, true, err);
  if (st != GG_OK) return fail(c, st, err);
  return pairs_form_host(c, who.c_str(), PairsForm{m, false, 0}, sketches, lens, n, rows, min_ani, out, n_out, sum);
}

// gg_pairs_border_matrix behind its context lookup
gg_status pairs_border_matrix_ctx(gg_ctx* c, const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t n_old,
                                  float min_ani, gg_pair** out, uint64_t* n_out, gg_pairs_matrix_summary* sum) {
  const std::string who = "gg_pairs_border_matrix";
  if (!out || !n_out) return fail(c, GG_ERR_INVALID_ARG, who + ": null argument");
  *out = nullptr;
  *n_out = 0;
  if (std::isnan(min_ani)) return fail(c, GG_ERR_INVALID_ARG, who + ": min_ani is NaN");
  if (n_old > n) return fail(c, GG_ERR_INVALID_ARG, who + ": n_old exceeds n");
  if (!matrix::border_limits_ok(n, n_old, c->s))
    return fail(c, GG_ERR_INVALID_ARG, who + ": 2^31 sketch slots or tile pairs, or more");
  std::string err;
  gg_status st = check_sketch_arrays(who, sketches, lens, n, nullptr, false, n, err);
  if (st == GG_OK) st = check_sketch_rows(who, lens, n, c->s, nullptr, n, false, err);
  if (st != GG_OK) return fail(c, st, err);
  return pairs_form_host(c, who.c_str(), PairsForm{n, true, n_old}, sketches, lens, n, nullptr, min_ani, out, n_out, sum);
}

}  // namespace

void count_pairs_path(gg_ctx* c, bool matrix) {
  ++c->pairs_paths_taken[!matrix ? 0 : c->pairs_path == GG_PAIRS_PATH_MATRIX ? 1 : 2];
}

gg_status pairs_rows_device(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                            float min_ani, gg_pair** d_pairs, uint64_t* n_pairs, uint32_t* n_passes, hipStream_t st,
                            gg_pairs_matrix_summary* msum) {
  *d_pairs = nullptr;
  *n_pairs = 0;
  *n_passes = 0;
  if (msum) *msum = gg_pairs_matrix_summary{};
  if (n < 2) return GG_OK;
  const PairsForm form{n, false, 0};
  const uint64_t all = form.all();
  const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(1 << 20, (uint64_t)n * 16), all);
  // the matrix: by request, or by AUTO's rule from the counts of the positions part
  bool matrix = false;
  MatrixPrep prep{};
  gg_pairs_matrix_summary ms{};
  gg_status r = matrix_route(c, who, form, d_sk, d_lens, n, st, &matrix, &prep, &ms);
  if (r != GG_OK) return r;
  r = sized_pair_passes(
      c, who, "rs_pairs", all, cap,
      [&](gg_pair* d_out, uint64_t pcap, uint64_t* d_count) {
        return matrix ? form.run(c, d_sk, prep, min_ani, d_out, pcap, d_count, st)
                      : pairs_core(c, d_sk, d_lens, n, 0, gg_pair_tiles(n), min_ani, d_out, pcap, d_count, st);
      },
      d_pairs, n_pairs, n_passes, st);
  if (r != GG_OK) return r;
  if (*n_pairs >= (1ull << 31)) return fail(c, GG_ERR_INVALID_ARG, std::string(who) + ": 2^31 pairs or more");
  count_pairs_path(c, matrix);
  if (msum) {
    *msum = ms;
    msum->n_pairs = *n_pairs;
    msum->path = matrix ? GG_PAIRS_PATH_MATRIX : GG_PAIRS_PATH_DEFAULT;
    msum->pair_passes = *n_passes;
  }
  return GG_OK;
}

gg_status border_routed_to_host(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                                uint32_t n_old, float min_ani, std::vector<gg_pair>& res, bool* ran, hipStream_t st) {
  const PairsForm form{n, true, n_old};
  MatrixPrep prep{};
  gg_pairs_matrix_summary ms{};
  gg_status r = matrix_route(c, who, form, d_sk, d_lens, n, st, ran, &prep, &ms);
  if (r != GG_OK || !*ran) return r;
  gg_pair* d_sorted = nullptr;
  uint64_t cnt = 0;
  uint32_t passes = 0;
  r = pairs_form_sorted(c, who, form, d_sk, prep, n, min_ani, &d_sorted, &cnt, &passes, st);
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
  const PairsForm form{n, true, n_old};
  MatrixPrep prep{};
  gg_pairs_matrix_summary ms{};
  const gg_status r = matrix_route(c, who, form, d_sk, d_lens, n, st, ran, &prep, &ms);
  if (r != GG_OK || !*ran) return r;
  return form.run(c, d_sk, prep, min_ani, d_out, cap, d_count, st);
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
  else if ((st = use_device(m)) == GG_OK)
    st = cluster_rows_device(m, d_sketches, d_lens, n, min_ani, cluster_ani, d_rep_of, summary, d_pairs, d_ani,
                             (hipStream_t)stream);
  return finish_call(ctx, m, st, [&] {
    if (summary) *summary = gg_cluster_summary{};
    if (d_pairs) *d_pairs = nullptr;
    if (d_ani) *d_ani = nullptr;
  });
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
  else if ((st = use_device(pm)) == GG_OK)
    st = pairs_form_device(pm, "gg_pairs_matrix", PairsForm{m, false, 0}, d_sketches, d_lens, n, d_rows, min_ani, d_out,
                           out_cap, d_count, summary, (hipStream_t)stream);
  return finish_call(ctx, pm, st, [&] { if (summary) *summary = gg_pairs_matrix_summary{}; });
}

// the failure tail of the host forms: the list is freed, nothing is reported
static gg_status finish_pair_list(gg_ctx* ctx, gg_ctx* pm, gg_status st, gg_pair** out, uint64_t* n_out,
                                  gg_pairs_matrix_summary* summary) {
  return finish_call(ctx, pm, st, [&] {
    free_out(out);
    if (n_out) *n_out = 0;
    if (summary) *summary = gg_pairs_matrix_summary{};
  });
}

gg_status gg_pairs_matrix(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint32_t* rows,
                          uint32_t m, float min_ani, gg_pair** out, uint64_t* n_out, gg_pairs_matrix_summary* summary) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  if (summary) *summary = gg_pairs_matrix_summary{};
  return finish_pair_list(ctx, pm, pairs_matrix_ctx(pm, sketches, lens, n, rows, m, min_ani, out, n_out, summary), out,
                          n_out, summary);
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
  else if (!work || (st = use_device(pm)) == GG_OK)  // (no work: nothing is run, the count is left as it is)
    st = pairs_form_device(pm, "gg_pairs_border_matrix", PairsForm{n, true, n_old}, d_sketches, d_lens, n, nullptr, min_ani,
                           d_out, out_cap, d_count, summary, (hipStream_t)stream);
  return finish_call(ctx, pm, st, [&] { if (summary) *summary = gg_pairs_matrix_summary{}; });
}

gg_status gg_pairs_border_matrix(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t n_old,
                                 float min_ani, gg_pair** out, uint64_t* n_out, gg_pairs_matrix_summary* summary) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  if (summary) *summary = gg_pairs_matrix_summary{};
  return finish_pair_list(ctx, pm, pairs_border_matrix_ctx(pm, sketches, lens, n, n_old, min_ani, out, n_out, summary), out,
                          n_out, summary);
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
