// The context behind the C ABI (gg_ctx) and the single-device building
// blocks the entry points are made of (api.cpp), shared with the
// multi-device orchestration (multi.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gg_internal.hpp"

// One host thread per member of a multi-device context beyond the first
// (member 0 runs on the calling thread), kept for the context's life: a
// distances() call hands work to the members several times (sketch,
// replicate, pairs), and starting 7 threads each time cost ~0.5 ms per call
// at 8 devices, where a C3 step is ~7 ms.
class MemberPool {
 public:
  explicit MemberPool(size_t n) {
    for (size_t i = 1; i < n; ++i) th_.emplace_back([this, i] { loop(i); });
  }
  ~MemberPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  size_t size() const { return th_.size() + 1; }
  // f(i) for every member i, member 0 on the calling thread; returns when all are done
  void run(const std::function<void(size_t)>& f) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      job_ = &f;
      pending_ = th_.size();
      ++gen_;
    }
    cv_.notify_all();
    f(0);
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [&] { return pending_ == 0; });
    job_ = nullptr;
  }

 private:
  void loop(size_t i) {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [&] { return quit_ || gen_ != seen; });
      if (quit_) return;
      seen = gen_;
      const std::function<void(size_t)>* f = job_;
      lk.unlock();
      (*f)(i);
      lk.lock();
      if (--pending_ == 0) done_.notify_all();
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_, done_;
  const std::function<void(size_t)>* job_ = nullptr;
  size_t pending_ = 0;
  uint64_t gen_ = 0;
  bool quit_ = false;
};

// A context is either ONE device (devs empty: the fields below drive it) or
// a multi-device context whose members devs[i] are single-device contexts
// (one per entry of the device list; the same ordinal may appear more than
// once, each entry then being its own shard with its own stream).
struct gg_ctx {
  int k = 21;
  uint32_t s = 1000;
  uint64_t seed = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // grow-only device scratch, keyed by purpose
  std::map<std::string, std::pair<void*, size_t>> scratch;
  // K1's candidate sets ("table" scratch) known empty, with their flags
  // clear, over [0, clean_table_bytes) of clean_table: the finalize kernel
  // leaves every set it reads empty, so only a new or grown buffer is cleared
  const void* clean_table = nullptr;
  size_t clean_table_bytes = 0;
  // grow-only pinned host staging buffer (streamed ingest)
  void* pinned = nullptr;
  size_t pinned_bytes = 0;
  // device-inflate staging slots (ingest_gz.cpp GzStager): batch N is inflated
  // from one while N + 1 is staged into the other by a helper thread, which
  // touches only its slot (grow-only pinned and device buffers, its stream)
  struct GzSlot {
    uint8_t* host = nullptr;      // (mapped: host_dev is its device address)
    uint8_t* host_dev = nullptr;
    size_t host_cap = 0;
    uint8_t* dev = nullptr;
    size_t dev_cap = 0;
    hipStream_t st = nullptr;
  };
  GzSlot gz_slot[2];
  // grow-only pinned host buffers keyed by purpose (small read-backs: one
  // DMA instead of a staged copy of pageable memory, ~35 us each)
  std::map<std::string, std::pair<void*, size_t>> host_scratch;
  // cached cmin table
  float cmin_key = -1.0f;
  std::vector<uint32_t> cmin_host;
  // per-kernel timing (gg_timing_enable)
  struct Timed {
    int kernel;
    hipEvent_t a, b;
    uint64_t work;
  };
  std::vector<gg::PairSeg> seg_host;
  std::vector<uint64_t> sstart_host;
  int pairs_kernel = 0;  // GALAHGPU_PAIRS_KERNEL: 0 auto, 1 table, 2 merge, 3 gate, 4 index
  std::vector<uint32_t> sufmin_host;
  bool timing = false;
  std::vector<Timed> timed;
  std::vector<hipEvent_t> spare_events;
  // multi-device context: the members (owned) and their host threads
  std::vector<gg_ctx*> devs;
  // helper contexts of this device (owned; created on first use, kept for
  // the context's life): the device-inflate ingest runs several batches at
  // once, each processing lane on its own stream with its own scratch
  // (ingest_gz.cpp); lanes[0] is unused (lane 0 is this context)
  std::vector<gg_ctx*> lanes;
  std::unique_ptr<MemberPool> pool;
  // a member's copy streams, one per peer it gathers rows from (created on
  // first use), so the copies from different peers run at once
  std::vector<hipStream_t> peer_streams;
  uint64_t pair_paths[GG_PATH_COUNT] = {};  // gg_pair_paths
  // what pairs_rows_device runs (gg_set_pairs_path), and its calls that ran
  // the default K2, the matrix by request, the matrix by AUTO's choice
  int pairs_path = GG_PAIRS_PATH_DEFAULT;
  uint64_t pairs_paths_taken[3] = {};
  // of the index calls abandoned for the gate kernel (GG_PATH_INDEX_ABANDONED),
  // those whose member reads outweighed the gate kernel's merges (gg_info_line)
  uint64_t index_costly = 0;
  // gg_fallbacks (the two index entries are read from pair_paths)
  uint64_t fallbacks[GG_FALLBACK_COUNT] = {};
  uint64_t inflate_dev_batches = 0;  // gzip batches inflated on the device (gg_info_line)
  // device-inflate plans beyond a batch's first: member boundaries found by
  // the decode (files of several gzip members), full-size token areas after
  // a tight one filled (gg_info_line)
  uint64_t gz_member_plans = 0, gz_full_plans = 0;
  // the largest inflate scratch of a batch on this lane (tokens, sub-span
  // areas, val, text), bytes: the per-lane footprint the info line reports
  uint64_t gz_scratch_bytes = 0;
  // gg_cluster_pairs(_device) calls on this device, and the launches of the
  // representative-round kernel in the last one (gg_info_line)
  uint64_t cluster_calls = 0, cluster_rounds = 0;
  // gg_preclusters(_device) calls on this device, and the pointer-jumping
  // launches of the last one (gg_info_line)
  uint64_t precluster_calls = 0, precluster_jumps = 0;
  // scratch / host-scratch buffers regrown (and the wall ms it took), gg_info_line
  uint64_t scratch_regrows = 0;
  double scratch_regrow_ms = 0;
  // a device scratch buffer that grows is allocated for this many times the
  // size asked (an ingest batch smaller than the largest the call may stage:
  // its buffers sized for that one at once, so that no later batch regrows
  // them -- a regrowth's hipFree waits for the whole device)
  double scratch_hint = 1.0;
  // multi-device context: [a * M + b] = 1 when member a reaches member b's
  // memory directly (same device, or peer access enabled), gg_peer_links
  std::vector<uint8_t> peer_direct;
  // a member's replication events, per peer: copies started / done (device
  // time of the copies, read after the pairs phase) and whether they are live
  std::vector<hipEvent_t> rep_start, rep_done;
  std::vector<char> rep_live;
  // recorded on `stream` when this member's rows of the call are final
  // (sketch phase done): the other members' replication copies wait on it
  hipEvent_t rows_ready = nullptr;
  hipStream_t copy_stream = nullptr;  // run-table uploads beside work on `stream` (sketch_core)
  hipEvent_t copy_done = nullptr;
  // host threads for file ingest (<= 0: gg_pack_files' default)
  int host_threads = 0;
  // wall-clock phases of the last fused call (GG_PHASE_*)
  double phase_ms[GG_PHASE_COUNT] = {0};
};

// A collection resident on the device (collection.cpp owns and changes it;
// query.cpp reads it).
struct gg_collection {
  gg_ctx* ctx = nullptr;  // as given to create / load
  float min_ani = 0.0f;
  uint32_t n = 0, row_cap = 0;
  uint64_t n_pairs = 0;
  uint64_t* sk = nullptr;    // [row_cap x s]
  uint32_t* lens = nullptr;  // [row_cap]
  gg_pair* pairs[2] = {nullptr, nullptr};
  float* ani[2] = {nullptr, nullptr};
  uint64_t pair_cap[2] = {0, 0};
  int cur = 0;  // the buffer that holds the list
  uint32_t grows = 0, rows_moved = 0;
};

namespace gg {

// The member that single-device entry points use on a multi-device context.
inline gg_ctx* primary(gg_ctx* c) { return c && !c->devs.empty() ? c->devs[0] : c; }

gg_status fail(gg_ctx* c, gg_status st, const std::string& msg);
gg_status hip_fail(gg_ctx* c, hipError_t e, const char* what);

#define GG_HIP(ctx, expr)                                        \
  do {                                                           \
    hipError_t _e = (expr);                                      \
    if (_e != hipSuccess) return ::gg::hip_fail((ctx), _e, #expr); \
  } while (0)

// Grow-only device scratch buffer owned by the context.
hipError_t scratch(gg_ctx* c, const char* key, size_t bytes, void** out);
template <typename T>
hipError_t scratch_t(gg_ctx* c, const char* key, size_t count, T** out) {
  void* p = nullptr;
  hipError_t e = scratch(c, key, count * sizeof(T), &p);
  *out = (T*)p;
  return e;
}
// Grow-only pinned host buffer of the context (contents not preserved).
hipError_t pinned(gg_ctx* c, size_t bytes, void** out);
// Grow-only pinned host buffer keyed by purpose (contents not preserved).
hipError_t host_scratch(gg_ctx* c, const char* key, size_t bytes, void** out);
template <typename T>
hipError_t host_scratch_t(gg_ctx* c, const char* key, size_t count, T** out) {
  void* p = nullptr;
  hipError_t e = host_scratch(c, key, count * sizeof(T), &p);
  *out = static_cast<T*>(p);
  return e;
}

// The run-table checks sketch_core applies (genome < n_genomes and
// non-decreasing, len >= k, base + len <= 16 n_words), for callers that
// read the table before sketch_core does (gg_sketch splits it by genome).
gg_status check_runs(gg_ctx* c, const gg_run* runs, uint64_t n_runs, uint32_t n_genomes, uint64_t n_words);
// K1 over device-resident packed words; runs are host metadata with genome
// indices in [0, n_genomes).  Row g of d_out / entry g of d_lens receive
// genome g, or genome g goes to row d_row_of[g] when d_row_of (device, n_genomes
// entries) is given.  Synchronises st.
gg_status sketch_core(gg_ctx* c, const uint32_t* d_words, uint64_t n_words, const gg_run* runs,
                      uint64_t n_runs, uint32_t n_genomes, uint64_t* d_out, uint32_t* d_lens,
                      const uint32_t* d_row_of, hipStream_t st);
// K2 over tiles [tb, te) of n device sketches; appends to d_out / *d_count.
// n_old in (0, n): the border instead (gg_pairs_border) -- over every tile,
// only the pairs (i < j) with j >= n_old; tb and te are not read.
gg_status pairs_core(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                     uint64_t tb, uint64_t te, float min_ani, gg_pair* d_out, uint64_t cap,
                     uint64_t* d_count, hipStream_t st, uint32_t n_old = 0);
// K2 over tiles [tb, te), passing pairs appended to res, the appended part
// in (i, j) order.
constexpr uint64_t kDeviceSortPairs = 4096;  // pairs_range_to_host sorts this many or more on the device
gg_status pairs_range_to_host(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                              uint64_t tb, uint64_t te, float min_ani, std::vector<gg_pair>& res,
                              hipStream_t st, uint32_t n_old = 0);

// The finch + finch clustering step over device-resident pairs (cluster.hip):
// rep_of[] by the rules of cluster_core.hpp.  Synchronises st.
gg_status cluster_device(gg_ctx* c, uint32_t n, const gg_pair* d_pairs, const float* d_ani, uint64_t n_pairs, float T,
                         uint32_t* d_rep_of, hipStream_t st);
// The precluster step over device-resident pairs (precluster.hip): members,
// offsets and, with d_pair_offsets, the local pairs.  Synchronises st.
gg_status preclusters_device(gg_ctx* c, uint32_t n, const gg_pair* d_pairs, uint64_t n_pairs, uint32_t* d_members,
                             uint32_t* d_offsets, uint32_t* n_sets, gg_local_pair* d_local, uint64_t* d_pair_offsets,
                             hipStream_t st);
// The f32 ANI of device-resident pairs (ani_f32.hip, by ani_core.hpp): d_ani[p]
// = gg_ani_f32 of pair p bit for bit, d_ani_f64 (may be null) the f64 before
// rounding, *n_rechecked (may be null) the entries the host recomputed.
// Synchronises st.
gg_status ani_f32_device(gg_ctx* c, const gg_pair* d_pairs, uint64_t n_pairs, float* d_ani, double* d_ani_f64,
                         uint64_t* n_rechecked, hipStream_t st);
// The host side of the flagged list behind it, for any kernel that computes
// ani::value per item (ani_flag.hpp): produce(E, list, cap, count) enqueues
// the kernel on st, which writes the f32 of every item and appends the
// flagged ones; it is run once, and once more at the exact count when the
// list was too small.  The flagged entries are then recomputed with the
// host's log and patched into d_ani (and d_ani_f64, may be null) at their
// index; mirror_m != 0: d_ani is an [mirror_m x mirror_m] matrix and the
// cell across the diagonal is patched too.  *n_flagged (may be null) the
// list's length.  Synchronises st.
struct AniFlagged;
using AniProducer = std::function<hipError_t(double E, AniFlagged* list, uint64_t cap, unsigned long long* count)>;
gg_status ani_flagged_passes(gg_ctx* c, const char* who, uint64_t n_items, const AniProducer& produce, float* d_ani,
                             double* d_ani_f64, uint32_t mirror_m, uint64_t* n_flagged, hipStream_t st);
// The dense matrix of m listed rows (ani_matrix.hip, by matrix_core.hpp):
// common / total / ani [m x m], each may be null; d_rows null: positions are
// rows 0 .. m-1.  Synchronises st.
gg_status ani_matrix_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n, const uint32_t* d_rows,
                            uint32_t m, uint32_t* d_common, uint32_t* d_total, float* d_ani, gg_matrix_summary* sum,
                            hipStream_t st);
// The dense matrices of many groups in one call (ani_matrix.hip, by
// matrix_core.hpp, groups): group g is d_members[offsets[g] .. offsets[g+1])
// (offsets: host words), its [m_g x m_g] block begins at the sum of the
// earlier groups' m^2.  Each output may be null.  Synchronises st.
gg_status ani_matrix_groups_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                                   const uint32_t* d_members, const uint32_t* offsets, uint32_t n_groups,
                                   uint32_t* d_common, uint32_t* d_total, float* d_ani, gg_matrix_summary* sum,
                                   hipStream_t st);
// The positions part of a matrix call (ani_matrix.hip), the one of every form,
// in context scratch until the next matrix call on the context, and the counts
// read back.  The form (matrix_core.hpp):
//   kRows    the m rows listed in d_rows (null: rows 0 .. m-1);
//   kBorder  m == n >= n_old, d_rows is not read: the new rows at the first
//            positions, the border column rule, and new_entries, the kept
//            entries of the new rows;
//   kGroups  d_rows the members of n_groups groups, group g at positions
//            d_offsets[g] .. d_offsets[g+1] (device words): columns and ids per
//            group; d_seg [n_groups + 1] device words, which receive every
//            group's first sorted entry.
struct MatrixForm {
  enum Kind { kRows, kBorder, kGroups } kind = kRows;
  uint32_t n_old = 0;
  const uint32_t* d_offsets = nullptr;
  uint32_t* d_seg = nullptr;
  uint32_t n_groups = 0;
};
struct MatrixPrep {
  const uint32_t *pos_row, *pos_len, *piece, *piece_cnt;
  uint32_t m;
  uint64_t n_entries, n_columns, column_entries;
  uint64_t new_entries = 0;
};
gg_status matrix_prepare(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                         const uint32_t* d_rows, uint32_t m, const MatrixForm& form, MatrixPrep* out, hipStream_t st);
// What the host-input forms of the matrix calls share (ani_matrix.hip): the
// argument tests in two steps, the message to `err` -- null arrays (rows too
// when rows_needed) and more positions than rows; then a sketch longer than
// sketch_size, a row index out of range and, with listed_once, one listed
// twice -- and the upload of the rows (and of `count` row indices, rows
// non-null) into context scratch, enqueued on st.
gg_status check_sketch_arrays(const std::string& w, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                              const uint32_t* rows, bool rows_needed, uint32_t count, std::string& err);
gg_status check_sketch_rows(const std::string& w, const uint32_t* lens, uint32_t n, uint32_t sketch_size,
                            const uint32_t* rows, uint32_t count, bool listed_once, std::string& err);
gg_status upload_sketch_rows(gg_ctx* c, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint32_t* rows,
                             uint32_t count, uint64_t** d_sk, uint32_t** d_len, uint32_t** d_rows, hipStream_t st);
// The host call frame of an extern "C" entry point that runs on pm =
// primary(ctx): use_device(pm) before its first HIP call, every failure
// reported on pm (fail, GG_HIP), and finish_call as its last statement: on
// failure on_failure() puts the outputs back -- the entry point's one cleanup
// -- and the message goes to ctx.  (A step that reports on ctx itself -- the
// file sketching of multi.cpp -- returns before the frame.)  Which member
// holds a copy of the message is not part of the contract.
inline gg_status use_device(gg_ctx* c, gg_ctx* report = nullptr) {
  return hipSetDevice(c->device) == hipSuccess ? GG_OK : fail(report ? report : c, GG_ERR_HIP, "hipSetDevice failed");
}
template <typename OnFailure>
gg_status finish_call(gg_ctx* ctx, gg_ctx* pm, gg_status st, const OnFailure& on_failure) {
  if (st != GG_OK) {
    on_failure();
    if (pm != ctx) ctx->err = pm->err;
  }
  return st;
}
inline gg_status finish_call(gg_ctx* ctx, gg_ctx* pm, gg_status st) {
  return finish_call(ctx, pm, st, [] {});
}
// The pair form of the product (ani_matrix.hip, matrix_core.hpp): the passing
// pairs of the prepared positions appended to d_out, gg_pairs_device's output
// contract.  d_cmin / d_sufmin: pairs_tables'.  Asynchronous.
gg_status pairs_matrix_launch(gg_ctx* c, const uint64_t* d_sk, const MatrixPrep& p, const uint32_t* d_cmin,
                              const uint32_t* d_sufmin, gg_pair* d_out, uint64_t cap, uint64_t* d_count,
                              hipStream_t st);
// The border form of it over positions prepared as a border
// of n_old = p.m - n_new.  Asynchronous.
gg_status pairs_border_matrix_launch(gg_ctx* c, const uint64_t* d_sk, const MatrixPrep& p, uint32_t n_new,
                                     const uint32_t* d_cmin, const uint32_t* d_sufmin, gg_pair* d_out, uint64_t cap,
                                     uint64_t* d_count, hipStream_t st);
// cmin / sufmin of min_ani on the device, as every pair kernel takes them
// (api.cpp's ensure_cmin; c->sufmin_host[0] == 0: some pair without a shared hash passes)
gg_status pairs_tables(gg_ctx* c, float min_ani, uint32_t** d_cmin, uint32_t** d_sufmin, hipStream_t st);
// cnt < 2^31 device pairs with row indices < n sorted by (i, j) into context
// scratch (*d_sorted); enqueued on st
gg_status sorted_pairs_device(gg_ctx* c, const gg_pair* d_pairs, uint64_t cnt, uint32_t n, gg_pair** d_sorted,
                              hipStream_t st);
// The passing pairs of n resident rows into context scratch (resident.cpp),
// by the context's pairs path (gg_set_pairs_path): K2 over every tile, or the
// pair form of the matrix product.  max(2^20, 16 n) pairs clipped to
// n (n - 1) / 2, the count read back, one retry at the exact count.  *d_out
// the pairs (unsorted), *cnt their number, *passes 1 or 2 (n < 2: nothing is
// run, 0 pairs); msum (may be null) what ran.  Synchronises st.
gg_status pairs_rows_device(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                            float min_ani, gg_pair** d_out, uint64_t* cnt, uint32_t* passes, hipStream_t st,
                            gg_pairs_matrix_summary* msum = nullptr);
// A border call (border.cpp) of n >= 2 resident rows, n_old < n, by the
// context's pairs path (resident.cpp).  *ran false: nothing
// was emitted and the caller runs the index border as ever (DEFAULT, which
// runs nothing here, or AUTO's choice after the border positions part); true:
// the border form of the matrix product gave the pairs -- appended to res in
// (i, j) order (sized passes into context scratch, sorted on the device;
// synchronises st), or appended to d_out by gg_pairs_border_device's contract
// (synchronises st once, before the product).  count_pairs_path counts the
// call for gg_pairs_paths_taken once it has succeeded.
gg_status border_routed_to_host(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                                uint32_t n_old, float min_ani, std::vector<gg_pair>& res, bool* ran, hipStream_t st);
gg_status border_routed_append(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                               uint32_t n_old, float min_ani, gg_pair* d_out, uint64_t cap, uint64_t* d_count, bool* ran,
                               hipStream_t st);
void count_pairs_path(gg_ctx* c, bool matrix);
// The sized passes of a pair producer into scratch `key`: the first at `cap`,
// one retry at the exact count.  run(d_out, cap, d_count) enqueues it on st.
// Every caller sizes through it: pairs_range_to_host (api.cpp, `who` empty:
// its messages carry no prefix), resident.cpp's calls and the collection's
// border (collection.cpp).  Any count up to `all` is returned: a caller whose
// next step takes an int count (the device sort, the ANI kernel) refuses 2^31
// pairs or more itself.  Synchronises st.
template <typename Run>
gg_status sized_pair_passes(gg_ctx* c, const std::string& who, const char* key, uint64_t all, uint64_t cap,
                            const Run& run, gg_pair** d_pairs, uint64_t* n_pairs, uint32_t* n_passes, hipStream_t st) {
  const std::string w = who.empty() ? who : who + ": ";
  gg_pair* d_out = nullptr;
  uint64_t cnt = 0;
  uint32_t passes = 0;
  uint64_t *d_count, *h_count;
  GG_HIP(c, scratch_t(c, "rs_count", 1, &d_count));
  GG_HIP(c, host_scratch_t(c, "rs_count", 1, &h_count));
  for (;;) {
    if (passes == 2) return fail(c, GG_ERR_INTERNAL, w + "pair output sizing failed");
    GG_HIP(c, scratch_t(c, key, (size_t)(cap > 1 ? cap : 1), &d_out));
    GG_HIP(c, hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
    const gg_status ps = run(d_out, cap, d_count);
    if (ps != GG_OK) return ps;
    ++passes;
    GG_HIP(c, hipMemcpyAsync(h_count, d_count, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    GG_HIP(c, hipStreamSynchronize(st));
    cnt = *h_count;
    if (cnt > all) return fail(c, GG_ERR_INTERNAL, w + "bad pair count");
    if (cnt <= cap) break;
    cap = cnt;
  }
  *d_pairs = d_out;
  *n_pairs = cnt;
  *n_passes = passes;
  return GG_OK;
}
// The files-to-rows step of every call that needs a file list's rows on the
// first member's device (multi.cpp: gg_precluster_files_resident,
// gg_precluster_matrices_files, gg_cluster_files_resident on one device;
// collection.cpp: gg_collection_add_files).  The phases are reset, the files
// sketched by sketch_files_members (cache and errors as gg_sketch_files) and
// GG_PHASE_SKETCH stamped; a multi-device context sketches on every member and
// the rows then go to the first through the host (scratch mx_h_sk / mx_h_len,
// its stream synchronised).  The first member's device is current afterwards.
// *d_sk / *d_len: context scratch of the first member, valid until its next
// call; n == 0: both null.  Every failure is reported on ctx: a caller returns
// it as it is, before its own frame.
gg_status sketch_files_first(gg_ctx* ctx, const char* const* paths, uint32_t n, const char* cache_dir,
                             const uint64_t** d_sk, const uint32_t** d_len);
// Rows resident -> rep_of resident (resident.cpp): K2 into context scratch,
// ani_f32_device, cluster_device; with sum, the partition of
// preclusters_device.  *d_pairs / *d_ani (may be null) receive the scratch
// arrays.  Synchronises st.
gg_status cluster_rows_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n, float min_ani,
                              float T, uint32_t* d_rep_of, gg_cluster_summary* sum, const gg_pair** d_pairs,
                              const float** d_ani, hipStream_t st);
// The input checks of its host-input forms (cluster.cpp; the thread's error is set).
gg_status cluster_check_input(const char* who, uint32_t n_genomes, const gg_pair* pairs, const float* ani,
                              uint64_t n_pairs, float cluster_ani, const uint32_t* rep_of);

// A batch of files inflated on m's device (inflate_host.cpp): h_in (pinned,
// in_bytes) holds files[f]'s bytes; *d_text receives the batch's FASTA text,
// file f at foff[f] (16-byte aligned, gaps '\n').  *ok = false (status GG_OK)
// when the device path does not take the batch: the caller decodes it on the
// host.  d_in: the batch already queued to the device on m->stream (at least
// in_bytes + kInflatePad bytes; nullptr: inflate_batch uploads h_in).
// Synchronises m->stream.
constexpr uint64_t kInflatePad = 4096;  // device bytes past a batch's last file (readers run past its end)
gg_status inflate_batch(gg_ctx* m, const uint8_t* h_in, uint64_t in_bytes, const std::vector<InflateFile>& files,
                        uint8_t** d_text, std::vector<uint64_t>& foff, bool* ok, uint8_t* d_in = nullptr);

// One batch of FASTA text already in device memory (d_text, file f at
// foff[f]) parsed on the device: 2-bit words into *d_words (scratch of m),
// runs of >= k bases (genome = file index in the batch) into runs.
// Synchronises m->stream.  stats (optional): the files' assembly statistics
// (src/genome_stats.rs:11-51) from two more passes over the same text; not
// asked for, the call launches the parser's three kernels only.  (multi.cpp)
gg_status parse_raw_batch(gg_ctx* m, const uint8_t* d_text, const std::vector<uint64_t>& foff, uint32_t** d_words,
                          uint64_t* n_words, std::vector<gg_run>& runs,
                          std::vector<gg_genome_stats>* stats = nullptr);

// The query of resident rows (query.hip, by query_core.hpp):
// the passing cells (row i, query q) as gg_pair{i, n + q, common, total}
// appended to d_out by gg_pairs_device's output contract.  n, nq >= 1 and
// n + nq < 2^31: the caller's.
//   query_append_device       a table of every batch of at most `batch`
//     queries (clipped to query_core.hpp's), the rows streamed against it;
//     d_cmin / d_sufmin: pairs_tables' with sufmin[0] != 0.  Synchronises st
//     once per batch (the batch's entry count sizes its sort and table).
//   query_rect_append_device  every cell, through the named-pair kernel
//     (min_ani <= 0: all pass).  Asynchronous.
gg_status query_append_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n, const uint64_t* d_q_sk,
                              const uint32_t* d_q_lens, uint32_t nq, uint32_t batch, const uint32_t* d_cmin,
                              const uint32_t* d_sufmin, gg_pair* d_out, uint64_t cap, uint64_t* d_count, hipStream_t st);
gg_status query_rect_append_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                                   const uint64_t* d_q_sk, const uint32_t* d_q_lens, uint32_t nq, gg_pair* d_out,
                                   uint64_t cap, uint64_t* d_count, hipStream_t st);
// best[q] / best_ani[q] of nq queries from their hits in any order (d_rank
// [n] or null); pairs that name no row < n or no query are skipped.  Asynchronous.
gg_status query_best_device(gg_ctx* c, uint32_t n, uint32_t nq, const gg_pair* d_pairs, const float* d_ani,
                            uint64_t n_pairs, const uint32_t* d_rank, gg_pair* d_best, float* d_best_ani, hipStream_t st);

// A timing event of c (a spare one, else a new one; nullptr on failure).
hipEvent_t take_event(gg_ctx* c);
// Runs `launch` (which enqueues one kernel on st); when timing is enabled
// brackets it with events recorded on the same stream (gg_timing_read).
template <typename F>
hipError_t timed_launch(gg_ctx* c, int kernel, uint64_t work, hipStream_t st, F&& launch) {
  if (!c->timing) return launch();
  hipEvent_t a = take_event(c), b = take_event(c);
  if (!a || !b) return hipErrorOutOfMemory;
  hipError_t e = hipEventRecord(a, st);
  if (e != hipSuccess) return e;
  e = launch();
  if (e != hipSuccess) return e;
  e = hipEventRecord(b, st);
  if (e != hipSuccess) return e;
  c->timed.push_back(gg_ctx::Timed{kernel, a, b, work});
  return hipSuccess;
}

// Records m->rows_ready on m->stream (after the member's sketching).
gg_status mark_rows_ready(gg_ctx* m);

// Helper context i >= 1 of single-device context m: the same device, k, s
// and seed, its own stream and scratch (api.cpp; owned by m).
gg_ctx* lane_ctx(gg_ctx* m, size_t i);

// The file list of one device-inflate ingest call, shared by every member
// and lane (ingest_gz.cpp).  Files are claimed one at a time, so each batch
// is cut at its size limits whatever the number of stagers; a claimed file
// that does not fit its batch is given back and claimed again first.
struct GzClaims {
  const char* const* paths = nullptr;  // the files to sketch (not found in the cache)
  const uint32_t* row_of = nullptr;    // their rows in the call's sketch array
  uint32_t n = 0;
  const char* cache_dir = nullptr;     // new sketches stored there (files stamped before they are read)
  gg_genome_stats* stats = nullptr;    // gg_sketch_files_stats: the files' statistics, by row (else null)
  std::mutex mu;
  uint32_t cursor = 0;
  std::vector<uint32_t> back;  // claimed, given back
  std::vector<uint32_t> abandoned;  // placed in a batch that was dropped undecoded
  uint32_t batches = 0;        // batches begun (the first ones are cut smaller)
  // the tail of the list cut into equal batches, a multiple of the stagers
  // (members x lanes), so that they finish together instead of the last
  // lane running a full batch alone
  uint32_t stagers = 1;
  uint64_t seen_files = 0, seen_bytes = 0;  // files staged so far, their bytes
  uint32_t tail_cap = 0;                    // files per batch from the tail on (0: not there yet)
  bool stop = false;           // no more claims: a failure
  // the failing file with the lowest index (a file that did not read, or
  // did not decode or parse on the host): the call's error, as a serial
  // reader meets it
  uint32_t err_idx = UINT32_MAX;
  gg_status err_st = GG_OK;
  std::string err_msg;
  bool claim(uint32_t* i);
  void give_back(uint32_t i);
  void abandon(const std::vector<uint32_t>& idx);
  void file_error(uint32_t i, gg_status st, const std::string& msg);
  void halt();
};
// Inflate lanes per device (GALAHGPU_GZ_LANES, default 2).
int gz_lane_count();
// Member m's share of the list: inflated, parsed and sketched on m's device
// by several lanes at once, rows into d_sk / d_len (m's [n x s] arrays);
// the rows sketched are appended to owned.  host_threads: the host threads
// this member may use (staging reads, host decodes).
gg_status gz_member_ingest(gg_ctx* m, GzClaims& cl, uint64_t* d_sk, uint32_t* d_len, int host_threads,
                           std::vector<uint32_t>& owned);
// After a file error: files given back (never read) below the failing index
// are read on the host, so the lowest failing index is reported.
void gz_settle_errors(GzClaims& cl);
// Whether a file list takes the device inflate: GALAHGPU_INFLATE=device /
// host, else when one of its first files is gzip (by its magic bytes).
bool gz_device_list(const char* const* paths, uint32_t n);

// A call's library-owned outputs (gg_free): max(count, 1) elements holding a
// host vector (null: out of memory), or the first cnt elements of a device
// array, their copy enqueued on st; free_out frees and nulls those of a call
// that fails after it made them (its on_failure; null arguments are skipped).
template <typename T>
T* copy_out(const std::vector<T>& v) {
  T* p = (T*)malloc(std::max<size_t>(v.size(), 1) * sizeof(T));
  if (p && !v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}
template <typename T>
gg_status copy_out(gg_ctx* c, const T* d_src, uint64_t cnt, T** out, hipStream_t st) {
  *out = (T*)malloc(std::max<uint64_t>(cnt, 1) * sizeof(T));
  if (!*out) return fail(c, GG_ERR_OUT_OF_MEMORY, "out of host memory");
  if (cnt) GG_HIP(c, hipMemcpyAsync(*out, d_src, cnt * sizeof(T), hipMemcpyDeviceToHost, st));
  return GG_OK;
}
template <typename... T>
void free_out(T**... out) {
  ((out ? (free(*out), *out = nullptr, 0) : 0), ...);
}

}  // namespace gg
