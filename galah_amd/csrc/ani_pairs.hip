// Named-pair ANI and cluster validation.
//
// The all-pairs kernels answer "which pairs reach a threshold"; galah also
// asks for the value of pairs it names, whatever that value is:
//   src/lib.rs:29-37                 ClusterDistanceFinder::calculate_ani(fasta1, fasta2)
//   src/cluster_validation.rs:7-78   validate_clusters: every member against
//     its representative (:21-45), every pair of representatives (:47-77).
//
// Kernel: one wave per listed pair, a grid-stride loop over the list, one
// launch per list.  finch's merge (src/finch.rs:57) ends when the row with
// the smaller last element (T) is exhausted, so (validate_core.hpp)
//   common = |T n S|,  total = |T| + #{s in S : s <= last T} - common.
// The wave copies S into its own LDS slice when it fits, its lanes stream T
// coalesced and binary-search each element in the slice with 8-byte LDS
// reads; one more search, of last T, gives the rank.  A row longer than the
// slice is searched where it lies (global memory; an 8-96 KB row stays in
// L2).  Every pair owns its output slot: no atomics, no workgroup waits for
// another, no __syncthreads (the waves of a block run different numbers of
// pairs).  The device writes the integers only; no device log produces a
// value: the f32 ANI is gg_ani_f32 of those integers, on the host.
//
// Rows must be ascending without repeats (what a sketch is); with a repeat
// the merge and the searches would count differently.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "context.hpp"
#include "device_util.hpp"
#include "gg_internal.hpp"
#include "validate_core.hpp"

namespace gg {
namespace {

constexpr int kAniBlock = 256;
constexpr int kAniWaves = kAniBlock / 64;
// LDS slice of a wave, in hashes: 2,048 x 8 B = 16 KiB, 64 KiB per
// workgroup, so two workgroups fit a CU's 160 KiB.  Smaller sketch sizes
// take a slice of their own size (a multiple of 2 hashes: every slice starts
// 16-byte aligned in the dynamic region, which holds all of the kernel's LDS).
constexpr uint32_t kAniSliceMax = 2048;
constexpr uint32_t kAniGridMax = 2048;  // 8,192 waves: 8 per SIMD of 256 CUs

struct AniPairsLaunch {
  const uint64_t* sketches;
  const uint32_t* lens;
  uint32_t n;
  uint32_t stride;  // u64 per sketch row (= sketch size)
  gg_pair* list;
  uint64_t m;
  uint32_t slice;   // hashes per wave slice
};

// Orders a wave's own LDS writes before its reads of other lanes' entries
// (and the reads before the next pair's writes).  The LDS serves a wave's
// accesses in order; this keeps the compiler from moving them.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// |T n S| (wave-uniform result): lane l takes T[l], T[l + 64], ...
template <typename Ptr>
__device__ __forceinline__ uint32_t count_common(const uint64_t* __restrict__ T, uint32_t lt, Ptr S, uint32_t ls,
                                                 uint32_t hibit, uint32_t lane) {
  uint32_t c = 0;
  for (uint32_t e = lane; e < lt; e += 64) {
    const uint64_t v = T[e];
    const uint32_t r = validate::rank_le(S, ls, hibit, v);
    c += (r != 0 && S[r - 1] == v) ? 1u : 0u;
  }
  return wave_sum(c);
}

__global__ __launch_bounds__(kAniBlock) void ani_pairs_kernel(AniPairsLaunch a) {
  extern __shared__ __align__(16) uint8_t ani_smem[];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t* slice = reinterpret_cast<uint64_t*>(ani_smem) + (size_t)wave * a.slice;
  const uint64_t waves = (uint64_t)gridDim.x * kAniWaves;
  for (uint64_t p = (uint64_t)blockIdx.x * kAniWaves + wave; p < a.m; p += waves) {
    const uint32_t i = uni32(a.list[p].i), j = uni32(a.list[p].j);
    uint32_t common = 0, total = 0;
    if (i < a.n && j < a.n) {  // (an out-of-range pair is never followed)
      const uint32_t la = min(uni32(a.lens[i]), a.stride), lb = min(uni32(a.lens[j]), a.stride);
      if (la != 0 && lb != 0) {
        if (i == j) {
          common = total = la;
        } else {
          const uint64_t* A = a.sketches + (uint64_t)i * a.stride;
          const uint64_t* B = a.sketches + (uint64_t)j * a.stride;
          const uint64_t lastA = uni64(A[la - 1]), lastB = uni64(B[lb - 1]);
          const bool a_ends = lastA <= lastB;  // A is exhausted first (or both together)
          const uint64_t* T = a_ends ? A : B;
          const uint64_t* S = a_ends ? B : A;
          const uint32_t lt = a_ends ? la : lb, ls = a_ends ? lb : la;
          const uint64_t lastT = a_ends ? lastA : lastB;
          const uint32_t hibit = validate::hibit_of(ls);
          uint32_t rank;
          if (ls <= a.slice) {
            for (uint32_t e = lane; e < ls; e += 64) slice[e] = S[e];
            wave_lds_sync();
            common = count_common(T, lt, (const uint64_t*)slice, ls, hibit, lane);
            rank = validate::rank_le((const uint64_t*)slice, ls, hibit, lastT);
            wave_lds_sync();
          } else {
            common = count_common(T, lt, S, ls, hibit, lane);
            rank = validate::rank_le(S, ls, hibit, lastT);
          }
          total = validate::total_from_rank(lt, rank, common);
        }
      }
    }
    if (lane == 0) {
      a.list[p].common = common;
      a.list[p].total = total;
    }
  }
}

hipError_t launch_ani_pairs(const AniPairsLaunch& a, hipStream_t st) {
  if (a.m == 0) return hipSuccess;
  const size_t lds = (size_t)kAniWaves * a.slice * sizeof(uint64_t);
  hipError_t e =
      hipFuncSetAttribute((const void*)ani_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(kAniGridMax, (a.m + kAniWaves - 1) / kAniWaves);
  hipLaunchKernelGGL(ani_pairs_kernel, dim3(grid), dim3(kAniBlock), lds, st, a);
  return hipGetLastError();
}

// GALAHGPU_ANI_PAIRS_LDS=0 leaves every row in global memory (A/B runs and
// the tests of that path at small sketch sizes); results never depend on it.
uint32_t ani_slice(uint32_t s) {
  const char* e = getenv("GALAHGPU_ANI_PAIRS_LDS");
  if (e && strcmp(e, "0") == 0) return 0;
  return std::min(kAniSliceMax, (s + 1u) & ~1u);
}

// (common, total) of list[0 .. m) on c's device, timed as GG_KERNEL_ANI_PAIRS.  Async.
gg_status ani_pairs_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n, gg_pair* d_list,
                           uint64_t m, hipStream_t st) {
  if (m == 0) return GG_OK;
  AniPairsLaunch a{d_sk, d_lens, n, c->s, d_list, m, ani_slice(c->s)};
  GG_HIP(c, timed_launch(c, GG_KERNEL_ANI_PAIRS, m, st, [&] { return launch_ani_pairs(a, st); }));
  return GG_OK;
}

// ---- checks of the host-input forms (the message goes to `err`) -----------
gg_status check_rows(const std::string& w, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                     uint32_t sketch_size, int k, std::string& err) {
  if (n && (!sketches || !lens)) {
    err = w + ": null argument";
    return GG_ERR_INVALID_ARG;
  }
  if (k < 1 || k > 32 || sketch_size < 1) {
    err = w + ": kmer_length must be 1..32 and sketch_size at least 1";
    return GG_ERR_INVALID_ARG;
  }
  for (uint32_t g = 0; g < n; ++g)
    if (lens[g] > sketch_size) {
      err = w + ": sketch longer than sketch_size";
      return GG_ERR_INVALID_ARG;
    }
  return GG_OK;
}

gg_status check_list(const std::string& w, uint32_t n, const gg_pair* list, uint64_t m, std::string& err) {
  if (m && !list) {
    err = w + ": null argument";
    return GG_ERR_INVALID_ARG;
  }
  if (m >= (1ull << 31)) {
    err = w + ": 2^31 pairs or more";
    return GG_ERR_INVALID_ARG;
  }
  for (uint64_t p = 0; p < m; ++p)
    if (list[p].i >= n || list[p].j >= n) {
      err = w + ": pair index out of range";
      return GG_ERR_INVALID_ARG;
    }
  return GG_OK;
}

gg_status check_clusters(const std::string& w, uint32_t n, const uint32_t* members, const uint32_t* offsets,
                         uint32_t n_clusters, float ani, const gg_validation* sum, gg_pair** bad, float** bad_ani,
                         uint64_t* n_bad, std::string& err) {
  if (!sum || !bad || !bad_ani || !n_bad || !offsets || (n_clusters && !members)) {
    err = w + ": null argument";
    return GG_ERR_INVALID_ARG;
  }
  if (std::isnan(ani)) {
    err = w + ": ani is NaN";
    return GG_ERR_INVALID_ARG;
  }
  for (uint32_t c = 0; c < n_clusters; ++c)
    if (offsets[c + 1] <= offsets[c]) {
      err = w + ": empty cluster or offsets not ascending";
      return GG_ERR_INVALID_ARG;
    }
  if (n_clusters && (uint64_t)offsets[n_clusters] - offsets[0] >= (1ull << 31)) {
    err = w + ": 2^31 listed genomes or more";
    return GG_ERR_INVALID_ARG;
  }
  for (uint32_t x = n_clusters ? offsets[0] : 0; n_clusters && x < offsets[n_clusters]; ++x)
    if (members[x] >= n) {
      err = w + ": genome index out of range";
      return GG_ERR_INVALID_ARG;
    }
  return GG_OK;
}

void fill_ani(const gg_pair* list, uint64_t m, int k, float* ani) {
  for (uint64_t p = 0; p < m; ++p) ani[p] = (float)ani_f64(list[p].common, list[p].total, k);
}

// The two halves of a validation, each a list of evaluated pairs in output
// order, put through the rule and handed out.
gg_status finish_validation(const std::vector<gg_pair>& member_list, std::vector<gg_pair>& rep_pairs, uint32_t R, int k,
                            float ani, gg_validation* sum, gg_pair** bad, float** bad_ani, uint64_t* n_bad,
                            std::string& err) {
  std::vector<gg_pair> out;
  std::vector<float> out_ani;
  sum->member_pairs = member_list.size();
  sum->member_bad = 0;
  for (const gg_pair& p : member_list) {
    const float v = (float)ani_f64(p.common, p.total, k);
    if (!validate::member_bad(v, ani)) continue;
    out.push_back(p);
    out_ani.push_back(v);
    ++sum->member_bad;
  }
  std::sort(rep_pairs.begin(), rep_pairs.end(),
            [](const gg_pair& x, const gg_pair& y) { return x.i != y.i ? x.i < y.i : x.j < y.j; });
  sum->rep_pairs = (uint64_t)R * (R ? R - 1 : 0) / 2;
  sum->rep_bad = 0;
  for (const gg_pair& p : rep_pairs) {
    const float v = (float)ani_f64(p.common, p.total, k);
    if (!validate::reps_bad(v, ani)) continue;
    out.push_back(p);
    out_ani.push_back(v);
    ++sum->rep_bad;
  }
  *bad = copy_out(out);
  *bad_ani = copy_out(out_ani);
  if (!*bad || !*bad_ani) {
    free(*bad);
    free(*bad_ani);
    *bad = nullptr;
    *bad_ani = nullptr;
    err = "out of host memory";
    return GG_ERR_OUT_OF_MEMORY;
  }
  *n_bad = out.size();
  return GG_OK;
}

std::vector<gg_pair> member_list_of(const uint32_t* members, const uint32_t* offsets, uint32_t n_clusters) {
  const std::vector<validate::NamedPair> named = validate::member_pairs(members, offsets, n_clusters);
  std::vector<gg_pair> list(named.size());
  for (size_t p = 0; p < named.size(); ++p) list[p] = gg_pair{named[p].rep, named[p].member, 0, 0};
  return list;
}

// A pair of clusters (a < b, positions among the representatives) as the
// pair of their genomes, smaller first.
gg_pair rep_pair_of(const uint32_t* members, const uint32_t* offsets, uint32_t a, uint32_t b, uint32_t common,
                    uint32_t total) {
  const uint32_t ga = members[offsets[a]], gb = members[offsets[b]];
  return gg_pair{std::min(ga, gb), std::max(ga, gb), common, total};
}

gg_status ani_pairs_ctx(gg_ctx* m, const uint64_t* sketches, const uint32_t* lens, uint32_t n, gg_pair* list,
                        uint64_t cnt, float* ani) {
  std::string err;
  gg_status st = check_rows("gg_ani_pairs", sketches, lens, n, m->s, m->k, err);
  if (st == GG_OK) st = check_list("gg_ani_pairs", n, list, cnt, err);
  if (st != GG_OK) return fail(m, st, err);
  if (cnt == 0) return GG_OK;
  st = use_device(m);
  if (st != GG_OK) return st;
  uint64_t* d_sk = nullptr;
  uint32_t* d_len = nullptr;
  gg_pair* d_list = nullptr;
  GG_HIP(m, scratch_t(m, "ap_sk", (size_t)n * m->s, &d_sk));
  GG_HIP(m, scratch_t(m, "ap_len", (size_t)n, &d_len));
  GG_HIP(m, scratch_t(m, "ap_list", (size_t)cnt, &d_list));
  GG_HIP(m, hipMemcpyAsync(d_sk, sketches, (size_t)n * m->s * sizeof(uint64_t), hipMemcpyHostToDevice, m->stream));
  GG_HIP(m, hipMemcpyAsync(d_len, lens, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
  GG_HIP(m, hipMemcpyAsync(d_list, list, cnt * sizeof(gg_pair), hipMemcpyHostToDevice, m->stream));
  st = ani_pairs_device(m, d_sk, d_len, n, d_list, cnt, m->stream);
  if (st != GG_OK) return st;
  GG_HIP(m, hipMemcpyAsync(list, d_list, cnt * sizeof(gg_pair), hipMemcpyDeviceToHost, m->stream));
  GG_HIP(m, hipStreamSynchronize(m->stream));
  if (ani) fill_ani(list, cnt, m->k, ani);
  return GG_OK;
}

}  // namespace
}  // namespace gg

using namespace gg;

extern "C" {

gg_status gg_ani_pairs_host(const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t sketch_size,
                            int kmer_length, gg_pair* list, uint64_t m, float* ani) {
  std::string err;
  gg_status st = check_rows("gg_ani_pairs_host", sketches, lens, n, sketch_size, kmer_length, err);
  if (st == GG_OK) st = check_list("gg_ani_pairs_host", n, list, m, err);
  if (st != GG_OK) {
    set_thread_error(err);
    return st;
  }
  for (uint64_t p = 0; p < m; ++p) {
    const uint32_t i = list[p].i, j = list[p].j;
    validate::merge_counts(sketches + (size_t)i * sketch_size, lens[i], sketches + (size_t)j * sketch_size, lens[j],
                           &list[p].common, &list[p].total);
  }
  if (ani) fill_ani(list, m, kmer_length, ani);
  return GG_OK;
}

gg_status gg_ani_pairs(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n, gg_pair* list,
                       uint64_t m, float* ani) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  return finish_call(ctx, pm, ani_pairs_ctx(pm, sketches, lens, n, list, m, ani));
}

gg_status gg_ani_pairs_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                              gg_pair* d_list, uint64_t m, void* stream) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  gg_status st = GG_OK;
  if (m && (!d_list || (n && (!d_sketches || !d_lens))))
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_ani_pairs_device: null buffer");
  else if ((st = use_device(pm)) == GG_OK)
    st = ani_pairs_device(pm, d_sketches, d_lens, n, d_list, m, (hipStream_t)stream);
  return finish_call(ctx, pm, st);
}

gg_status gg_validate_clusters_host(const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t sketch_size,
                                    int kmer_length, const uint32_t* members, const uint32_t* offsets,
                                    uint32_t n_clusters, float ani, gg_validation* sum, gg_pair** bad, float** bad_ani,
                                    uint64_t* n_bad) {
  std::string err;
  gg_status st = check_rows("gg_validate_clusters_host", sketches, lens, n, sketch_size, kmer_length, err);
  if (st == GG_OK)
    st = check_clusters("gg_validate_clusters_host", n, members, offsets, n_clusters, ani, sum, bad, bad_ani, n_bad,
                        err);
  if (st != GG_OK) {
    set_thread_error(err);
    return st;
  }
  *bad = nullptr;
  *bad_ani = nullptr;
  *n_bad = 0;
  auto merge = [&](uint32_t i, uint32_t j, gg_pair* p) {
    validate::merge_counts(sketches + (size_t)i * sketch_size, lens[i], sketches + (size_t)j * sketch_size, lens[j],
                           &p->common, &p->total);
  };
  std::vector<gg_pair> list = member_list_of(members, offsets, n_clusters);
  for (gg_pair& p : list) merge(p.i, p.j, &p);
  // every pair of representatives (:47-77), kept when the rule may hold
  std::vector<gg_pair> reps;
  for (uint32_t a = 0; a < n_clusters; ++a)
    for (uint32_t b = a + 1; b < n_clusters; ++b) {
      gg_pair p = rep_pair_of(members, offsets, a, b, 0, 0);
      merge(p.i, p.j, &p);
      if (validate::reps_bad((float)ani_f64(p.common, p.total, kmer_length), ani)) reps.push_back(p);
    }
  st = finish_validation(list, reps, n_clusters, kmer_length, ani, sum, bad, bad_ani, n_bad, err);
  if (st != GG_OK) set_thread_error(err);
  return st;
}

gg_status gg_validate_clusters(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                               const uint32_t* members, const uint32_t* offsets, uint32_t n_clusters, float ani,
                               gg_validation* sum, gg_pair** bad, float** bad_ani, uint64_t* n_bad) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  std::string err;
  gg_status st = check_rows("gg_validate_clusters", sketches, lens, n, pm->s, pm->k, err);
  if (st == GG_OK)
    st = check_clusters("gg_validate_clusters", n, members, offsets, n_clusters, ani, sum, bad, bad_ani, n_bad, err);
  if (st != GG_OK) return fail(ctx, st, err);
  *bad = nullptr;
  *bad_ani = nullptr;
  *n_bad = 0;
  const uint32_t s = pm->s;
  // members: the named list through the named-pair kernel (first member)
  std::vector<gg_pair> list = member_list_of(members, offsets, n_clusters);
  st = ani_pairs_ctx(pm, sketches, lens, n, list.data(), list.size(), nullptr);
  if (st != GG_OK) return finish_call(ctx, pm, st);
  // representatives: their rows gathered, through the all-pairs path at the
  // superset threshold (validate_core.hpp), then the f32 rule
  std::vector<gg_pair> reps;
  if (n_clusters >= 2) {
    std::vector<uint64_t> rows((size_t)n_clusters * s);
    std::vector<uint32_t> rlens(n_clusters);
    for (uint32_t c = 0; c < n_clusters; ++c) {
      const uint32_t g = members[offsets[c]];
      memcpy(rows.data() + (size_t)c * s, sketches + (size_t)g * s, (size_t)s * sizeof(uint64_t));
      rlens[c] = lens[g];
    }
    gg_pair* found = nullptr;
    uint64_t n_found = 0;
    st = gg_pairs(ctx, rows.data(), rlens.data(), n_clusters, validate::superset_threshold(ani), &found, &n_found);
    if (st != GG_OK) return st;
    reps.reserve(n_found);
    for (uint64_t p = 0; p < n_found; ++p)
      reps.push_back(rep_pair_of(members, offsets, found[p].i, found[p].j, found[p].common, found[p].total));
    gg_free(found);
  }
  st = finish_validation(list, reps, n_clusters, pm->k, ani, sum, bad, bad_ani, n_bad, err);
  if (st != GG_OK) return fail(ctx, st, err);
  return GG_OK;
}

gg_status gg_validate_files(gg_ctx* ctx, const char* const* paths, uint32_t n_paths, const uint32_t* members,
                            const uint32_t* offsets, uint32_t n_clusters, float ani, const char* cache_dir,
                            gg_validation* sum, gg_pair** bad, float** bad_ani, uint64_t* n_bad) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  if (n_paths && !paths) return fail(ctx, GG_ERR_INVALID_ARG, "gg_validate_files: null argument");
  const uint32_t s = primary(ctx)->s;
  std::vector<uint64_t> rows((size_t)std::max<uint32_t>(n_paths, 1) * s);
  std::vector<uint32_t> rlens(std::max<uint32_t>(n_paths, 1));
  const gg_status st = gg_sketch_files(ctx, paths, n_paths, cache_dir, rows.data(), rlens.data(), nullptr);
  if (st != GG_OK) return st;
  return gg_validate_clusters(ctx, rows.data(), rlens.data(), n_paths, members, offsets, n_clusters, ani, sum, bad,
                              bad_ani, n_bad);
}

}  // extern "C"
