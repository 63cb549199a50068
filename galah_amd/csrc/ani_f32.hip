// The f32 ANI of device-resident pairs: d_ani[p] =
// gg_ani_f32(common, total, k) bit for bit, by the rule of ani_core.hpp.
//
//   ani_f32_kernel    one pair per thread in a grid-stride loop: the 16-byte
//                     gg_pair read as one 128-bit load (a wave reads 1 KB
//                     contiguous), the f32 (and, when asked for, the f64)
//                     stored coalesced.  An entry the margin test flags goes
//                     to a list in context scratch (ani_flag.hpp): one ballot
//                     and one atomicAdd per wave, the wave's flagged lanes
//                     write {index, common, total}; entries past the list's
//                     capacity are dropped and the counter says so.
//   ani_patch_kernel  d_ani[list[q].index] = val[q] for the entries the host
//                     recomputed (of a mirrored matrix, the cell across the
//                     diagonal too).
//
// The host side, ani_flagged_passes, is shared with the dense matrix
// (ani_matrix.hip), whose product kernel is the producer there: it reads the
// counter back, runs the producer once more when the list was too small (at
// the exact count: at most two passes), recomputes the listed entries with
// the host's log and patches them in.  No workgroup waits for another.  The
// kernels are launched plainly (no gg_timing_read slot).
#include <algorithm>
#include <cstdlib>

#include "ani_core.hpp"
#include "ani_flag.hpp"
#include "context.hpp"

namespace gg {
namespace {

__global__ __launch_bounds__(256) void ani_f32_kernel(const gg_pair* __restrict__ pairs, uint64_t n_pairs, int k,
                                                      double E, float* __restrict__ out, double* __restrict__ out64,
                                                      AniFlagged* __restrict__ list, uint64_t cap,
                                                      unsigned long long* __restrict__ count) {
  // (the loop's bound is the workgroup's, so that whole waves reach the ballot)
  for (uint64_t base = (uint64_t)blockIdx.x * 256; base < n_pairs; base += (uint64_t)gridDim.x * 256) {
    const uint64_t p = base + threadIdx.x;
    uint32_t common = 0, total = 0;
    bool flagged = false;
    if (p < n_pairs) {
      const uint4 x = reinterpret_cast<const uint4*>(pairs)[p];
      common = x.z;
      total = x.w;
      const ani::Value r = ani::value(common, total, k, E, DeviceLog{});
      out[p] = r.f;
      if (out64) out64[p] = r.v;
      flagged = r.flagged;
    }
    ani_flag_push(flagged, (uint32_t)p, common, total, list, cap, count);
  }
}

// (mirror_m != 0: out is an [mirror_m x mirror_m] matrix, index = a * mirror_m + b, and (b, a) is patched too)
__global__ __launch_bounds__(256) void ani_patch_kernel(const AniFlagged* __restrict__ list, uint64_t n,
                                                        const float* __restrict__ val,
                                                        const double* __restrict__ val64, float* __restrict__ out,
                                                        double* __restrict__ out64, uint32_t mirror_m) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (uint64_t)gridDim.x * 256) {
    const uint32_t p = list[q].index;
    out[p] = val[q];
    if (out64) out64[p] = val64[q];
    if (mirror_m) out[(uint64_t)(p % mirror_m) * mirror_m + p / mirror_m] = val[q];
  }
}

inline dim3 grid_for(uint64_t items) { return dim3((uint32_t)std::min<uint64_t>(8192, (items + 255) / 256)); }

}  // namespace

gg_status ani_flagged_passes(gg_ctx* c, const char* who, uint64_t n_items, const AniProducer& produce, float* d_ani,
                             double* d_ani_f64, uint32_t mirror_m, uint64_t* n_flagged, hipStream_t st) {
  if (n_flagged) *n_flagged = 0;
  if (n_items == 0) return GG_OK;
  // (tests: another margin, 2^value, so that every entry is flagged and the first list overflows)
  int margin = ani::kMarginLog2;
  if (const char* e = getenv("GALAHGPU_TEST_ANI_MARGIN_LOG2")) margin = std::max(-1000, std::min(1000, atoi(e)));
  const double E = ani::pow2(margin);
  unsigned long long *d_count, *h_count;
  GG_HIP(c, scratch_t(c, "ani_count", 1, &d_count));
  GG_HIP(c, host_scratch_t(c, "ani_count", 1, &h_count));
  uint64_t cap = std::max<uint64_t>(4096, n_items >> 12), cnt = 0;
  AniFlagged* d_list = nullptr;
  for (int attempt = 0;; ++attempt) {
    if (attempt == 2) return fail(c, GG_ERR_INTERNAL, std::string(who) + ": list sizing failed");
    GG_HIP(c, scratch_t(c, "ani_list", (size_t)cap, &d_list));
    GG_HIP(c, hipMemsetAsync(d_count, 0, sizeof *d_count, st));
    GG_HIP(c, produce(E, d_list, cap, d_count));
    GG_HIP(c, hipMemcpyAsync(h_count, d_count, sizeof *d_count, hipMemcpyDeviceToHost, st));
    GG_HIP(c, hipStreamSynchronize(st));
    cnt = *h_count;
    if (cnt > n_items) return fail(c, GG_ERR_INTERNAL, std::string(who) + ": bad flagged count");
    if (cnt <= cap) break;
    cap = cnt;  // the exact count: the second pass fits
  }
  if (n_flagged) *n_flagged = cnt;
  if (cnt == 0 || !d_ani) return GG_OK;
  // the flagged entries by the host's log: the list down, the values up
  // (pinned: [cnt] f64, [cnt] f32, then the list)
  double* h_val64;
  GG_HIP(c, host_scratch_t(c, "ani_val", (size_t)(3 * cnt + 1), &h_val64));  // 8 + 4 + 12 bytes an entry
  float* h_val = (float*)(h_val64 + cnt);
  AniFlagged* h_list = (AniFlagged*)(h_val + cnt);
  GG_HIP(c, hipMemcpyAsync(h_list, d_list, cnt * sizeof(AniFlagged), hipMemcpyDeviceToHost, st));
  GG_HIP(c, hipStreamSynchronize(st));
  for (uint64_t q = 0; q < cnt; ++q) {
    h_val64[q] = ani_f64(h_list[q].common, h_list[q].total, c->k);
    h_val[q] = (float)h_val64[q];
  }
  double* d_val64;
  GG_HIP(c, scratch_t(c, "ani_val", (size_t)(2 * cnt), &d_val64));  // [cnt] f64, [cnt] f32
  float* d_val = (float*)(d_val64 + cnt);
  GG_HIP(c, hipMemcpyAsync(d_val64, h_val64, cnt * (sizeof(double) + sizeof(float)), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(ani_patch_kernel, grid_for(cnt), dim3(256), 0, st, d_list, cnt, d_val, d_val64, d_ani, d_ani_f64,
                     mirror_m);
  GG_HIP(c, hipGetLastError());
  GG_HIP(c, hipStreamSynchronize(st));  // (the pinned values are the next call's)
  return GG_OK;
}

gg_status ani_f32_device(gg_ctx* c, const gg_pair* d_pairs, uint64_t n_pairs, float* d_ani, double* d_ani_f64,
                         uint64_t* n_rechecked, hipStream_t st) {
  const int k = c->k;
  return ani_flagged_passes(
      c, "gg_ani_f32_device", n_pairs,
      [&](double E, AniFlagged* list, uint64_t cap, unsigned long long* count) {
        hipLaunchKernelGGL(ani_f32_kernel, grid_for(n_pairs), dim3(256), 0, st, d_pairs, n_pairs, k, E, d_ani,
                           d_ani_f64, list, cap, count);
        return hipGetLastError();
      },
      d_ani, d_ani_f64, 0, n_rechecked, st);
}

}  // namespace gg

using namespace gg;

extern "C" {

gg_status gg_ani_f32_device(gg_ctx* ctx, const gg_pair* d_pairs, uint64_t n_pairs, float* d_ani, double* d_ani_f64,
                            uint64_t* n_rechecked, void* stream) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* m = primary(ctx);
  gg_status st = GG_OK;
  if (n_rechecked) *n_rechecked = 0;
  if (n_pairs && (!d_pairs || !d_ani))
    st = fail(m, GG_ERR_INVALID_ARG, "gg_ani_f32_device: null buffer");
  else if ((uintptr_t)d_pairs % 16 != 0)
    st = fail(m, GG_ERR_INVALID_ARG, "gg_ani_f32_device: d_pairs is not 16-byte aligned");
  else if (n_pairs >= (1ull << 31))
    st = fail(m, GG_ERR_INVALID_ARG, "gg_ani_f32_device: 2^31 pairs or more");
  else if ((st = use_device(m)) == GG_OK)
    st = ani_f32_device(m, d_pairs, n_pairs, d_ani, d_ani_f64, n_rechecked, (hipStream_t)stream);
  return finish_call(ctx, m, st);
}

}  // extern "C"
