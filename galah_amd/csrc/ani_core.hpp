// The f32 ANI of a pair from its two integers, stated once
// for the kernel (ani_f32.hip), its host wrapper and a stand-alone host test
// (tests/cpp/test_ani_core.cpp).  Templated on a Log policy: std::log on the
// host, the device log in the kernel, a perturbed log in the test.
//
//   src/finch.rs:56-64  ani = 1 - mash_distance(common, total, k), f64, with
//     Rust's f64::min / f64::max (a NaN operand gives the other one);
//   src/finch.rs:70     the cache stores `ani as f32`.
//
// The value is ani_f64 of api.cpp, operation for operation.  Host and device
// differ in log only, so an entry whose f32 another log could change is
// *flagged*, and the caller recomputes it with the host's gg_ani_f32:
//   - the unclamped distance d within E of 1 (the clamp's corner);
//   - v = 1 - d within E of either f32 rounding boundary around (float)v (the
//     midpoints to its two f32 neighbours, exact in f64).
// E = 2^-44 absolute on v: a log off by a few ulp moves v by about 2^-51 at
// most (d <= 1, then one rounding of 1 - d), so E keeps more than a factor of
// 100 over that; what the device log does is measured (tests/test_resident_gpu.py).
// Decided by the integers alone, never flagged: total == 0 or common == 0
// gives 0, common >= total gives 1 (the log's argument is >= 1, d clamps to 0).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_ANI_HD __host__ __device__
#else
#define GG_ANI_HD
#endif

namespace gg {
namespace ani {

constexpr int kMarginLog2 = -44;

// 2^e for e in [-1022, 1023]
GG_ANI_HD inline double pow2(int e) {
  const uint64_t b = (uint64_t)(e + 1023) << 52;
  double x;
  __builtin_memcpy(&x, &b, sizeof x);
  return x;
}

// f64::min / f64::max of Rust: a NaN operand gives the other one
GG_ANI_HD inline double rust_min(double a, double b) {
  if (a != a) return b;
  if (b != b) return a;
  return a < b ? a : b;
}
GG_ANI_HD inline double rust_max(double a, double b) {
  if (a != a) return b;
  if (b != b) return a;
  return a > b ? a : b;
}

struct HostLog {
  double operator()(double x) const { return std::log(x); }
};

struct Value {
  double v;      // 1 - mash distance, f64
  float f;       // (float)v: final unless flagged
  bool flagged;  // another log might round differently: recompute on the host
};

template <class Log>
GG_ANI_HD inline Value value(uint32_t common, uint32_t total, int k, double E, Log lg) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (total == 0 || common == 0) return Value{0.0, 0.0f, false};
  if (common >= total) return Value{1.0, 1.0f, false};
  const double jaccard = (double)common / (double)total;
  const double d = -1.0 * lg((2.0 * jaccard) / (1.0 + jaccard)) / (double)k;
  const double v = 1.0 - rust_max(rust_min(d, 1.0), 0.0);
  const float f = (float)v;
  if (d > 1.0 + E) return Value{v, f, false};  // 0 with any log within the margin
  if (!(d < 1.0 - E)) return Value{v, f, true};
  // 0 < v < 1 here, f a positive f32: its neighbours are the next bit patterns
  uint32_t bits;
  __builtin_memcpy(&bits, &f, sizeof bits);
  const uint32_t ub = bits + 1, lb = bits - 1;
  float up, dn;
  __builtin_memcpy(&up, &ub, sizeof up);
  __builtin_memcpy(&dn, &lb, sizeof dn);
  const double hi = (double)f + ((double)up - (double)f) * 0.5;
  const double lo = (double)f - ((double)f - (double)dn) * 0.5;
  const bool near = !(hi - v > E) || !(v - lo > E);
  return Value{v, f, near};
}

}  // namespace ani
}  // namespace gg
