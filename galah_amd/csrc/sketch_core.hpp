// The tail of K1's hash and its tau prefilter, stated once
// for the kernel (sketch.hip) and a stand-alone host test
// (tests/cpp/test_sketch_core.cpp): everything of the tau test that touches
// no LDS.
//
// murmur3's fmix64 is k ^= k >> 33; k *= C1; k ^= k >> 33; k *= C2;
// k ^= k >> 33.  hash_parts (sketch.hip) returns the two finaliser states
// after their first multiply, y_i = fmix64_mid(h_i); with p_i = y_i * C2 (mod
// 2^64) and L(k) = k ^ (k >> 33) the hash is
//   h = L(p1) + L(p2)                                   (mod 2^64).
//
// The prefilter decides from one multiply chain on y1 + y2 whether h can be
// <= tau:
//   * L leaves the high word alone, so hi(h) = hi(p1) + hi(p2) + c' (mod
//     2^32), c' in {0, 1} the carry of the xor-shifted low words;
//   * P = (y1 + y2) * C2 = p1 + p2 (mod 2^64), so hi(P) = hi(p1) + hi(p2) +
//     c'' (mod 2^32), c'' in {0, 1} the carry of the raw low words;
//   * hence hi(h) - hi(P) in {-1, 0, +1} (mod 2^32), and h <= tau, which needs
//     hi(h) <= hi(tau), needs hi(P) in [-1, hi(tau) + 1] (mod 2^32), that is
//     hi(P) + 1 (mod 2^32) <= hi(tau) + 2;
//   * when hi(tau) >= 2^32 - 3 that window is every value: everything passes.
// The test has no false negatives; what passes it takes the exact test
// exact_hash(y1, y2) <= tau.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GG_SKETCH_HD __host__ __device__
#else
#define GG_SKETCH_HD
#endif

namespace gg {
namespace sketch {

GG_SKETCH_HD inline uint64_t fmix_last(uint64_t k) { return k ^ (k >> 33); }

// fmix64 up to its second multiply: fmix64(k) = fmix_last(fmix64_mid(k) * kFmixC2)
constexpr uint64_t kFmixC2 = 0xc4ceb9fe1a85ec53ull;
GG_SKETCH_HD inline uint64_t fmix64_mid(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  return k ^ (k >> 33);
}

GG_SKETCH_HD inline uint32_t mul_hi_u32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// high word of y * kFmixC2 (mod 2^64) without the low word: one v_mul_hi_u32
// and two v_mul_lo_u32 instead of a v_mad_u64_u32 and two v_mul_lo_u32
GG_SKETCH_HD inline uint32_t hi_times_c2(uint64_t y) {
  const uint32_t lo = (uint32_t)y, hi = (uint32_t)(y >> 32);
  return mul_hi_u32(lo, (uint32_t)kFmixC2) + lo * (uint32_t)(kFmixC2 >> 32) + hi * (uint32_t)kFmixC2;
}

// the hash of a k-mer from its two finaliser states
GG_SKETCH_HD inline uint64_t exact_hash(uint64_t f1, uint64_t f2) {
  return fmix_last(f1 * kFmixC2) + fmix_last(f2 * kFmixC2);
}

// hi(P) + 1 (mod 2^32) of the k-mer with finaliser states f1, f2 (the sum
// wraps mod 2^64)
GG_SKETCH_HD inline uint32_t prefilter_word(uint64_t f1, uint64_t f2) { return hi_times_c2(f1 + f2) + 1u; }

// exact_hash(f1, f2) <= tau implies prefilter_word(f1, f2) <= prefilter_threshold(tau)
GG_SKETCH_HD inline uint32_t prefilter_threshold(uint64_t tau) {
  const uint32_t tau_hi = (uint32_t)(tau >> 32);
  return tau_hi >= 0xFFFFFFFDu ? 0xFFFFFFFFu : tau_hi + 2u;
}

}  // namespace sketch
}  // namespace gg
