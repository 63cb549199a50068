// Host test of galah_amd/csrc/sketch_core.hpp: the tail of K1's hash and the
// tau prefilter on the sum of the two finaliser states.
//
//   1. exact_hash(f1, f2) = fmix64 tail of h1 + fmix64 tail of h2, murmur3's
//      finaliser written out here on its own;
//   2. hi(exact_hash) - hi((f1 + f2) * C2) is -1, 0 or +1 (mod 2^32), each
//      of the three seen;
//   3. exact_hash(f1, f2) <= tau implies prefilter_word(f1, f2) <=
//      prefilter_threshold(tau): no false negative.
//
// Cases: >= 10^6 random (f1, f2, tau), and cases built by inverting C2 so that
// P = (f1 + f2) * C2 lands on chosen values: f2 = (target - f1 * C2) * C2^-1,
// target's high word at hi(tau) + {-2 .. +3}, its low word at 0, 1, 2^32 - 2,
// 2^32 - 1 and random values, for hi(tau) in {0, 1, 2^21, 2^31 - 1, 2^32 - 4
// .. 2^32 - 1}; for each, tau's low word at 0, 2^32 - 1, the hash's own low
// word and its neighbours.  Prints "ok <cases>" and, for information, the
// prefilter's false positives among random k-mers at hi(tau) = 2^21.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../galah_amd/csrc/sketch_core.hpp"

namespace sk = gg::sketch;

namespace {

// splitmix64
struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
};

// murmur3's fmix64, from the reference implementation's text
uint64_t fmix64_ref(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}
// ... up to and including the xor-shift after its first multiply
uint64_t fmix64_ref_mid(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  return k;
}

// inverse of an odd number mod 2^64 (Newton: each step doubles the exact bits)
uint64_t inverse(uint64_t a) {
  uint64_t x = a;  // exact to 3 bits
  for (int i = 0; i < 6; ++i) x *= 2 - a * x;
  return x;
}

long long fails = 0;
long long cases = 0;
long long seen[3] = {0, 0, 0};  // hi(h) - hi(P) = -1, 0, +1
long long built_cases = 0, built_pass = 0, built_fp = 0;  // cases with hi(tau) = 2^21 (information only)

void fail(const char* what, uint64_t f1, uint64_t f2, uint64_t tau) {
  if (++fails <= 10)
    std::printf("FAIL %s: f1=%016llx f2=%016llx tau=%016llx\n", what, (unsigned long long)f1, (unsigned long long)f2,
                (unsigned long long)tau);
}

// checks 2 and 3 for one (f1, f2, tau); returns true when the prefilter passes
bool check(uint64_t f1, uint64_t f2, uint64_t tau) {
  ++cases;
  const uint64_t h = sk::exact_hash(f1, f2);
  const uint64_t P = (f1 + f2) * sk::kFmixC2;
  const uint32_t diff = (uint32_t)(h >> 32) - (uint32_t)(P >> 32);
  if (diff == 0xFFFFFFFFu) ++seen[0];
  else if (diff == 0u) ++seen[1];
  else if (diff == 1u) ++seen[2];
  else fail("high words differ by more than one", f1, f2, tau);
  if (sk::hi_times_c2(f1 + f2) != (uint32_t)(P >> 32)) fail("hi_times_c2", f1, f2, tau);
  const bool pass = sk::prefilter_word(f1, f2) <= sk::prefilter_threshold(tau);
  if (h <= tau && !pass) fail("false negative", f1, f2, tau);
  if ((uint32_t)(tau >> 32) == 1u << 21) {
    ++built_cases;
    built_pass += pass;
    built_fp += pass && h > tau;
  }
  return pass;
}

}  // namespace

int main() {
  Rng rng{20240611};
  const uint64_t c2inv = inverse(sk::kFmixC2);
  if (c2inv * sk::kFmixC2 != 1ull) {
    std::printf("FAIL inverse\n");
    return 1;
  }

  // 1. the hash's tail against murmur3's own finaliser; the header's
  // fmix64_mid against the same text
  for (int i = 0; i < 1000000; ++i) {
    uint64_t h1 = rng.next(), h2 = rng.next();
    if (i < 64) h1 = i & 1 ? ~0ull << (i / 2) : 1ull << i, h2 = i & 2 ? 0ull : ~0ull >> (i / 2);
    const uint64_t f1 = sk::fmix64_mid(h1), f2 = sk::fmix64_mid(h2);
    if (f1 != fmix64_ref_mid(h1) || f2 != fmix64_ref_mid(h2)) fail("fmix64_mid", h1, h2, 0);
    if (sk::exact_hash(f1, f2) != fmix64_ref(h1) + fmix64_ref(h2)) fail("exact_hash", f1, f2, 0);
    if (sk::fmix_last(f1 * sk::kFmixC2) != fmix64_ref(h1)) fail("fmix_last", f1, f2, 0);
    ++cases;
  }

  // 2, 3. random (f1, f2, tau): tau uniform, and tau at, just below and at
  // every distance above a random hash
  for (int i = 0; i < 1000000; ++i) {
    const uint64_t f1 = rng.next(), f2 = rng.next();
    check(f1, f2, rng.next());
    const uint64_t h = sk::exact_hash(f1, f2);
    check(f1, f2, h);                                  // h == tau
    check(f1, f2, h - 1);                              // just above tau (h = 0: tau = 2^64 - 1)
    check(f1, f2, h + (rng.next() >> (i & 63)));       // at or above h by every magnitude, may wrap
  }

  // constructed: P on and around tau's high word, every carry of the low words
  const uint32_t tau_his[] = {0u, 1u, 1u << 21, 0x7FFFFFFFu, 0xFFFFFFFCu, 0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu};
  const int kLows = 4 + 12;  // four fixed low words and twelve random ones
  for (uint32_t th : tau_his) {
    for (int dh = -2; dh <= 3; ++dh) {
      for (int li = 0; li < kLows; ++li) {
        for (int rep = 0; rep < 200; ++rep) {
          const uint32_t fixed[4] = {0u, 1u, 0xFFFFFFFEu, 0xFFFFFFFFu};
          const uint32_t tl = li < 4 ? fixed[li] : (uint32_t)rng.next();
          const uint64_t target = ((uint64_t)(th + (uint32_t)dh) << 32) | tl;
          const uint64_t f1 = rng.next();
          const uint64_t f2 = (target - f1 * sk::kFmixC2) * c2inv;
          if ((f1 + f2) * sk::kFmixC2 != target) fail("construction", f1, f2, target);
          const uint64_t h = sk::exact_hash(f1, f2);
          const uint32_t hl = (uint32_t)h;
          const uint32_t tau_los[] = {0u, 0xFFFFFFFFu, hl, hl - 1u, hl + 1u, (uint32_t)rng.next()};
          for (uint32_t lo : tau_los) check(f1, f2, ((uint64_t)th << 32) | lo);
          // tau at the hash itself and next to it, whatever its high word
          check(f1, f2, h);
          check(f1, f2, h - 1);
          check(f1, f2, h + 1);
        }
      }
    }
  }

  // constructed on the hash: h = tau, tau - 1, tau + 1 exactly, and on either
  // side of a high-word carry.  L(p) = p ^ (p >> 33) is a bijection (its
  // inverse is itself: the shift is > 32), so p2 = L(h - L(p1)) gives h.
  for (uint32_t th : tau_his) {
    for (int rep = 0; rep < 3000; ++rep) {
      const uint32_t los[] = {0u, 1u, 0xFFFFFFFEu, 0xFFFFFFFFu, (uint32_t)rng.next()};
      for (uint32_t lo : los) {
        const uint64_t tau = ((uint64_t)th << 32) | lo;
        for (int dt = -1; dt <= 1; ++dt) {
          const uint64_t want = tau + (uint64_t)(int64_t)dt;
          const uint64_t f1 = rng.next();
          const uint64_t rest = want - sk::fmix_last(f1 * sk::kFmixC2);
          const uint64_t f2 = sk::fmix_last(rest) * c2inv;
          if (sk::exact_hash(f1, f2) != want) fail("construction of h", f1, f2, tau);
          check(f1, f2, tau);
        }
      }
    }
  }

  for (int d = 0; d < 3; ++d)
    if (seen[d] == 0) {
      std::printf("FAIL difference %d never seen\n", d - 1);
      ++fails;
    }

  // for information: how many k-mers pass the prefilter at hi(tau) = 2^21
  // without being <= tau, among the constructed cases above and among random
  // k-mers (the window is hi(tau) + 3 values of hi(P) wide where h <= tau
  // takes hi(tau) + 1/2 values of hi(h): ~2.5 in 2^21 of those that pass)
  std::printf("info hi(tau)=2^21: %lld of %lld constructed cases pass the prefilter, %lld of them false positives\n",
              built_pass, built_cases, built_fp);
  {
    const uint64_t tau = ((uint64_t)(1u << 21) << 32) | 0x80000000ull;
    long long pass = 0, fp = 0;
    const long long n = 20000000;
    for (long long i = 0; i < n; ++i) {
      const uint64_t f1 = rng.next(), f2 = rng.next();
      if (sk::prefilter_word(f1, f2) <= sk::prefilter_threshold(tau)) {
        ++pass;
        if (sk::exact_hash(f1, f2) > tau) ++fp;
      }
    }
    std::printf("info hi(tau)=2^21: %lld of %lld random k-mers pass the prefilter, %lld of them false positives\n", pass,
                n, fp);
  }

  if (fails) {
    std::printf("FAILED %lld of %lld\n", fails, cases);
    return 1;
  }
  std::printf("ok %lld cases; hi(h) - hi(P) = -1: %lld, 0: %lld, +1: %lld\n", cases, seen[0], seen[1], seen[2]);
  return 0;
}
