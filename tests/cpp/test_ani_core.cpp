// The f32 ANI rule of the device (galah_amd/csrc/ani_core.hpp) on the host,
// without a device.  Grid: total 1 .. 2000, common 0 .. min(total, 1000), plus
// total = 0, plus a few common > total, for k = 2, 5, 21, 32.
//   (a) the core with std::log equals the library's ani_f64 expression,
//       restated here, bit for bit in f64 and in f32, on every entry;
//   (b) with the log moved by +-1, +-4, +-16 and +-64 ulp every entry is
//       either flagged or has the unperturbed f32 (what the kernel relies on:
//       an unflagged f32 is final whatever the device's log does within that);
//   (c) at E = 2^-44 at most 1e-4 of the grid is flagged (the recheck stays
//       cheap);
//   (d) the entries decided by the integers (total == 0, common == 0,
//       common >= total) are never flagged, at any margin and any log;
//   and at E = 1 (GALAHGPU_TEST_ANI_MARGIN_LOG2=0) every other entry is,
//   but for a distance above 2.
// Prints "ok <entries>" and the flagged counts per k.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../galah_amd/csrc/ani_core.hpp"

namespace ani = gg::ani;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

// ---- the library's host expression (api.cpp ani_f64), restated
static double rmin(double a, double b) {
  if (std::isnan(a)) return b;
  if (std::isnan(b)) return a;
  return a < b ? a : b;
}
static double rmax(double a, double b) {
  if (std::isnan(a)) return b;
  if (std::isnan(b)) return a;
  return a > b ? a : b;
}
static double literal_f64(uint32_t common, uint32_t total, int k) {
  const double jaccard = (double)common / (double)total;
  double d = -1.0 * std::log((2.0 * jaccard) / (1.0 + jaccard)) / (double)k;
  d = rmax(rmin(d, 1.0), 0.0);
  return 1.0 - d;
}

static uint64_t bits64(double x) {
  uint64_t b;
  memcpy(&b, &x, sizeof b);
  return b;
}
static uint32_t bits32(float x) {
  uint32_t b;
  memcpy(&b, &x, sizeof b);
  return b;
}

// std::log moved by `ulp` units in the last place (towards +inf when positive)
struct ShiftedLog {
  int ulp;
  double operator()(double x) const {
    const double y = std::log(x);
    if (y == 0.0 || !std::isfinite(y)) return y;
    int64_t b;
    memcpy(&b, &y, sizeof b);
    b += y > 0.0 ? ulp : -ulp;  // (sign-magnitude: a negative value grows by a smaller magnitude)
    double z;
    memcpy(&z, &b, sizeof z);
    return z;
  }
};

struct Entry {
  uint32_t common, total;
};

int main() {
  std::vector<Entry> grid;
  for (uint32_t t = 1; t <= 2000; ++t)
    for (uint32_t c = 0; c <= (t < 1000 ? t : 1000); ++c) grid.push_back(Entry{c, t});
  for (uint32_t c : {0u, 1u, 7u, 1000u}) grid.push_back(Entry{c, 0});
  for (Entry e : {Entry{2, 1}, Entry{11, 10}, Entry{1000, 999}, Entry{1000, 1}, Entry{4000000000u, 3u}}) grid.push_back(e);
  const double E = ani::pow2(ani::kMarginLog2);
  CHECK(E == std::ldexp(1.0, -44) && ani::pow2(0) == 1.0 && ani::pow2(-1000) == std::ldexp(1.0, -1000));
  const int ks[4] = {2, 5, 21, 32};
  const int ulps[8] = {1, -1, 4, -4, 16, -16, 64, -64};
  uint64_t flagged_k[4] = {0, 0, 0, 0};
  double worst_dv = 0.0;
  for (int ki = 0; ki < 4; ++ki) {
    const int k = ks[ki];
    for (const Entry& e : grid) {
      const bool by_integers = e.total == 0 || e.common == 0 || e.common >= e.total;
      // (a)
      const ani::Value r = ani::value(e.common, e.total, k, E, ani::HostLog{});
      const double lit = literal_f64(e.common, e.total, k);
      CHECK(bits64(r.v) == bits64(lit));
      CHECK(bits32(r.f) == bits32((float)lit));
      flagged_k[ki] += r.flagged;
      // (d)
      if (by_integers) {
        CHECK(!r.flagged);
        CHECK(!ani::value(e.common, e.total, k, 1.0, ani::HostLog{}).flagged);
      } else {
        // (a distance above 1 + E = 2 is 0 with any log: k = 2 has some)
        const double jaccard = (double)e.common / (double)e.total;
        const double d = -1.0 * std::log((2.0 * jaccard) / (1.0 + jaccard)) / (double)k;
        const ani::Value w = ani::value(e.common, e.total, k, 1.0, ani::HostLog{});
        if (d > 2.0) CHECK(!w.flagged && w.f == 0.0f);
        else CHECK(w.flagged);
      }
      // (b)
      for (int u : ulps) {
        const ani::Value s = ani::value(e.common, e.total, k, E, ShiftedLog{u});
        if (by_integers) CHECK(!s.flagged && bits32(s.f) == bits32(r.f) && bits64(s.v) == bits64(r.v));
        CHECK(s.flagged || bits32(s.f) == bits32(r.f));
        const double dv = std::fabs(s.v - r.v);
        if (dv > worst_dv) worst_dv = dv;
      }
    }
    // (c)
    CHECK((double)flagged_k[ki] <= 1e-4 * (double)grid.size());
  }
  // a log 64 ulp off stays well inside the margin
  CHECK(worst_dv < E);
  printf("ok %zu\n", grid.size());
  printf("flagged k=2:%llu k=5:%llu k=21:%llu k=32:%llu  largest |dv| at 64 ulp %.3g (E %.3g)\n",
         (unsigned long long)flagged_k[0], (unsigned long long)flagged_k[1], (unsigned long long)flagged_k[2],
         (unsigned long long)flagged_k[3], worst_dv, E);
  return 0;
}
