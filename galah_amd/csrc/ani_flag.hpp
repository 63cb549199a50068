// The device side of the flagged list of ani_core.hpp, shared by the kernels
// that compute an f32 ANI (ani_f32.hip over a pair list, ani_matrix.hip over
// the cells of a matrix): the device log, the list entry and the wave's
// append.  The host side (read the counter back, one re-run at the exact
// count, recompute with the host's log, patch) is ani_flagged_passes of
// ani_f32.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gg {

struct DeviceLog {
  __device__ double operator()(double x) const { return ::log(x); }
};

struct AniFlagged {
  uint32_t index, common, total;
};
static_assert(sizeof(AniFlagged) == 12, "the flagged list is 12 bytes an entry");

// Appends the wave's flagged lanes: one ballot and one atomicAdd per wave.
// The whole wave must reach the call.  Entries past the list's capacity are
// dropped and the counter says so.
__device__ __forceinline__ void ani_flag_push(bool flagged, uint32_t index, uint32_t common, uint32_t total,
                                              AniFlagged* __restrict__ list, uint64_t cap,
                                              unsigned long long* __restrict__ count) {
  const uint32_t lane = threadIdx.x & 63;
  const unsigned long long m = __ballot(flagged);
  if (m == 0) return;
  const int leader = __ffsll((long long)m) - 1;
  unsigned long long at = 0;
  if ((int)lane == leader) at = atomicAdd(count, (unsigned long long)__popcll(m));
  at = __shfl(at, leader);
  if (flagged) {
    const unsigned long long slot = at + __popcll(m & ((1ull << lane) - 1));
    if (slot < cap) list[slot] = AniFlagged{index, common, total};
  }
}

}  // namespace gg
