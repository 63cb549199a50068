// The kernels of the resident collection (include/galahgpu.h
// "a collection resident on the device"), by the rules of collection_core.hpp.
//
//   co_row_bounds_kernel   the [n + 1] row boundaries of two (i, j)-sorted lists
//                          in one launch (a binary search per boundary);
//   co_merge_kernel        old list + sorted border -> the merged list, pair and
//                          ANI, each item to its closed-form position: reads
//                          coalesced, writes in runs (a row's old pairs, then
//                          its border pairs);
//   co_pair_flags_kernel   1 where both ends of a pair survive a removal;
//   co_pair_compact_kernel the survivors renumbered to the positions of the
//                          (hipcub) exclusive scan of the flags;
//   co_rows_gather_kernel  the kept rows of one batch of source rows into the
//                          bounce buffer (rows and lens), a workgroup per row;
//   co_pos_kernel, co_relabel_kernel   pos[order[x]] = x, then {pos[i], pos[j]}.
//
// Bandwidth kernels: 256 threads, a grid-stride loop over at most 2,048
// workgroups, a pair moved as one 16-byte access where the buffer is the
// collection's own (hipMalloc: 256-byte aligned); the sorted border lies in
// context scratch at an 8-byte boundary and is read as the struct.  No
// workgroup waits for another, nothing is launched cooperatively, every store
// is a plain vector store.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "collection_core.hpp"
#include "gg_internal.hpp"

namespace gg {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxGrid = 2048;

static_assert(sizeof(gg_pair) == sizeof(uint4), "a pair is one 16-byte access");

inline uint32_t grid_for(uint64_t items) {
  const uint64_t g = (items + kThreads - 1) / kThreads;
  return (uint32_t)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g);
}

__device__ inline gg_pair load_pair16(const gg_pair* p) {  // p 16-byte aligned
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  return gg_pair{v.x, v.y, v.z, v.w};
}
__device__ inline void store_pair16(gg_pair* p, uint32_t i, uint32_t j, uint32_t common, uint32_t total) {
  *reinterpret_cast<uint4*>(p) = make_uint4(i, j, common, total);
}

__global__ __launch_bounds__(kThreads) void co_row_bounds_kernel(const gg_pair* a, uint32_t na, uint32_t* a_start,
                                                                 const gg_pair* b, uint32_t nb, uint32_t* b_start,
                                                                 uint32_t n) {
  const uint64_t total = 2ull * ((uint64_t)n + 1);
  for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (uint64_t)gridDim.x * kThreads) {
    const bool second = t > n;
    const uint32_t r = (uint32_t)(second ? t - n - 1 : t);
    if (second)
      b_start[r] = collection::row_boundary(b, nb, r);
    else
      a_start[r] = collection::row_boundary(a, na, r);
  }
}

__global__ __launch_bounds__(kThreads) void co_merge_kernel(const gg_pair* old_pairs, const float* old_ani, uint32_t n_old,
                                                            const gg_pair* border, const float* border_ani,
                                                            uint32_t n_border, const uint32_t* old_start,
                                                            const uint32_t* border_start, uint32_t n, gg_pair* out,
                                                            float* out_ani) {
  const uint64_t total = (uint64_t)n_old + n_border;
  for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (uint64_t)gridDim.x * kThreads) {
    gg_pair v;
    float a;
    uint32_t at = ~0u;
    if (t < n_old) {
      v = load_pair16(old_pairs + t);
      a = old_ani[t];
      if (v.i < n) at = collection::merged_old((uint32_t)t, v.i, border_start);
    } else {
      const uint32_t q = (uint32_t)(t - n_old);
      v = border[q];
      a = border_ani[q];
      if (v.i < n) at = collection::merged_border(q, v.i, old_start);
    }
    if (at < total) {  // (always, for lists that keep the contract: i < n, both sorted)
      store_pair16(out + at, v.i, v.j, v.common, v.total);
      out_ani[at] = a;
    }
  }
}

__global__ __launch_bounds__(kThreads) void co_pair_flags_kernel(const gg_pair* pairs, uint32_t cnt, uint32_t n,
                                                                 const uint32_t* new_index, uint32_t* flags) {
  // flags[cnt] = 0: the scan's last entry is the number of survivors
  for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t <= cnt; t += (uint64_t)gridDim.x * kThreads) {
    uint32_t f = 0;
    if (t < cnt) {
      const gg_pair v = load_pair16(pairs + t);
      f = v.i < n && v.j < n && collection::pair_survives(new_index, v.i, v.j);
    }
    flags[t] = f;
  }
}

__global__ __launch_bounds__(kThreads) void co_pair_compact_kernel(const gg_pair* pairs, const float* ani, uint32_t cnt,
                                                                   const uint32_t* new_index, const uint32_t* flags,
                                                                   const uint32_t* at, uint32_t out_cap, gg_pair* out,
                                                                   float* out_ani) {
  for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < cnt; t += (uint64_t)gridDim.x * kThreads) {
    if (!flags[t]) continue;
    const uint32_t d = at[t];
    if (d >= out_cap) continue;  // (never: out holds the scan's total)
    const gg_pair v = load_pair16(pairs + t);
    store_pair16(out + d, new_index[v.i], new_index[v.j], v.common, v.total);
    out_ani[d] = ani[t];
  }
}

// one workgroup per source row (grid-stride over the batch's rows)
__global__ __launch_bounds__(kThreads) void co_rows_gather_kernel(const uint64_t* sk, const uint32_t* lens, uint32_t s,
                                                                  uint32_t src0, uint32_t src1, uint32_t dst0,
                                                                  uint32_t bounce_rows, const uint32_t* new_index,
                                                                  uint64_t* bounce, uint32_t* bounce_lens) {
  for (uint32_t r = src0 + blockIdx.x; r < src1; r += gridDim.x) {
    const uint32_t d = new_index[r];
    if (d == collection::kNone) continue;
    const uint32_t slot = d - dst0;
    if (slot >= bounce_rows) continue;  // (never: a batch keeps at most its own rows)
    const uint64_t* from = sk + (size_t)r * s;
    uint64_t* to = bounce + (size_t)slot * s;
    for (uint32_t x = threadIdx.x; x < s; x += kThreads) to[x] = from[x];
    if (threadIdx.x == 0) bounce_lens[slot] = lens[r];
  }
}

__global__ __launch_bounds__(kThreads) void co_pos_kernel(const uint32_t* order, uint32_t n, uint32_t* pos) {
  for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += (uint64_t)gridDim.x * kThreads) {
    const uint32_t g = order[t];
    if (g < n) pos[g] = (uint32_t)t;  // (a permutation: checked on the host)
  }
}

__global__ __launch_bounds__(kThreads) void co_relabel_kernel(const gg_pair* pairs, uint32_t cnt, uint32_t n,
                                                              const uint32_t* pos, gg_pair* out) {
  for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < cnt; t += (uint64_t)gridDim.x * kThreads) {
    const gg_pair v = load_pair16(pairs + t);
    const uint32_t i = v.i < n ? pos[v.i] : v.i, j = v.j < n ? pos[v.j] : v.j;
    store_pair16(out + t, i, j, v.common, v.total);
  }
}

}  // namespace

hipError_t launch_collection_row_bounds(const gg_pair* a, uint32_t na, uint32_t* a_start, const gg_pair* b, uint32_t nb,
                                        uint32_t* b_start, uint32_t n, hipStream_t st) {
  hipLaunchKernelGGL(co_row_bounds_kernel, dim3(grid_for(2ull * ((uint64_t)n + 1))), dim3(kThreads), 0, st, a, na, a_start,
                     b, nb, b_start, n);
  return hipGetLastError();
}

hipError_t launch_collection_merge(const gg_pair* old_pairs, const float* old_ani, uint32_t n_old, const gg_pair* border,
                                   const float* border_ani, uint32_t n_border, const uint32_t* old_start,
                                   const uint32_t* border_start, uint32_t n, gg_pair* out, float* out_ani,
                                   hipStream_t st) {
  if ((uint64_t)n_old + n_border == 0) return hipSuccess;
  hipLaunchKernelGGL(co_merge_kernel, dim3(grid_for((uint64_t)n_old + n_border)), dim3(kThreads), 0, st, old_pairs, old_ani,
                     n_old, border, border_ani, n_border, old_start, border_start, n, out, out_ani);
  return hipGetLastError();
}

size_t collection_scan_tmp_bytes(uint32_t cnt) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(cnt + 1));
  return bytes;
}

hipError_t launch_collection_pair_scan(const gg_pair* pairs, uint32_t cnt, uint32_t n, const uint32_t* new_index,
                                       uint32_t* flags, uint32_t* at, void* tmp, size_t tmp_bytes, hipStream_t st) {
  hipLaunchKernelGGL(co_pair_flags_kernel, dim3(grid_for((uint64_t)cnt + 1)), dim3(kThreads), 0, st, pairs, cnt, n,
                     new_index, flags);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, flags, at, (int)(cnt + 1), st);
}

hipError_t launch_collection_pair_compact(const gg_pair* pairs, const float* ani, uint32_t cnt, const uint32_t* new_index,
                                          const uint32_t* flags, const uint32_t* at, uint32_t out_cap, gg_pair* out,
                                          float* out_ani, hipStream_t st) {
  if (cnt == 0) return hipSuccess;
  hipLaunchKernelGGL(co_pair_compact_kernel, dim3(grid_for(cnt)), dim3(kThreads), 0, st, pairs, ani, cnt, new_index, flags,
                     at, out_cap, out, out_ani);
  return hipGetLastError();
}

hipError_t launch_collection_rows_gather(const uint64_t* sk, const uint32_t* lens, uint32_t s, uint32_t src0, uint32_t src1,
                                         uint32_t dst0, uint32_t bounce_rows, const uint32_t* new_index, uint64_t* bounce,
                                         uint32_t* bounce_lens, hipStream_t st) {
  if (src1 <= src0) return hipSuccess;
  hipLaunchKernelGGL(co_rows_gather_kernel, dim3(std::min<uint32_t>(src1 - src0, 8 * kMaxGrid)), dim3(kThreads), 0, st, sk,
                     lens, s, src0, src1, dst0, bounce_rows, new_index, bounce, bounce_lens);
  return hipGetLastError();
}

hipError_t launch_collection_relabel(const uint32_t* order, uint32_t n, uint32_t* pos, const gg_pair* pairs, uint32_t cnt,
                                     gg_pair* out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(co_pos_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, order, n, pos);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || cnt == 0) return e;
  hipLaunchKernelGGL(co_relabel_kernel, dim3(grid_for(cnt)), dim3(kThreads), 0, st, pairs, cnt, n, pos, out);
  return hipGetLastError();
}

}  // namespace gg
