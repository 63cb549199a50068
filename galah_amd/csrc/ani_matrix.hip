// The dense ANI matrix of a set of rows: for m listed rows
// of a sketch matrix, common / total / f32 ANI of every two of them, [m x m],
// by the rules of matrix_core.hpp.  common is a contraction: with the 0/1
// incidence matrix A [positions x columns], common = A A^T, on the i8 matrix
// instruction.
//
// The positions part -- matrix_prepare, the one of all four forms (DESIGN.md
// 4.14); a MatrixForm selects the three places in which the forms differ:
//
//   mx_offsets_kernel  one workgroup: every position's row, length and the
//                      exclusive sum of the lengths (the dense form, and the
//                      pair and border forms up to kMaxRows rows); else
//   mx_positions_kernel<groups> and hipcub ExclusiveSum: the same for any
//                      number of positions, with every position's group.
//                      [border: mxb_rows_kernel before it, the new rows first;
//                       groups: mxg_segments_kernel, every group's first entry]
//   mx_keys_kernel     (hash, slot = position * s + e) of every entry, the
//                      valid ones packed to the front, the others (key ~0)
//                      behind them, so the sort's count needs no read-back.
//   hipcub SortPairs   on the 64-bit key (stable: the padding stays behind).
//                      [two groups or more: mxg_entry_groups_kernel, a stable
//                       SortPairs on the group's bits, mxg_gather_kernel -- the
//                       entries by (group, hash); one group: a memset]
//                      [border: mxb_starts_kernel and an inclusive max, every
//                       entry's first entry of its run of equal hashes]
//   mx_flags_kernel<Rule>  the column rule on the sorted keys, both flags
//                      packed: PlainRule, BorderRule (the runs whose first entry
//                      lies at a new position) or GroupRule (within a group);
//   hipcub InclusiveSum  column ids and, at the end, the two counts.
//   mx_ids_kernel<Rule>  the id (or none) of every entry, scattered to its
//                      slot (GroupRule: local to the group).
//   mx_pieces_kernel   one workgroup per position: its kept ids compacted in
//                      order into a contiguous piece with a count.
//   [read back: entries, columns, column entries, and a border's new entries
//    -- the one sync before the product]
//   mx_common_kernel   the product and the epilogue, below.
//
// Flags and ids live in whichever of the two sort buffers the sorted keys and
// slots are not in; a border's run starts in the value buffer the ids go to
// later and in the piece buffer.
//
// mx_common_kernel: one workgroup (4 waves) per tile pair ti <= tj of 64 x 64
// positions, K over the columns in chunks of 512.  Per chunk: one thread per
// row finds the row's cursor (a binary search of its piece from the last
// cursor) and its next id, a wave minimum per tile gives the chunk to run --
// chunks in which either tile holds nothing are jumped over; the workgroup
// clears the two [64 x 512] byte images (one for a diagonal tile), every wave
// takes rows in turn and its 64 lanes scatter the row's entries of the chunk
// (64 ids per step from the cursor); after the barrier wave w reads the A
// fragments of rows 16 w .. 16 w + 15 and the B fragments of the four 16-row
// blocks of the other tile and issues mfma_i32_16x16x64_i8, 8 k-steps x 4
// blocks, into four i32x4 accumulators that live across the chunks.
// Epilogue per element: total by the rank rule from the two rows in global
// memory, the ANI by ani::value with the device log, stores at (a, b) and
// (b, a); a diagonal tile writes a <= b only.  LDS: 2 x 33,792 B images +
// 3,080 B of row state = 70,664 B, two workgroups per CU.
//
// No workgroup waits for another, the kernels are not persistent, and the
// only atomic is the flagged list's counter (ani_flag.hpp).  The kernels are
// launched plainly (no gg_timing_read slot).
//
// The matrices of many groups in one call are further down:
// the same product kernel instantiated on MxGroupLaunch, fed by entries sorted
// by (group, hash) with column ids local to a group.
//
// The pair form is the third instantiation, on MxPairLaunch:
// the same prologue, chunk loop and accumulators, and instead of the dense
// epilogue the thresholded one of matrix_core.hpp -- a tile pair that ran no
// chunk returns at once (unless pairs without a shared hash pass), a cell pays
// the rank search only when its common can pass, and the passing pairs are
// staged in the image area (free after the loop's last barrier), counted with
// one LDS add per wave and step, and appended to the output with one global
// add per workgroup and 16-byte stores.
//
// The border form is the fourth instantiation, on
// MxBorderLaunch: the pair form over rows of which the last n_new are new,
// with the new rows at the first positions (mxb_rows_kernel writes the map as
// a row list), the tile pairs that hold a new tile only, the cells of a new
// position only, and the border column rule in the positions part.
//
// Around the kernel the forms share launch_of (the fields of every launch),
// dense_product (the dense and the grouped tail) and launch_pair_slices (the
// pair and the border launches).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ani_core.hpp"
#include "ani_flag.hpp"
#include "context.hpp"
#include "device_util.hpp"
#include "gg_internal.hpp"
#include "matrix_core.hpp"

namespace gg {
namespace {

using matrix::kChunk;
using matrix::kNoColumn;
using matrix::kRowBytes;
using matrix::kTile;
using matrix::kTileBytes;

constexpr uint32_t kNoRow = 0xFFFFFFFFu;  // a position whose row index is out of range: the one empty row
constexpr uint32_t kOffBlock = 1024;
constexpr uint32_t kOffPer = matrix::kMaxRows / kOffBlock;  // positions per thread of mx_offsets_kernel

typedef int i32x4 __attribute__((ext_vector_type(4)));

inline dim3 grid_for(uint64_t items) { return dim3((uint32_t)std::min<uint64_t>(16384, (items + 255) / 256)); }

// GALAHGPU_TEST_PAIRS_SLICE, read per call: fewer tile pairs per launch of the pair form (tests of the slices at small m)
uint32_t test_pair_slice() {
  const char* e = getenv("GALAHGPU_TEST_PAIRS_SLICE");
  if (!e || !*e) return matrix::kPairSlice;
  return (uint32_t)std::min<uint64_t>(matrix::kPairSlice, std::max<uint64_t>(1, strtoull(e, nullptr, 10)));
}

// pos_row[a] (kNoRow: an index >= n, an empty row), pos_len[a], pos_off[0 .. m] the exclusive sum of the lengths
__global__ __launch_bounds__(kOffBlock) void mx_offsets_kernel(const uint32_t* __restrict__ lens, uint32_t n, uint32_t s,
                                                               const uint32_t* __restrict__ rows, uint32_t m,
                                                               uint32_t* __restrict__ pos_row,
                                                               uint32_t* __restrict__ pos_len,
                                                               uint32_t* __restrict__ pos_off) {
  __shared__ uint32_t part[kOffBlock];
  const uint32_t t = threadIdx.x, a0 = t * kOffPer;
  uint32_t sum = 0;
  for (uint32_t a = a0; a < min(a0 + kOffPer, m); ++a) {
    const uint32_t g = rows ? rows[a] : a;
    const bool ok = g < n;
    const uint32_t len = ok ? min(lens[g], s) : 0u;
    pos_row[a] = ok ? g : kNoRow;
    pos_len[a] = len;
    sum += len;
  }
  part[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < kOffBlock; d <<= 1) {  // inclusive sum of the partial sums
    const uint32_t v = t >= d ? part[t - d] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t off = part[t] - sum;
  for (uint32_t a = a0; a < min(a0 + kOffPer, m); ++a) {
    pos_off[a] = off;
    off += pos_len[a];
  }
  if (t == kOffBlock - 1) pos_off[m] = part[t];
}

// the same rows and lengths for any number of positions (the pair and border
// forms beyond kMaxRows, the grouped form always): len1[0 .. m] the lengths and
// a 0 behind them (the scan's last item: its exclusive sum is the number of
// entries), for the scan that gives pos_off.  kGroups: len1 is pos_len itself,
// of m + 1 words, and pos_grp[a] the position's group (a search of offsets)
template <bool kGroups>
__global__ __launch_bounds__(256) void mx_positions_kernel(const uint32_t* __restrict__ lens, uint32_t n, uint32_t s,
                                                           const uint32_t* __restrict__ rows, uint32_t m,
                                                           uint32_t* __restrict__ pos_row, uint32_t* __restrict__ pos_len,
                                                           uint32_t* __restrict__ len1,
                                                           const uint32_t* __restrict__ offsets, uint32_t n_groups,
                                                           uint32_t* __restrict__ pos_grp) {
  for (uint32_t a = blockIdx.x * 256 + threadIdx.x; a <= m; a += gridDim.x * 256) {
    if (a == m) {
      len1[a] = 0;
      continue;
    }
    const uint32_t g = rows ? rows[a] : a;
    const bool ok = g < n;
    const uint32_t len = ok ? min(lens[g], s) : 0u;
    pos_row[a] = ok ? g : kNoRow;
    pos_len[a] = len;
    if constexpr (kGroups) pos_grp[a] = matrix::group_of_position(offsets, n_groups, a);
    else len1[a] = len;
  }
}

__global__ __launch_bounds__(256) void mx_keys_kernel(const uint64_t* __restrict__ sk, uint32_t s, uint32_t m,
                                                      const uint32_t* __restrict__ pos_row,
                                                      const uint32_t* __restrict__ pos_len,
                                                      const uint32_t* __restrict__ pos_off,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t N = m * s, ne = pos_off[m];
  for (uint32_t slot = blockIdx.x * 256 + threadIdx.x; slot < N; slot += gridDim.x * 256) {
    const uint32_t a = slot / s, e = slot - a * s;
    const uint32_t len = pos_len[a], off = pos_off[a];
    if (e < len) {
      keys[off + e] = sk[(uint64_t)pos_row[a] * s + e];
      vals[off + e] = slot;
    } else {
      const uint32_t at = ne + (a * s - off) + (e - len);  // the slots without an entry, in slot order
      keys[at] = ~0ull;
      vals[at] = kNoColumn;
    }
  }
}

// ---- the column rules (matrix_core.hpp) ------------------------------------------
// A rule gives, for the sorted entry i < ne, flags(K, i, ne) -- both flags of
// the column rule packed, for the sum -- and id(K, sums, i, ne), the entry's
// column id or kNoColumn.
struct PlainRule {
  __device__ uint64_t flags(const uint64_t* K, uint32_t i, uint32_t ne) const { return matrix::column_flags(K, i, ne); }
  __device__ uint32_t id(const uint64_t* K, const uint64_t* sums, uint32_t i, uint32_t ne) const {
    return matrix::in_column(K, i, ne) ? matrix::column_id(sums[i]) : kNoColumn;
  }
};
// the border form: the run of entry i is a border column's when its first
// entry (the lowest slot of the run) lies at a new position (start1[i] >= 1:
// entry 0 opens a run)
struct BorderRule {
  const uint32_t* slot_of;
  const uint32_t* start1;
  uint32_t s, n_new;
  __device__ bool kept(uint32_t i) const { return matrix::border_column_kept(slot_of[start1[i] - 1] / s, n_new); }
  __device__ uint64_t flags(const uint64_t* K, uint32_t i, uint32_t ne) const {
    return kept(i) ? matrix::column_flags(K, i, ne) : 0ull;
  }
  __device__ uint32_t id(const uint64_t* K, const uint64_t* sums, uint32_t i, uint32_t ne) const {
    return matrix::in_column(K, i, ne) && kept(i) ? matrix::column_id(sums[i]) : kNoColumn;
  }
};
// the grouped form: entries sorted by (group, hash), ids local to the group (seg[g] the group's first entry)
struct GroupRule {
  const uint32_t* grp;
  const uint32_t* seg;
  __device__ uint64_t flags(const uint64_t* K, uint32_t i, uint32_t ne) const { return matrix::column_flags(K, grp, i, ne); }
  __device__ uint32_t id(const uint64_t* K, const uint64_t* sums, uint32_t i, uint32_t ne) const {
    return matrix::in_column(K, grp, i, ne) ? matrix::column_id(sums[i]) - matrix::group_first_id(sums, seg[grp[i]])
                                            : kNoColumn;
  }
};

template <class Rule>
__global__ __launch_bounds__(256) void mx_flags_kernel(const uint64_t* __restrict__ K, uint32_t N,
                                                       const uint32_t* __restrict__ pos_off, uint32_t m, Rule rule,
                                                       uint64_t* __restrict__ flags) {
  const uint32_t ne = pos_off[m];
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256)
    flags[i] = i < ne ? rule.flags(K, i, ne) : 0ull;
}

template <class Rule>
__global__ __launch_bounds__(256) void mx_ids_kernel(const uint64_t* __restrict__ K, const uint32_t* __restrict__ slot_of,
                                                     const uint64_t* __restrict__ sums,
                                                     const uint32_t* __restrict__ pos_off, uint32_t m, Rule rule,
                                                     uint32_t* __restrict__ id_of) {
  const uint32_t ne = pos_off[m];
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < ne; i += gridDim.x * 256) id_of[slot_of[i]] = rule.id(K, sums, i, ne);
}

// ---- the border form's own kernels (matrix_core.hpp, the border form) ------------
// the border's positions as a row list: the new rows first
__global__ __launch_bounds__(256) void mxb_rows_kernel(uint32_t n, uint32_t n_old, uint32_t* __restrict__ rows) {
  for (uint32_t a = blockIdx.x * 256 + threadIdx.x; a < n; a += gridDim.x * 256)
    rows[a] = matrix::border_row_of(a, n, n_old);
}

// start1[i] = i + 1 at the first entry of a run of equal hashes, else 0: the
// inclusive max over it gives every entry its run's first entry (plus one)
__global__ __launch_bounds__(256) void mxb_starts_kernel(const uint64_t* __restrict__ K, uint32_t N,
                                                         const uint32_t* __restrict__ pos_off, uint32_t m,
                                                         uint32_t* __restrict__ start1) {
  const uint32_t ne = pos_off[m];
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256)
    start1[i] = i < ne && (i == 0 || K[i] != K[i - 1]) ? i + 1 : 0u;
}

// ---- the grouped form's own kernels (matrix_core.hpp, groups) ---------------------
// seg[g] the first sorted entry of group g, seg[n_groups] the number of entries
__global__ __launch_bounds__(256) void mxg_segments_kernel(const uint32_t* __restrict__ offsets, uint32_t n_groups,
                                                           const uint32_t* __restrict__ pos_off,
                                                           uint32_t* __restrict__ seg) {
  for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g <= n_groups; g += gridDim.x * 256) seg[g] = pos_off[offsets[g]];
}

// the group of every hash-sorted entry from its slot (the padding: n_groups, behind every group)
__global__ __launch_bounds__(256) void mxg_entry_groups_kernel(const uint32_t* __restrict__ slot_of, uint32_t N,
                                                               uint32_t s, const uint32_t* __restrict__ pos_grp,
                                                               uint32_t n_groups, uint32_t* __restrict__ grp) {
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
    const uint32_t slot = slot_of[i];
    grp[i] = slot == kNoColumn ? n_groups : pos_grp[slot / s];
  }
}

// the hash of every entry from its slot, after the stable sort on the group
__global__ __launch_bounds__(256) void mxg_gather_kernel(const uint64_t* __restrict__ sk, uint32_t s,
                                                         const uint32_t* __restrict__ pos_row,
                                                         const uint32_t* __restrict__ slot_of,
                                                         const uint32_t* __restrict__ pos_off, uint32_t P,
                                                         uint64_t* __restrict__ K) {
  const uint32_t ne = pos_off[P];
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < ne; i += gridDim.x * 256) {
    const uint32_t slot = slot_of[i], p = slot / s;
    K[i] = sk[(uint64_t)pos_row[p] * s + (slot - p * s)];
  }
}

// a group of one position: its cell is the diagonal rule's
__global__ __launch_bounds__(256) void mxg_single_kernel(const uint32_t* __restrict__ offsets,
                                                         const uint64_t* __restrict__ cell_off, uint32_t n_groups,
                                                         const uint32_t* __restrict__ pos_len,
                                                         uint32_t* __restrict__ common, uint32_t* __restrict__ total,
                                                         float* __restrict__ ani) {
  for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < n_groups; g += gridDim.x * 256) {
    const uint32_t p = offsets[g];
    if (offsets[g + 1] - p != 1) continue;
    const uint32_t len = pos_len[p];
    const uint64_t cell = cell_off[g];
    if (common) common[cell] = len;
    if (total) total[cell] = len;
    if (ani) ani[cell] = len ? 1.0f : 0.0f;
  }
}

// piece[a * s ..) the ids of position a's entries that lie in a column, in the row's order; piece_cnt[a]
__global__ __launch_bounds__(256) void mx_pieces_kernel(const uint32_t* __restrict__ id_of,
                                                        const uint32_t* __restrict__ pos_len, uint32_t s,
                                                        uint32_t* __restrict__ piece, uint32_t* __restrict__ piece_cnt) {
  __shared__ uint32_t wave_cnt[4];
  const uint32_t a = blockIdx.x, len = pos_len[a], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t* in = id_of + (uint64_t)a * s;
  uint32_t* out = piece + (uint64_t)a * s;
  uint32_t done = 0;
  for (uint32_t base = 0; base < len; base += 256) {  // (len is the workgroup's: whole waves reach the ballot)
    const uint32_t e = base + threadIdx.x;
    const uint32_t id = e < len ? in[e] : kNoColumn;
    const bool keep = id != kNoColumn;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t at = done;
    for (uint32_t w = 0; w < wave; ++w) at += wave_cnt[w];
    if (keep) out[at + lanes_below(mask)] = id;
    done += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) piece_cnt[a] = done;
}

struct MxLaunch {
  const uint64_t* sk;
  uint32_t s, m;
  const uint32_t* pos_row;
  const uint32_t* pos_len;
  const uint32_t* piece;
  const uint32_t* piece_cnt;
  uint32_t* common;
  uint32_t* total;
  float* ani;
  int k;
  double E;
  AniFlagged* list;
  uint64_t cap;
  unsigned long long* count;
  static constexpr bool kGroups = false;
  static constexpr bool kPairs = false;
  static constexpr bool kBorder = false;
};
// the grouped form (matrix_core.hpp, groups): m is not read, a workgroup finds its group in tp_off
struct MxGroupLaunch : MxLaunch {
  const uint32_t* offsets;   // [n_groups + 1] first position of a group
  const uint32_t* tp_off;    // [n_groups + 1] first workgroup of a group
  const uint64_t* cell_off;  // [n_groups + 1] first cell of a group's block
  uint32_t n_groups;
  static constexpr bool kGroups = true;
};
// the pair form (matrix_core.hpp, the pair form): common / total / ani / list are
// not read, the passing pairs are appended to out and counted in `count`
struct MxPairLaunch : MxLaunch {
  const uint32_t* cmin;    // [tmax + 1]
  const uint32_t* sufmin;  // [tmax + 1]
  uint32_t tmax;
  uint32_t zero_passes;
  gg_pair* out;
  uint64_t out_cap;
  uint32_t wg_base;  // the tile pair of the launch's workgroup 0 (a call is launched in slices)
  static constexpr bool kPairs = true;
};
// the border form (matrix_core.hpp, the border form): m rows at the border's
// positions, the first n_new of them new (tiles_new tiles of them); wg_base
// counts border tile pairs
struct MxBorderLaunch : MxPairLaunch {
  uint32_t n_new;
  uint32_t tiles_new;
  static constexpr bool kBorder = true;
};

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  for (int d = 32; d; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d));
  return v;
}

// L = MxLaunch: the tile pairs of one [m x m] matrix.  L = MxGroupLaunch: the
// tile pairs of every group in turn; positions, bounds and cells are the
// group's (first position p0, m positions, first cell c0), the pieces hold
// group-local ids, and a flagged cell is listed on both sides of the diagonal
// (the list's patch then needs no matrix width).
template <class L>
__global__ __launch_bounds__(256) void mx_common_kernel(L a) {
  __shared__ __align__(16) uint8_t image[2 * kTileBytes];
  __shared__ uint64_t s_last[2 * kTile];
  __shared__ uint32_t s_row[2 * kTile], s_len[2 * kTile], s_cnt[2 * kTile], s_cur[2 * kTile];
  __shared__ uint32_t s_min[2];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t ti, tj, p0 = 0, m = a.m;
  uint64_t c0 = 0;
  if constexpr (L::kGroups) {
    const uint32_t g = matrix::group_of_workgroup(a.tp_off, a.n_groups, blockIdx.x);
    p0 = a.offsets[g];
    m = a.offsets[g + 1] - p0;
    c0 = a.cell_off[g];
    matrix::tile_pair_of(blockIdx.x - a.tp_off[g], &ti, &tj);
  } else if constexpr (L::kBorder) {
    matrix::border_tile_pair_of(a.wg_base + blockIdx.x, a.tiles_new, &ti, &tj);  // (< 2^31: border_limits_ok)
  } else if constexpr (L::kPairs) {
    matrix::tile_pair_of(a.wg_base + blockIdx.x, &ti, &tj);  // (< 2^31: pair_limits_ok)
  } else {
    matrix::tile_pair_of(blockIdx.x, &ti, &tj);
  }
  const bool diag = ti == tj;
  const uint32_t sides = diag ? 1u : 2u;
  // rows 0 .. 63 of the state are tile ti's positions, 64 .. 127 tile tj's (not filled for a diagonal tile)
  if (t < sides * kTile) {
    const uint32_t pos = (t < kTile ? ti : tj) * kTile + (t & (kTile - 1));
    const bool ok = pos < m;
    const uint32_t row = ok ? a.pos_row[p0 + pos] : kNoRow;
    const uint32_t len = ok ? a.pos_len[p0 + pos] : 0u;
    s_row[t] = row;
    s_len[t] = len;
    s_cnt[t] = ok ? a.piece_cnt[p0 + pos] : 0u;
    s_cur[t] = 0;
    s_last[t] = len ? a.sk[(uint64_t)row * a.s + len - 1] : 0ull;
  }
  __syncthreads();

  i32x4 acc[4];
  for (int nb = 0; nb < 4; ++nb) acc[nb] = i32x4{0, 0, 0, 0};
  const uint8_t* img_a = image;
  const uint8_t* img_b = image + (diag ? 0u : kTileBytes);
  uint32_t k0 = 0;  // (every branch on k0, s_min is the workgroup's)
  [[maybe_unused]] bool ran = false;  // (the pair form) a chunk was run
  for (;;) {
    if (t < 2 * kTile) {  // waves 0 and 1: a tile each
      uint32_t next = kNoColumn;
      if (t < sides * kTile) {
        const uint32_t pos = (t < kTile ? ti : tj) * kTile + (t & (kTile - 1));
        const uint32_t cnt = s_cnt[t];
        const uint32_t* pc = a.piece + (uint64_t)(p0 + pos) * a.s;  // (not read when cnt == 0)
        const uint32_t cur = matrix::cursor_at(pc, s_cur[t], cnt, k0);
        s_cur[t] = cur;
        if (cur < cnt) next = pc[cur];
      }
      next = wave_min(next);
      if (lane == 0) s_min[wave] = next;
    }
    __syncthreads();
    const uint32_t kc = matrix::next_chunk(s_min[0], diag ? s_min[0] : s_min[1]);
    if (kc == kNoColumn) break;
    if (kc != k0) {  // a chunk (or more) in which a tile holds nothing: jump, find the cursors there
      k0 = kc;
      __syncthreads();
      continue;
    }
    for (uint32_t i = t; i < sides * kTileBytes / 16; i += 256) reinterpret_cast<uint4*>(image)[i] = uint4{0, 0, 0, 0};
    __syncthreads();
    for (uint32_t r = wave; r < sides * kTile; r += 4) {
      const uint32_t pos = (r < kTile ? ti : tj) * kTile + (r & (kTile - 1));
      const uint32_t cnt = s_cnt[r];
      const uint32_t* pc = a.piece + (uint64_t)(p0 + pos) * a.s;
      uint8_t* img = image + (r < kTile ? 0u : kTileBytes);
      for (uint32_t e = s_cur[r] + lane;; e += 64) {  // (s_cur[r], cnt are the wave's)
        bool in = e < cnt;
        uint32_t col = 0;
        if (in) {
          col = pc[e] - k0;
          in = col < kChunk;
        }
        if (in) img[matrix::image_offset(r & (kTile - 1), col)] = 1;
        if (__ballot(in) != ~0ull) break;
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t ks = 0; ks < matrix::kKSteps; ++ks) {
      const i32x4 af = *reinterpret_cast<const i32x4*>(img_a + matrix::fragment_offset(lane, ks, wave));
#pragma unroll
      for (uint32_t nb = 0; nb < 4; ++nb) {
        const i32x4 bf = *reinterpret_cast<const i32x4*>(img_b + matrix::fragment_offset(lane, ks, nb));
        acc[nb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf, acc[nb], 0, 0, 0);
      }
    }
    k0 += kChunk;
    if constexpr (L::kPairs) ran = true;
    __syncthreads();
  }

  if constexpr (L::kPairs) {
    // The pair epilogue.  The image area is free after the loop's last
    // barrier: the passing pairs of the tile pair (at most kPairStage) are
    // staged there, a wave taking its slots with one LDS add per step; then
    // one add to the global count for the workgroup and 16-byte stores.
    __shared__ uint32_t s_found;
    __shared__ unsigned long long s_base;
    if (matrix::pair_early_exit(ran, a.zero_passes != 0)) return;  // (the workgroup's)
    gg_pair* stage = reinterpret_cast<gg_pair*>(image);
    if (t == 0) s_found = 0;
    __syncthreads();
    const uint32_t sb = diag ? 0u : kTile;  // tile tj's row state
#pragma unroll
    for (uint32_t nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (uint32_t reg = 0; reg < 4; ++reg) {
        const uint32_t ra = wave * 16 + matrix::cd_row(lane, reg), rb = nb * 16 + matrix::cd_col(lane);
        const uint32_t pa = ti * kTile + ra, pb = tj * kTile + rb;
        uint32_t common = 0, total = 0, ga = 0, gb = 0;
        bool pass = false;
        if (pa < m && pb < m) {
          ga = s_row[ra];
          gb = s_row[sb + rb];
          bool visited;
          if constexpr (L::kBorder) visited = matrix::border_visited(pa, pb, a.n_new, ga, gb);
          else visited = matrix::pair_visited(pa, pb, ga, gb);
          if (visited)
            pass = matrix::pair_cell(a.sk + (uint64_t)ga * a.s, s_len[ra], s_last[ra], a.sk + (uint64_t)gb * a.s,
                                     s_len[sb + rb], s_last[sb + rb], (uint32_t)acc[nb][reg], a.cmin, a.sufmin, a.tmax,
                                     &common, &total);
        }
        const unsigned long long mk = __ballot(pass);
        if (mk) {
          const uint32_t first = (uint32_t)__builtin_ctzll(mk);
          uint32_t at = 0;
          if (lane == first) at = atomicAdd(&s_found, (uint32_t)__popcll(mk));
          at = (uint32_t)__shfl((int)at, (int)first);
          if (pass) stage[at + lanes_below(mk)] = gg_pair{min(ga, gb), max(ga, gb), common, total};
        }
      }
    }
    __syncthreads();
    const uint32_t found = s_found;
    if (found == 0) return;
    if (t == 0) s_base = atomicAdd(a.count, (unsigned long long)found);
    __syncthreads();
    const unsigned long long base = s_base;
    for (uint32_t i = t; i < found; i += 256)
      if (base + i < a.out_cap) a.out[base + i] = stage[i];
    return;
  }

  // epilogue: wave w holds rows 16 w .. 16 w + 15 of tile ti against the 64 positions of tile tj
  const uint32_t sb = diag ? 0u : kTile;  // tile tj's row state
#pragma unroll
  for (uint32_t nb = 0; nb < 4; ++nb) {
#pragma unroll
    for (uint32_t reg = 0; reg < 4; ++reg) {
      const uint32_t ra = wave * 16 + matrix::cd_row(lane, reg), rb = nb * 16 + matrix::cd_col(lane);
      const uint32_t pa = ti * kTile + ra, pb = tj * kTile + rb;
      const bool live = pa < m && pb < m && (!diag || pa <= pb);
      uint32_t common = 0, total = 0;
      uint64_t ab = 0, ba = 0;
      bool flagged = false;
      if (live) {
        const uint32_t ga = s_row[ra], gb = s_row[sb + rb];
        matrix::cell_counts(pa == pb || ga == gb, a.sk + (uint64_t)ga * a.s, s_len[ra], s_last[ra],
                            a.sk + (uint64_t)gb * a.s, s_len[sb + rb], s_last[sb + rb], (uint32_t)acc[nb][reg], &common,
                            &total);
        ab = c0 + (uint64_t)pa * m + pb;
        ba = c0 + (uint64_t)pb * m + pa;
        if (a.common) {
          a.common[ab] = common;
          a.common[ba] = common;
        }
        if (a.total) {
          a.total[ab] = total;
          a.total[ba] = total;
        }
        if (a.ani) {
          const ani::Value v = ani::value(common, total, a.k, a.E, DeviceLog{});
          a.ani[ab] = v.f;
          a.ani[ba] = v.f;
          flagged = v.flagged;
        }
      }
      // (a * m + b < 2^30; a flagged cell is off the diagonal, a < b or of an off-diagonal tile)
      if constexpr (L::kGroups) {  // (a cell index is < 2^32: group_limits_ok)
        if (a.ani) {
          ani_flag_push(flagged, (uint32_t)ab, common, total, a.list, a.cap, a.count);
          ani_flag_push(flagged, (uint32_t)ba, common, total, a.list, a.cap, a.count);
        }
      } else {
        if (a.ani) ani_flag_push(flagged, pa * a.m + pb, common, total, a.list, a.cap, a.count);
      }
    }
  }
}

uint32_t bits_for(uint32_t values) {  // the bits that hold 0 .. values - 1
  uint32_t b = 1;
  while (b < 32 && (1ull << b) < values) ++b;
  return b;
}

// flags, their inclusive sum and the ids of the sorted entries by one column rule
template <class Rule>
hipError_t columns_by(const Rule& rule, const uint64_t* K, const uint32_t* slot_of, uint32_t N, const uint32_t* pos_off,
                      uint32_t m, uint64_t* flags, uint64_t* sums, uint32_t* id_of, void* tmp, size_t tmp_bytes,
                      hipStream_t st) {
  hipLaunchKernelGGL(mx_flags_kernel<Rule>, grid_for(N), dim3(256), 0, st, K, N, pos_off, m, rule, flags);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipcub::DeviceScan::InclusiveSum(tmp, tmp_bytes, (const uint64_t*)flags, sums, (int)N, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mx_ids_kernel<Rule>, grid_for(N), dim3(256), 0, st, K, slot_of, sums, pos_off, m, rule, id_of);
  return hipGetLastError();
}

}  // namespace

// The positions part of every form, up to the one read-back before the
// product: pos_row / pos_len / piece / piece_cnt in context scratch and the
// counts.  m s < 2^31 (the caller's check).  Synchronises st.  The form selects
// three things, everything else is one sequence:
//   the positions and their offsets -- kRows at m <= kMaxRows: mx_offsets_kernel;
//     more rows (the pair and border forms), and kGroups always:
//     mx_positions_kernel and a scan; kBorder (m == n >= n_old, the caller's
//     check; d_rows is not read): the border's positions as a row list first;
//     kGroups: every group's first entry (mxg_segments_kernel);
//   kGroups with two groups or more: after the 64-bit sort a stable sort of
//     (group, slot) on the group's bits and a gather of the hashes (a segmented
//     sort over the groups' entry ranges was measured and dropped, DESIGN.md
//     4.11); one group: the group words are cleared;
//   the column rule -- plain, the border's (mxb_starts_kernel and an inclusive
//     max give every sorted entry the first entry of its run; new_entries is
//     counted) or the group's (ids local to a group).
gg_status matrix_prepare(gg_ctx* c, const char* who, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                         const uint32_t* d_rows, uint32_t m, const MatrixForm& form, MatrixPrep* out, hipStream_t st) {
  const uint32_t s = c->s, G = form.n_groups;
  const uint32_t N = (uint32_t)((uint64_t)m * s);
  const bool border = form.kind == MatrixForm::kBorder, groups = form.kind == MatrixForm::kGroups;
  const uint32_t n_new = border ? n - form.n_old : 0u;
  uint32_t *pos_row, *pos_len, *pos_off, *vals_in, *vals_out, *piece, *piece_cnt, *pos_grp = nullptr;
  uint64_t *keys_in, *keys_out, *sums, *h_back;
  if (groups) {  // m + 1 words each: pos_len is scanned in place
    GG_HIP(c, scratch_t(c, "mxg_pos", (size_t)5 * (m + 1), &pos_row));
    pos_len = pos_row + (m + 1);
    pos_grp = pos_len + (m + 1);
    pos_off = pos_grp + (m + 1);
    piece_cnt = pos_off + (m + 1);
  } else {
    GG_HIP(c, scratch_t(c, "mx_pos", (size_t)4 * m + 1, &pos_row));
    pos_len = pos_row + m;
    piece_cnt = pos_len + m;
    pos_off = piece_cnt + m;
  }
  GG_HIP(c, scratch_t(c, "mx_keys_in", (size_t)N, &keys_in));
  GG_HIP(c, scratch_t(c, "mx_keys_out", (size_t)N, &keys_out));
  GG_HIP(c, scratch_t(c, "mx_sums", (size_t)N, &sums));
  GG_HIP(c, scratch_t(c, "mx_vals_in", (size_t)N, &vals_in));
  GG_HIP(c, scratch_t(c, "mx_vals_out", (size_t)N, &vals_out));
  GG_HIP(c, scratch_t(c, "mx_piece", (size_t)N, &piece));
  GG_HIP(c, host_scratch_t(c, "mx_back", 3, &h_back));
  const bool scanned = groups || m > matrix::kMaxRows;  // the offsets by mx_positions_kernel and a scan
  const int group_bits = (int)bits_for(G + 1);
  size_t sort_bytes = 0, sort2_bytes = 0, scan_bytes = 0, off_bytes = 0, max_bytes = 0, red_bytes = 0;
  GG_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                               (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)N, 0, 64));
  GG_HIP(c, hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)N));
  if (scanned)
    GG_HIP(c, hipcub::DeviceScan::ExclusiveSum(nullptr, off_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                               (int)(m + 1)));
  uint32_t *grp_in = nullptr, *grp_out = nullptr;  // (groups) the group of every entry, before and after the second sort
  if (groups) {
    GG_HIP(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort2_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                 (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)N, 0, group_bits));
    GG_HIP(c, scratch_t(c, "mxg_grp_in", (size_t)N, &grp_in));
    GG_HIP(c, scratch_t(c, "mxg_grp_out", (size_t)N, &grp_out));
  }
  uint32_t *b_rows = nullptr, *b_new = nullptr;  // (the border) the row list; the new positions' kept entries
  if (border) {
    GG_HIP(c, hipcub::DeviceScan::InclusiveScan(nullptr, max_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                hipcub::Max(), (int)N));
    GG_HIP(c, hipcub::DeviceReduce::Sum(nullptr, red_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n_new));
    GG_HIP(c, scratch_t(c, "mxb_rows", (size_t)m + 1, &b_rows));
    b_new = b_rows + m;
  }
  const size_t tmp_bytes = std::max({sort_bytes, sort2_bytes, scan_bytes, off_bytes, max_bytes, red_bytes});
  uint8_t* tmp;
  GG_HIP(c, scratch_t(c, "mx_tmp", std::max<size_t>(tmp_bytes, 1), &tmp));

  size_t bytes = tmp_bytes;
  if (border) {
    hipLaunchKernelGGL(mxb_rows_kernel, grid_for(m), dim3(256), 0, st, n, form.n_old, b_rows);
    GG_HIP(c, hipGetLastError());
    d_rows = b_rows;
  }
  if (!scanned) {
    hipLaunchKernelGGL(mx_offsets_kernel, dim3(1), dim3(kOffBlock), 0, st, d_lens, n, s, d_rows, m, pos_row, pos_len,
                       pos_off);
    GG_HIP(c, hipGetLastError());
  } else {
    uint32_t* len1 = pos_len;  // the m lengths and a 0 behind them: the scan's last item is the number of entries
    if (groups) {
      hipLaunchKernelGGL(mx_positions_kernel<true>, grid_for((uint64_t)m + 1), dim3(256), 0, st, d_lens, n, s, d_rows, m,
                         pos_row, pos_len, len1, form.d_offsets, G, pos_grp);
    } else {
      GG_HIP(c, scratch_t(c, "mxp_len1", (size_t)m + 1, &len1));
      hipLaunchKernelGGL(mx_positions_kernel<false>, grid_for((uint64_t)m + 1), dim3(256), 0, st, d_lens, n, s, d_rows, m,
                         pos_row, pos_len, len1, nullptr, 0u, nullptr);
    }
    GG_HIP(c, hipGetLastError());
    GG_HIP(c, hipcub::DeviceScan::ExclusiveSum(tmp, bytes, (const uint32_t*)len1, pos_off, (int)(m + 1), st));
  }
  if (groups) {
    hipLaunchKernelGGL(mxg_segments_kernel, grid_for((uint64_t)G + 1), dim3(256), 0, st, form.d_offsets, G, pos_off,
                       form.d_seg);
    GG_HIP(c, hipGetLastError());
  }
  hipLaunchKernelGGL(mx_keys_kernel, grid_for(N), dim3(256), 0, st, d_sk, s, m, pos_row, pos_len, pos_off, keys_in,
                     vals_in);
  GG_HIP(c, hipGetLastError());
  // K, slot_of: the sorted entries; everything from the number of entries on is padding
  uint64_t* K = keys_out;
  uint32_t* slot_of = vals_out;
  bytes = tmp_bytes;
  GG_HIP(c, hipcub::DeviceRadixSort::SortPairs(tmp, bytes, (const uint64_t*)keys_in, keys_out, (const uint32_t*)vals_in,
                                               vals_out, (int)N, 0, 64, st));
  if (groups && G > 1) {  // by (group, hash)
    hipLaunchKernelGGL(mxg_entry_groups_kernel, grid_for(N), dim3(256), 0, st, vals_out, N, s, pos_grp, G, grp_in);
    GG_HIP(c, hipGetLastError());
    bytes = tmp_bytes;
    GG_HIP(c, hipcub::DeviceRadixSort::SortPairs(tmp, bytes, (const uint32_t*)grp_in, grp_out, (const uint32_t*)vals_out,
                                                 vals_in, (int)N, 0, group_bits, st));
    slot_of = vals_in;
    K = keys_in;
    hipLaunchKernelGGL(mxg_gather_kernel, grid_for(N), dim3(256), 0, st, d_sk, s, pos_row, slot_of, pos_off, m, K);
    GG_HIP(c, hipGetLastError());
  } else if (groups) {
    GG_HIP(c, hipMemsetAsync(grp_out, 0, (size_t)N * sizeof(uint32_t), st));
  }
  uint64_t* flags = K == keys_out ? keys_in : keys_out;  // (the buffer the sorted keys are not in)
  uint32_t* id_of = slot_of == vals_out ? vals_in : vals_out;
  bytes = tmp_bytes;
  if (border) {
    // every entry's run start: the two u32 arrays that are free until the ids (vals_in) and the pieces are written
    uint32_t *start_in = vals_in, *start1 = piece;
    hipLaunchKernelGGL(mxb_starts_kernel, grid_for(N), dim3(256), 0, st, K, N, pos_off, m, start_in);
    GG_HIP(c, hipGetLastError());
    GG_HIP(c, hipcub::DeviceScan::InclusiveScan(tmp, bytes, (const uint32_t*)start_in, start1, hipcub::Max(), (int)N, st));
    GG_HIP(c, columns_by(BorderRule{slot_of, start1, s, n_new}, K, slot_of, N, pos_off, m, flags, sums, id_of, tmp,
                         tmp_bytes, st));
  } else if (groups) {
    GG_HIP(c, columns_by(GroupRule{grp_out, form.d_seg}, K, slot_of, N, pos_off, m, flags, sums, id_of, tmp, tmp_bytes, st));
  } else {
    GG_HIP(c, columns_by(PlainRule{}, K, slot_of, N, pos_off, m, flags, sums, id_of, tmp, tmp_bytes, st));
  }
  hipLaunchKernelGGL(mx_pieces_kernel, dim3(m), dim3(256), 0, st, id_of, pos_len, s, piece, piece_cnt);
  GG_HIP(c, hipGetLastError());
  // entries, columns, column entries: the one read-back before the product
  GG_HIP(c, hipMemcpyAsync(&h_back[0], sums + (N - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  GG_HIP(c, hipMemcpyAsync(&h_back[1], pos_off + m, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  h_back[2] = 0;
  if (border && n_new) {  // with them, the kept entries of the new positions (the first n_new piece counts)
    bytes = tmp_bytes;
    GG_HIP(c, hipcub::DeviceReduce::Sum(tmp, bytes, (const uint32_t*)piece_cnt, b_new, (int)n_new, st));
    GG_HIP(c, hipMemcpyAsync(&h_back[2], b_new, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  }
  GG_HIP(c, hipStreamSynchronize(st));
  const uint64_t n_columns = (uint32_t)h_back[0], column_entries = h_back[0] >> 32, n_entries = (uint32_t)h_back[1];
  const uint64_t new_entries = (uint32_t)h_back[2];
  if (n_entries > N || column_entries > n_entries || 2 * n_columns > column_entries)
    return fail(c, GG_ERR_INTERNAL, std::string(who) + ": bad column counts");
  if (border && (new_entries > column_entries || new_entries < n_columns))
    return fail(c, GG_ERR_INTERNAL, std::string(who) + ": bad border column counts");
  *out = MatrixPrep{pos_row, pos_len, piece, piece_cnt, m, n_entries, n_columns, column_entries, new_entries};
  return GG_OK;
}

namespace {

// the fields every form's launch takes from the context and the positions part
template <class L>
L launch_of(gg_ctx* c, const uint64_t* d_sk, const MatrixPrep& p) {
  L a{};
  a.sk = d_sk;
  a.s = c->s;
  a.m = p.m;
  a.pos_row = p.pos_row;
  a.pos_len = p.pos_len;
  a.piece = p.piece;
  a.piece_cnt = p.piece_cnt;
  a.k = c->k;
  return a;
}

// The dense product of tile_pairs workgroups over `cells` cells and the
// summary: with d_ani by ani_flagged_passes (mirror_m: its patch mirrors a
// flagged cell of one [m x m] matrix; cells_per_flagged the cells a listed
// entry stands for), else a plain launch.  Synchronises st.
template <class L>
gg_status dense_product(gg_ctx* c, const char* who, L a, uint32_t tile_pairs, uint64_t cells, uint32_t mirror_m,
                        uint64_t cells_per_flagged, const MatrixPrep& p, gg_matrix_summary* sum, hipStream_t st) {
  const dim3 grid(tile_pairs);
  uint64_t flagged = 0;
  if (tile_pairs && a.ani) {
    const gg_status r = ani_flagged_passes(
        c, who, cells,
        [&](double E, AniFlagged* list, uint64_t cap, unsigned long long* count) {
          a.E = E;
          a.list = list;
          a.cap = cap;
          a.count = count;
          hipLaunchKernelGGL(mx_common_kernel<L>, grid, dim3(256), 0, st, a);
          return hipGetLastError();
        },
        a.ani, nullptr, mirror_m, &flagged, st);
    if (r != GG_OK) return r;
  } else {
    if (tile_pairs) {
      hipLaunchKernelGGL(mx_common_kernel<L>, grid, dim3(256), 0, st, a);
      GG_HIP(c, hipGetLastError());
    }
    GG_HIP(c, hipStreamSynchronize(st));
  }
  if (sum) {
    sum->n_entries = p.n_entries;
    sum->n_columns = p.n_columns;
    sum->column_entries = p.column_entries;
    sum->ani_rechecked = cells_per_flagged * flagged;
  }
  return GG_OK;
}

// The pair and border forms' launch over prepared positions (cmin / sufmin:
// ensure_cmin's tables on the device) and its launches: one takes fewer than
// 2^32 threads, 2^24 workgroups of 256, so the tile pairs (< 2^31: the limits
// of the form) go in slices of kPairSlice, in stream order.
template <class L>
L pair_launch_of(gg_ctx* c, const uint64_t* d_sk, const MatrixPrep& p, const uint32_t* d_cmin, const uint32_t* d_sufmin,
                 gg_pair* d_out, uint64_t cap, uint64_t* d_count) {
  L a = launch_of<L>(c, d_sk, p);
  a.count = (unsigned long long*)d_count;
  a.cmin = d_cmin;
  a.sufmin = d_sufmin;
  a.tmax = 2 * c->s;
  a.zero_passes = c->sufmin_host[0] == 0;
  a.out = d_out;
  a.out_cap = cap;
  return a;
}

template <class L>
gg_status launch_pair_slices(gg_ctx* c, L a, uint32_t tile_pairs, hipStream_t st) {
  const uint32_t slice = test_pair_slice();
  for (uint32_t base = 0; base < tile_pairs; base += std::min(slice, tile_pairs - base)) {
    a.wg_base = base;
    hipLaunchKernelGGL(mx_common_kernel<L>, dim3(std::min(slice, tile_pairs - base)), dim3(256), 0, st, a);
    GG_HIP(c, hipGetLastError());
  }
  return GG_OK;
}

}  // namespace

gg_status ani_matrix_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n, const uint32_t* d_rows,
                            uint32_t m, uint32_t* d_common, uint32_t* d_total, float* d_ani, gg_matrix_summary* sum,
                            hipStream_t st) {
  if (sum) *sum = gg_matrix_summary{};
  if (m == 0) return GG_OK;
  if ((uint64_t)m * c->s >= (1ull << 31)) return fail(c, GG_ERR_INVALID_ARG, "gg_ani_matrix: 2^31 sketch slots or more");
  MatrixPrep prep;
  const gg_status ps = matrix_prepare(c, "gg_ani_matrix", d_sk, d_lens, n, d_rows, m, MatrixForm{}, &prep, st);
  if (ps != GG_OK) return ps;
  MxLaunch a = launch_of<MxLaunch>(c, d_sk, prep);
  a.common = d_common;
  a.total = d_total;
  a.ani = d_ani;
  // (ani_rechecked counts cells: the matrix mirrors each listed entry)
  return dense_product(c, "gg_ani_matrix", a, matrix::tile_pairs_of(matrix::tiles_of(m)), (uint64_t)m * m, m, 2, prep, sum,
                       st);
}

// ---- the pair form ------------------------------------------
// The product over prepared positions with the thresholded epilogue: the
// passing pairs appended to d_out (unsorted), *d_count grown by the number
// found, nothing written past cap.  Asynchronous.
gg_status pairs_matrix_launch(gg_ctx* c, const uint64_t* d_sk, const MatrixPrep& p, const uint32_t* d_cmin,
                              const uint32_t* d_sufmin, gg_pair* d_out, uint64_t cap, uint64_t* d_count,
                              hipStream_t st) {
  if (p.m < 2) return GG_OK;
  return launch_pair_slices(c, pair_launch_of<MxPairLaunch>(c, d_sk, p, d_cmin, d_sufmin, d_out, cap, d_count),
                            matrix::tile_pairs_of(matrix::tiles_of(p.m)), st);
}

// ---- the border form ----------------------------------------
// The same over positions prepared as a border of n_old = p.m - n_new: the
// border tile pairs in slices, the cells of a new position only.  Asynchronous.
gg_status pairs_border_matrix_launch(gg_ctx* c, const uint64_t* d_sk, const MatrixPrep& p, uint32_t n_new,
                                     const uint32_t* d_cmin, const uint32_t* d_sufmin, gg_pair* d_out, uint64_t cap,
                                     uint64_t* d_count, hipStream_t st) {
  if (p.m < 2 || n_new == 0) return GG_OK;
  MxBorderLaunch a = pair_launch_of<MxBorderLaunch>(c, d_sk, p, d_cmin, d_sufmin, d_out, cap, d_count);
  a.n_new = n_new;
  a.tiles_new = matrix::tiles_of(n_new);
  return launch_pair_slices(c, a, matrix::border_tile_pairs(a.tiles_new, matrix::tiles_of(p.m)), st);
}

// ---- the matrices of many groups in one call ----------------
// The layout on the host (offsets arrive from it, and it shapes the launches),
// the positions part in its grouped form, then
//   mxg_single_kernel     the one cell of every group of one position;
//   mx_common_kernel<MxGroupLaunch>  the groups of two positions or more.
namespace {

// offsets of a grouped call (host words in every form): they begin at 0,
// ascend and keep the limits; cell_off / tp_off (may be null) receive the layout
gg_status check_group_offsets(const std::string& w, const uint32_t* offsets, uint32_t n_groups, uint64_t sketch_size,
                              uint64_t* cell_off, uint32_t* tp_off, std::string& err) {
  if (!offsets) {
    err = w + ": null argument";
    return GG_ERR_INVALID_ARG;
  }
  if (offsets[0] != 0) {
    err = w + ": offsets[0] is not 0";
    return GG_ERR_INVALID_ARG;
  }
  for (uint32_t g = 0; g < n_groups; ++g)
    if (offsets[g + 1] < offsets[g]) {
      err = w + ": offsets do not ascend";
      return GG_ERR_INVALID_ARG;
    }
  if (!matrix::group_layout(offsets, n_groups, sketch_size, cell_off, tp_off)) {
    err = w + ": 2^31 sketch slots, 2^32 cells or 2^31 tile pairs, or more";
    return GG_ERR_INVALID_ARG;
  }
  return GG_OK;
}

}  // namespace

gg_status ani_matrix_groups_device(gg_ctx* c, const uint64_t* d_sk, const uint32_t* d_lens, uint32_t n,
                                   const uint32_t* d_members, const uint32_t* offsets, uint32_t n_groups,
                                   uint32_t* d_common, uint32_t* d_total, float* d_ani, gg_matrix_summary* sum,
                                   hipStream_t st) {
  const char* who = "gg_ani_matrix_groups";
  if (sum) *sum = gg_matrix_summary{};
  if (n_groups == 0) return GG_OK;
  const uint32_t G = n_groups;
  uint32_t *h_off, *h_tp, *d_off, *d_tp, *d_seg;
  uint64_t *h_cell, *d_cell;
  GG_HIP(c, host_scratch_t(c, "mxg_h_off", (size_t)2 * (G + 1), &h_off));
  GG_HIP(c, host_scratch_t(c, "mxg_h_cell", (size_t)G + 1, &h_cell));
  h_tp = h_off + (G + 1);
  std::string err;
  const gg_status chk = check_group_offsets(who, offsets, G, c->s, h_cell, h_tp, err);
  if (chk != GG_OK) return fail(c, chk, err);
  const uint32_t P = offsets[G];
  if (P == 0) return GG_OK;
  memcpy(h_off, offsets, (size_t)(G + 1) * sizeof(uint32_t));
  bool singles = false;
  for (uint32_t g = 0; g < G && !singles; ++g) singles = offsets[g + 1] - offsets[g] == 1;
  GG_HIP(c, scratch_t(c, "mxg_off", (size_t)3 * (G + 1), &d_off));
  d_tp = d_off + (G + 1);
  d_seg = d_tp + (G + 1);
  GG_HIP(c, scratch_t(c, "mxg_cell", (size_t)G + 1, &d_cell));
  GG_HIP(c, hipMemcpyAsync(d_off, h_off, (size_t)2 * (G + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  GG_HIP(c, hipMemcpyAsync(d_cell, h_cell, (size_t)(G + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  MatrixPrep prep;
  const gg_status ps = matrix_prepare(c, who, d_sk, d_lens, n, d_members, P, MatrixForm{MatrixForm::kGroups, 0, d_off, d_seg, G},
                                      &prep, st);
  if (ps != GG_OK) return ps;
  if (singles) {
    hipLaunchKernelGGL(mxg_single_kernel, grid_for(G), dim3(256), 0, st, d_off, d_cell, G, prep.pos_len, d_common, d_total,
                       d_ani);
    GG_HIP(c, hipGetLastError());
  }
  MxGroupLaunch a = launch_of<MxGroupLaunch>(c, d_sk, prep);
  a.m = 0;  // (not read: a workgroup finds its group's positions in offsets)
  a.common = d_common;
  a.total = d_total;
  a.ani = d_ani;
  a.offsets = d_off;
  a.tp_off = d_tp;
  a.cell_off = d_cell;
  a.n_groups = G;
  // (the tile pairs' and the cells' totals are the host's; both sides of the diagonal are listed: no mirror)
  return dense_product(c, who, a, h_tp[G], h_cell[G], 0, 1, prep, sum, st);
}

// ---- the host-input forms: the argument tests and the upload they share ----------
// The tests come in two steps, since an entry point runs tests of its own
// before, between and after them; the message goes to `err`.  rows: the row
// list or the members of `count` positions (null: rows 0 .. count - 1).
gg_status check_sketch_arrays(const std::string& w, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                              const uint32_t* rows, bool rows_needed, uint32_t count, std::string& err) {
  if ((rows_needed && !rows) || (n && (!sketches || !lens))) {
    err = w + ": null argument";
    return GG_ERR_INVALID_ARG;
  }
  if (!rows && count > n) {
    err = w + ": more positions than rows";
    return GG_ERR_INVALID_ARG;
  }
  return GG_OK;
}

gg_status check_sketch_rows(const std::string& w, const uint32_t* lens, uint32_t n, uint32_t sketch_size,
                            const uint32_t* rows, uint32_t count, bool listed_once, std::string& err) {
  for (uint32_t g = 0; g < n; ++g)
    if (lens[g] > sketch_size) {
      err = w + ": sketch longer than sketch_size";
      return GG_ERR_INVALID_ARG;
    }
  std::vector<uint8_t> seen(rows && listed_once ? n : 0, 0);
  for (uint32_t a = 0; rows && a < count; ++a) {
    if (rows[a] >= n) {
      err = w + ": row index out of range";
      return GG_ERR_INVALID_ARG;
    }
    if (listed_once && seen[rows[a]]++) {
      err = w + ": row index listed twice";
      return GG_ERR_INVALID_ARG;
    }
  }
  return GG_OK;
}

gg_status upload_sketch_rows(gg_ctx* c, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint32_t* rows,
                             uint32_t count, uint64_t** d_sk, uint32_t** d_len, uint32_t** d_rows, hipStream_t st) {
  *d_rows = nullptr;
  GG_HIP(c, scratch_t(c, "mx_h_sk", (size_t)n * c->s, d_sk));
  GG_HIP(c, scratch_t(c, "mx_h_len", (size_t)n, d_len));
  GG_HIP(c, hipMemcpyAsync(*d_sk, sketches, (size_t)n * c->s * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  GG_HIP(c, hipMemcpyAsync(*d_len, lens, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (rows) {
    GG_HIP(c, scratch_t(c, "mx_h_rows", (size_t)count, d_rows));
    GG_HIP(c, hipMemcpyAsync(*d_rows, rows, (size_t)count * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  return GG_OK;
}

namespace {

// the checks of the dense host-input forms (the message goes to `err`): rows /
// count the row list of gg_ani_matrix, or the members of a grouped call, whose
// offsets (non-null) are checked first; *none: there is no position, nothing is run
gg_status check_dense_input(const std::string& w, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                            uint32_t sketch_size, int k, const uint32_t* rows, uint32_t count, const uint32_t* offsets,
                            uint32_t n_groups, bool grouped, const void* common, const void* total, const void* ani,
                            bool* none, std::string& err) {
  *none = true;
  if (k < 1 || k > 32 || sketch_size < 1) {
    err = w + ": kmer_length must be 1..32 and sketch_size at least 1";
    return GG_ERR_INVALID_ARG;
  }
  if (grouped) {
    const gg_status st = check_group_offsets(w, offsets, n_groups, sketch_size, nullptr, nullptr, err);
    if (st != GG_OK) return st;
    count = offsets[n_groups];
  } else if (count > matrix::kMaxRows) {
    err = w + ": more than 32768 rows listed";
    return GG_ERR_INVALID_ARG;
  }
  if (count == 0) return GG_OK;
  *none = false;
  if (!common && !total && !ani) {
    err = w + ": no output asked for";
    return GG_ERR_INVALID_ARG;
  }
  const gg_status st = check_sketch_arrays(w, sketches, lens, n, rows, grouped, count, err);
  return st != GG_OK ? st : check_sketch_rows(w, lens, n, sketch_size, rows, count, false, err);
}

// The host frame of the dense forms: the rows up, run(d_sk, d_len, d_rows,
// d_common, d_total, d_ani) on the context's stream, the outputs asked for down.
template <class Run>
gg_status dense_from_host(gg_ctx* pm, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint32_t* rows,
                          uint32_t count, size_t cells, uint32_t* common, uint32_t* total, float* ani, const Run& run) {
  gg_status st = use_device(pm);
  if (st != GG_OK) return st;
  uint64_t* d_sk = nullptr;
  uint32_t *d_len = nullptr, *d_rows = nullptr, *d_common = nullptr, *d_total = nullptr;
  float* d_ani = nullptr;
  st = upload_sketch_rows(pm, sketches, lens, n, rows, count, &d_sk, &d_len, &d_rows, pm->stream);
  if (st != GG_OK) return st;
  if (common) GG_HIP(pm, scratch_t(pm, "mx_h_common", cells, &d_common));
  if (total) GG_HIP(pm, scratch_t(pm, "mx_h_total", cells, &d_total));
  if (ani) GG_HIP(pm, scratch_t(pm, "mx_h_ani", cells, &d_ani));
  st = run(d_sk, d_len, d_rows, d_common, d_total, d_ani);
  if (st != GG_OK) return st;
  if (common) GG_HIP(pm, hipMemcpyAsync(common, d_common, cells * 4, hipMemcpyDeviceToHost, pm->stream));
  if (total) GG_HIP(pm, hipMemcpyAsync(total, d_total, cells * 4, hipMemcpyDeviceToHost, pm->stream));
  if (ani) GG_HIP(pm, hipMemcpyAsync(ani, d_ani, cells * 4, hipMemcpyDeviceToHost, pm->stream));
  GG_HIP(pm, hipStreamSynchronize(pm->stream));
  return GG_OK;
}

gg_status ani_matrix_ctx(gg_ctx* pm, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint32_t* rows,
                         uint32_t m, uint32_t* common, uint32_t* total, float* ani, gg_matrix_summary* summary) {
  std::string err;
  bool none;
  const gg_status chk = check_dense_input("gg_ani_matrix", sketches, lens, n, pm->s, pm->k, rows, m, nullptr, 0, false,
                                          common, total, ani, &none, err);
  if (chk != GG_OK) return fail(pm, chk, err);
  if (none) return GG_OK;
  return dense_from_host(pm, sketches, lens, n, rows, m, (size_t)m * m, common, total, ani,
                         [&](const uint64_t* d_sk, const uint32_t* d_len, const uint32_t* d_rows, uint32_t* d_common,
                             uint32_t* d_total, float* d_ani) {
                           return ani_matrix_device(pm, d_sk, d_len, n, d_rows, m, d_common, d_total, d_ani, summary,
                                                    pm->stream);
                         });
}

gg_status ani_matrix_groups_ctx(gg_ctx* pm, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                                const uint32_t* members, const uint32_t* offsets, uint32_t n_groups, uint32_t* common,
                                uint32_t* total, float* ani, gg_matrix_summary* summary) {
  std::string err;
  bool none;
  const gg_status chk = check_dense_input("gg_ani_matrix_groups", sketches, lens, n, pm->s, pm->k, members, 0, offsets,
                                          n_groups, true, common, total, ani, &none, err);
  if (chk != GG_OK) return fail(pm, chk, err);
  if (none) return GG_OK;
  uint64_t cells = 0;
  for (uint32_t g = 0; g < n_groups; ++g) cells += (uint64_t)(offsets[g + 1] - offsets[g]) * (offsets[g + 1] - offsets[g]);
  return dense_from_host(pm, sketches, lens, n, members, offsets[n_groups], (size_t)cells, common, total, ani,
                         [&](const uint64_t* d_sk, const uint32_t* d_len, const uint32_t* d_members, uint32_t* d_common,
                             uint32_t* d_total, float* d_ani) {
                           return ani_matrix_groups_device(pm, d_sk, d_len, n, d_members, offsets, n_groups, d_common,
                                                           d_total, d_ani, summary, pm->stream);
                         });
}

}  // namespace
}  // namespace gg

using namespace gg;

extern "C" {

gg_status gg_ani_matrix_host(const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t sketch_size,
                             int kmer_length, const uint32_t* rows, uint32_t m, uint32_t* common, uint32_t* total,
                             float* ani) {
  std::string err;
  bool none;
  const gg_status st = check_dense_input("gg_ani_matrix_host", sketches, lens, n, sketch_size, kmer_length, rows, m,
                                         nullptr, 0, false, common, total, ani, &none, err);
  if (st != GG_OK) {
    set_thread_error(err);
    return st;
  }
  // the merge itself per unordered pair (a row against itself gives its length twice), mirrored
  for (uint32_t a = 0; a < m; ++a) {
    const uint32_t ga = rows ? rows[a] : a;
    for (uint32_t b = a; b < m; ++b) {
      const uint32_t gb = rows ? rows[b] : b;
      uint32_t c, t;
      validate::merge_counts(sketches + (size_t)ga * sketch_size, lens[ga], sketches + (size_t)gb * sketch_size, lens[gb],
                             &c, &t);
      const size_t ab = (size_t)a * m + b, ba = (size_t)b * m + a;
      if (common) common[ab] = common[ba] = c;
      if (total) total[ab] = total[ba] = t;
      if (ani) ani[ab] = ani[ba] = (float)ani_f64(c, t, kmer_length);
    }
  }
  return GG_OK;
}

gg_status gg_ani_matrix(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n, const uint32_t* rows,
                        uint32_t m, uint32_t* common, uint32_t* total, float* ani, gg_matrix_summary* summary) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  if (summary) *summary = gg_matrix_summary{};
  const gg_status st = ani_matrix_ctx(pm, sketches, lens, n, rows, m, common, total, ani, summary);
  return finish_call(ctx, pm, st, [&] { if (summary) *summary = gg_matrix_summary{}; });
}

gg_status gg_ani_matrix_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                               const uint32_t* d_rows, uint32_t m, uint32_t* d_common, uint32_t* d_total, float* d_ani,
                               gg_matrix_summary* summary, void* stream) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  gg_status st = GG_OK;
  if (summary) *summary = gg_matrix_summary{};
  if (m > matrix::kMaxRows)
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_ani_matrix_device: more than 32768 rows listed");
  else if (m && !d_common && !d_total && !d_ani)
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_ani_matrix_device: no output asked for");
  else if (m && n && (!d_sketches || !d_lens))
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_ani_matrix_device: null buffer");
  else if ((st = use_device(pm)) == GG_OK)
    st = ani_matrix_device(pm, d_sketches, d_lens, n, d_rows, m, d_common, d_total, d_ani, summary, (hipStream_t)stream);
  return finish_call(ctx, pm, st, [&] { if (summary) *summary = gg_matrix_summary{}; });
}

gg_status gg_ani_matrix_files(gg_ctx* ctx, const char* const* paths, uint32_t n_paths, const char* cache_dir,
                              uint32_t* common, uint32_t* total, float* ani, gg_matrix_summary* summary) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  if (summary) *summary = gg_matrix_summary{};
  if (n_paths && !paths) return fail(ctx, GG_ERR_INVALID_ARG, "gg_ani_matrix_files: null argument");
  if (n_paths > matrix::kMaxRows) return fail(ctx, GG_ERR_INVALID_ARG, "gg_ani_matrix_files: more than 32768 files");
  if (n_paths && !common && !total && !ani)
    return fail(ctx, GG_ERR_INVALID_ARG, "gg_ani_matrix_files: no output asked for");
  const uint32_t s = primary(ctx)->s;
  std::vector<uint64_t> sk((size_t)std::max<uint32_t>(n_paths, 1) * s);
  std::vector<uint32_t> lens(std::max<uint32_t>(n_paths, 1));
  const gg_status st = gg_sketch_files(ctx, paths, n_paths, cache_dir, sk.data(), lens.data(), nullptr);
  if (st != GG_OK) return st;
  return gg_ani_matrix(ctx, sk.data(), lens.data(), n_paths, nullptr, n_paths, common, total, ani, summary);
}

gg_status gg_ani_matrix_group_cells(const uint32_t* offsets, uint32_t n_groups, uint64_t* cell_offsets) {
  std::string err;
  gg_status st = GG_OK;
  if (!cell_offsets) {
    err = "gg_ani_matrix_group_cells: null argument";
    st = GG_ERR_INVALID_ARG;
  } else {
    st = check_group_offsets("gg_ani_matrix_group_cells", offsets, n_groups, 1, cell_offsets, nullptr, err);
  }
  if (st != GG_OK) set_thread_error(err);
  return st;
}

gg_status gg_ani_matrix_groups_host(const uint64_t* sketches, const uint32_t* lens, uint32_t n, uint32_t sketch_size,
                                    int kmer_length, const uint32_t* members, const uint32_t* offsets,
                                    uint32_t n_groups, uint32_t* common, uint32_t* total, float* ani) {
  std::string err;
  bool none;
  const gg_status st = check_dense_input("gg_ani_matrix_groups_host", sketches, lens, n, sketch_size, kmer_length,
                                         members, 0, offsets, n_groups, true, common, total, ani, &none, err);
  if (st != GG_OK) {
    set_thread_error(err);
    return st;
  }
  // every group on its own: the merge itself per unordered pair, mirrored
  size_t cell0 = 0;
  for (uint32_t g = 0; g < n_groups; ++g) {
    const uint32_t* rows = members + offsets[g];
    const size_t m = offsets[g + 1] - offsets[g];
    for (size_t a = 0; a < m; ++a)
      for (size_t b = a; b < m; ++b) {
        uint32_t c, t;
        validate::merge_counts(sketches + (size_t)rows[a] * sketch_size, lens[rows[a]],
                               sketches + (size_t)rows[b] * sketch_size, lens[rows[b]], &c, &t);
        const size_t ab = cell0 + a * m + b, ba = cell0 + b * m + a;
        if (common) common[ab] = common[ba] = c;
        if (total) total[ab] = total[ba] = t;
        if (ani) ani[ab] = ani[ba] = (float)ani_f64(c, t, kmer_length);
      }
    cell0 += m * m;
  }
  return GG_OK;
}

gg_status gg_ani_matrix_groups(gg_ctx* ctx, const uint64_t* sketches, const uint32_t* lens, uint32_t n,
                               const uint32_t* members, const uint32_t* offsets, uint32_t n_groups, uint32_t* common,
                               uint32_t* total, float* ani, gg_matrix_summary* summary) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  if (summary) *summary = gg_matrix_summary{};
  const gg_status st = ani_matrix_groups_ctx(pm, sketches, lens, n, members, offsets, n_groups, common, total, ani,
                                             summary);
  return finish_call(ctx, pm, st, [&] { if (summary) *summary = gg_matrix_summary{}; });
}

gg_status gg_ani_matrix_groups_device(gg_ctx* ctx, const uint64_t* d_sketches, const uint32_t* d_lens, uint32_t n,
                                      const uint32_t* d_members, const uint32_t* offsets, uint32_t n_groups,
                                      uint32_t* d_common, uint32_t* d_total, float* d_ani, gg_matrix_summary* summary,
                                      void* stream) {
  if (!ctx) return fail(nullptr, GG_ERR_INVALID_ARG, "null context");
  gg_ctx* pm = primary(ctx);
  gg_status st = GG_OK;
  if (summary) *summary = gg_matrix_summary{};
  const uint32_t P = n_groups && offsets ? offsets[n_groups] : 0;
  if (n_groups && !offsets)
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_ani_matrix_groups_device: null offsets");
  else if (P && !d_common && !d_total && !d_ani)
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_ani_matrix_groups_device: no output asked for");
  else if (P && (!d_members || (n && (!d_sketches || !d_lens))))
    st = fail(pm, GG_ERR_INVALID_ARG, "gg_ani_matrix_groups_device: null buffer");
  else if ((st = use_device(pm)) == GG_OK)
    st = ani_matrix_groups_device(pm, d_sketches, d_lens, n, d_members, offsets, n_groups, d_common, d_total, d_ani,
                                  summary, (hipStream_t)stream);
  return finish_call(ctx, pm, st, [&] { if (summary) *summary = gg_matrix_summary{}; });
}

}  // extern "C"
