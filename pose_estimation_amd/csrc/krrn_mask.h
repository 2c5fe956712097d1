// The building blocks of the kernels that write, read or scan u8 mask planes and COCO run lists, stated once:
// rle.hip (decode), rle_encode.hip, rle_iou.hip, mask_paste.hip, and the plane stores of bop.hip's visibility
// kernel. Integer and comparison code only, so the per-file -ffp-contract flags of the Makefile cannot change what
// a helper computes. Every helper is __device__ __forceinline__ and assumes a block of kMaskThreads threads.
#pragma once
#include "krrn_common.h"

namespace {

// The tile layout: one thread per pixel of a 16 x 16 tile, thread t at column t & 15, row t >> 4, so a wave is 4
// rows of 16 pixels and a wave's 64-bit ballot of a pixel flag is four 16-bit rows.
constexpr int kMaskTile = 16;
constexpr int kMaskThreads = kMaskTile * kMaskTile;
constexpr int kMaskWaves = kMaskThreads / 64;
constexpr int kMaskWaveRows = 64 / kMaskTile;
constexpr int kMaskMaxY = 65535;  // grid.y's limit: more masks than that share blocks
static_assert(kMaskTile == 16 && kMaskThreads == 256 && kMaskWaves * kMaskWaveRows == kMaskTile,
              "a row of the tile is the 16 bytes of one store, a wave is 4 whole rows");

// 16 flag bits -> 16 bytes of 0 / 1 (bit i to byte i): one row of a tile's u8 plane
__device__ __forceinline__ uint4 krrn_row_bytes(unsigned bits) {
  auto four = [](unsigned n) { return ((n & 0xfu) * 0x00204081u) & 0x01010101u; };  // the shifted copies do not overlap
  return make_uint4(four(bits), four(bits >> 4), four(bits >> 8), four(bits >> 12));
}

// The rule of the 16-byte row access, `row` = a tile row's first pixel, `left` = the frame's columns from there on:
// a whole 16-pixel row inside the frame that starts on a 16-byte boundary is one 16-byte store (or load); any other
// row goes byte by byte. Uniform over the row's 16 lanes.
__device__ __forceinline__ bool mask_row_fast(const unsigned char* row, long long left) {
  return left >= kMaskTile && (reinterpret_cast<uintptr_t>(row) & 15) == 0;
}

// One wave's 4 rows of a plane from `bal`, its ballot of the pixel flag (false outside the frame): the lane at the
// head of a fast row expands its 16 bits to one 16-byte store, a lane of any other row stores its own byte. `pix`
// is the lane's pixel in `plane`, used only where `inside`; `fast` is mask_row_fast of the lane's row.
__device__ __forceinline__ void mask_store_row(unsigned long long bal, int lane, bool inside, bool fast,
                                               unsigned char* __restrict__ plane, size_t pix) {
  const unsigned bits = (unsigned)(bal >> lane);
  if (fast) {
    if ((lane & (kMaskTile - 1)) == 0 && inside) *reinterpret_cast<uint4*>(plane + pix) = krrn_row_bytes(bits & 0xffffu);
  } else if (inside) {
    plane[pix] = bits & 1u;
  }
}

// A mask's info row (count, x lo, y lo, x hi - x lo, y hi - y lo; zeros for an empty mask) from every thread's share
// (cnt, and the lowest / highest set column and row, INT32_MAX / -1 for none): the lanes by shuffles, the waves
// through s_red in a fixed order, thread 0 writes q[0 .. 5). One barrier; a loop adds one before the next call.
__device__ __forceinline__ void mask_info_row(int cnt, int xlo, int xhi, int ylo, int yhi, int (*s_red)[5],
                                              int* __restrict__ q) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int d = 32; d > 0; d >>= 1) {
    cnt += __shfl_xor(cnt, d);
    xlo = min(xlo, __shfl_xor(xlo, d)), xhi = max(xhi, __shfl_xor(xhi, d));
    ylo = min(ylo, __shfl_xor(ylo, d)), yhi = max(yhi, __shfl_xor(yhi, d));
  }
  if (lane == 0) s_red[wave][0] = cnt, s_red[wave][1] = xlo, s_red[wave][2] = xhi, s_red[wave][3] = ylo, s_red[wave][4] = yhi;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kMaskWaves; ++w) {
      cnt += s_red[w][0];
      xlo = min(xlo, s_red[w][1]), xhi = max(xhi, s_red[w][2]);
      ylo = min(ylo, s_red[w][3]), yhi = max(yhi, s_red[w][4]);
    }
    const bool any = cnt > 0;
    q[0] = cnt, q[1] = any ? xlo : 0, q[2] = any ? ylo : 0, q[3] = any ? xhi - xlo : 0, q[4] = any ? yhi - ylo : 0;
  }
}

// Inclusive block scan of one value per thread under an associative integer `op` with identity `zero`: the wave
// scans by __shfl_up, the waves' totals go through s_tot[kMaskWaves]. v becomes the scan over the thread's own wave
// up to itself, `before` the total of the waves before it (block-wide: op(before, v)), `all` the block's total.
// One barrier; a loop adds one before the next call on the same s_tot.
template <class T, class Op>
__device__ __forceinline__ void mask_block_scan(T& v, T zero, Op op, T* s_tot, T& before, T& all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(v, d);
    if (lane >= d) v = op(up, v);
  }
  if (lane == 63) s_tot[wave] = v;
  __syncthreads();
  before = all = zero;
  for (int w = 0; w < kMaskWaves; ++w) {
    if (w < wave) before = op(before, s_tot[w]);
    all = op(all, s_tot[w]);
  }
}

// The saturating prefix sums of a run list counts[0 .. nr), kMaskThreads runs per step with a carry between the
// steps (two barriers a step). A negative count is 0 and every sum saturates at `cap`, so the sums are
// non-decreasing and never wrap whatever the counts add up to. Every thread of the block calls f(k, start, end) for
// its run k of each step, [start, end) being the run's pixels; k >= nr is an empty run. Returns the saturated total.
template <class F>
__device__ __forceinline__ long long mask_scan_runs(const int* __restrict__ counts, int nr, long long cap,
                                                    long long* s_tot, F f) {
  long long carry = 0;  // uniform: the saturated sum of the steps before this one
  for (int base = 0; base < nr; base += kMaskThreads) {  // uniform over the block
    const int k = base + threadIdx.x;
    const int c = k < nr ? max(counts[k], 0) : 0;
    long long v = c, before, all;
    mask_block_scan(v, 0ll, [](long long a, long long b) { return a + b; }, s_tot, before, all);
    f(k, min(carry + before + v - c, cap), min(carry + before + v, cap));
    carry = min(carry + all, cap);
    __syncthreads();  // the next step rewrites s_tot
  }
  return carry;
}

// the runs of mask i: [r0, r0 + nr) of arrays n_counts long; a range negative, reversed or past offs[n] is empty
__device__ __forceinline__ void mask_runs_range(const int* __restrict__ offs, int n, int n_counts, int i, int& r0, int& nr) {
  const int a = offs[i], b = offs[i + 1], total = min(offs[n], n_counts);
  r0 = a, nr = b - a;
  if (a < 0 || b < a || b > total) r0 = 0, nr = 0;
}

// the number of e[0 .. nr) that are <= p (e non-decreasing)
__device__ __forceinline__ int mask_upper_bound(const int* __restrict__ e, int nr, int p) {
  int lo = 0, hi = nr;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= p) lo = mid + 1; else hi = mid;
  }
  return lo;
}

}  // namespace
