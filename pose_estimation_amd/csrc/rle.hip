// krrn_rle_decode_u8: n COCO run-length encoded masks to u8 [n][H][W] planes of 0 / 1, with each mask's pixel
// count and tight box (include/krrn_hip.h states the definition; tests/rle_ref.py restates it in numpy). Integer
// work only: no floating point, no atomics, nothing that depends on an order. Two launches:
//   1. rle_scan_kernel, one block per mask: the inclusive prefix sums of the mask's runs into `ends`, in chunks of
//      kRleChunk runs (one per thread: wave scan by shuffles, the waves' totals through LDS) with a carry between
//      chunks. Every sum saturates at H * W, so `ends` is non-decreasing and never wraps whatever the counts sum to;
//      an entry at H * W is <= no pixel, which is what the definition gives it anyway. The same pass takes the
//      mask's info row from the runs themselves: an odd run [s, e) holds e - s pixels in columns s / H .. (e - 1)
//      / H, rows s % H .. (e - 1) % H when it stays inside one column and 0 .. H - 1 when it does not; the block
//      reduces count / min / max and thread 0 writes the row. A mask's row depends on its own runs alone.
//   2. rle_tile_kernel, one block per 16 x 16 tile of the frame and mask, laid out like bop_visib_kernel: a wave is
//      4 rows of 16 pixels. Pixels are numbered column-major, so a tile column is 16 consecutive pixels: lanes
//      0 .. 15 of the first wave binary-search `ends` for the number of runs that end at or before their column's
//      first pixel, lanes 16 .. 31 for its last pixel, and the first number goes through LDS to the column's 16
//      lanes, each of which walks forward from it to its own pixel (a 16-pixel segment rarely crosses more than a
//      few runs). When every column of the tile starts and ends in the same run parity without a run ending in
//      between, the tile is filled with that parity without walking (most tiles of a frame that holds one object).
//      Stores as bop_visib_kernel: the wave's 64-bit ballot is four 16-bit rows, the lane at the head of a row
//      expands its 16 bits to one 16-byte store; a row cut by the right border, or one that does not start on a
//      16-byte boundary, takes per-pixel byte stores. Every tile stores all its pixels: no memset.
// Both kernels read `counts` / `ends` only inside the mask's own range, and take a range that is negative,
// reversed or past offs[n] as empty (an all-zero mask).
#include "krrn_common.h"

namespace {

constexpr int kRleThreads = 256;
constexpr int kRleChunk = kRleThreads;  // runs per scan step
constexpr int kRleWaves = kRleThreads / 64;
constexpr int kRleTile = 16;
constexpr int kRleMaxY = 65535;  // grid.y's limit: more masks than that share blocks

// the runs of mask i: counts / ends [r0, r0 + nr); a bad range is empty
__device__ __forceinline__ void rle_range(const int* __restrict__ offs, int n, int i, int& r0, int& nr) {
  const int a = offs[i], b = offs[i + 1], total = offs[n];
  r0 = a, nr = b - a;
  if (a < 0 || b < a || b > total) r0 = 0, nr = 0;
}

__global__ __launch_bounds__(kRleThreads) void rle_scan_kernel(const int* __restrict__ counts,
                                                               const int* __restrict__ offs, int n, int H, int HW,
                                                               int* __restrict__ ends, int* __restrict__ info) {
  __shared__ long long s_tot[kRleWaves];
  __shared__ int s_red[kRleWaves][5];
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int r0, nr;
  rle_range(offs, n, i, r0, nr);
  const long long cap = HW;
  long long carry = 0;  // uniform: the saturated sum of the chunks before this one
  int cnt = 0, xlo = 0x7fffffff, xhi = -1, ylo = 0x7fffffff, yhi = -1;
  auto ones = [&](int s, int e) {  // the set pixels [s, e), s < e <= HW
    const int x0 = s / H, x1 = (e - 1) / H;
    cnt += e - s;
    xlo = min(xlo, x0), xhi = max(xhi, x1);
    if (x1 > x0) {
      ylo = 0, yhi = H - 1;
    } else {
      ylo = min(ylo, s - x0 * H), yhi = max(yhi, (e - 1) - x0 * H);
    }
  };
  for (int base = 0; base < nr; base += kRleChunk) {  // uniform over the block
    const int k = base + tid;
    const int c = k < nr ? max(counts[r0 + k], 0) : 0;
    long long v = c;
    for (int d = 1; d < 64; d <<= 1) {
      const long long up = __shfl_up(v, d);
      if (lane >= d) v += up;
    }
    if (lane == 63) s_tot[wave] = v;
    __syncthreads();
    long long before = carry, all = 0;
    for (int w = 0; w < kRleWaves; ++w) {
      if (w < wave) before += s_tot[w];
      all += s_tot[w];
    }
    if (k < nr) {
      const long long e = min(before + v, cap), s = min(before + v - c, cap);
      ends[r0 + k] = (int)e;
      if ((k & 1) && e > s) ones((int)s, (int)e);
    }
    carry = min(carry + all, cap);
    __syncthreads();  // the next chunk rewrites s_tot
  }
  // a pixel at or past the runs' total takes the parity of the run count
  if (tid == 0 && (nr & 1) && carry < cap) ones((int)carry, HW);
  for (int d = 32; d > 0; d >>= 1) {
    cnt += __shfl_xor(cnt, d);
    xlo = min(xlo, __shfl_xor(xlo, d)), xhi = max(xhi, __shfl_xor(xhi, d));
    ylo = min(ylo, __shfl_xor(ylo, d)), yhi = max(yhi, __shfl_xor(yhi, d));
  }
  if (lane == 0) s_red[wave][0] = cnt, s_red[wave][1] = xlo, s_red[wave][2] = xhi, s_red[wave][3] = ylo, s_red[wave][4] = yhi;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kRleWaves; ++w) {
      cnt += s_red[w][0];
      xlo = min(xlo, s_red[w][1]), xhi = max(xhi, s_red[w][2]);
      ylo = min(ylo, s_red[w][3]), yhi = max(yhi, s_red[w][4]);
    }
    int* q = info + (size_t)i * 5;
    const bool any = cnt > 0;
    q[0] = cnt, q[1] = any ? xlo : 0, q[2] = any ? ylo : 0, q[3] = any ? xhi - xlo : 0, q[4] = any ? yhi - ylo : 0;
  }
}

// the number of e[0 .. nr) that are <= p (e non-decreasing)
__device__ __forceinline__ int rle_runs_upto(const int* __restrict__ e, int nr, int p) {
  int lo = 0, hi = nr;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= p) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kRleThreads) void rle_tile_kernel(const int* __restrict__ offs, int n, int H, int W,
                                                               int tiles_x, const int* __restrict__ ends,
                                                               unsigned char* __restrict__ mask) {
  __shared__ int s_k[kRleTile];
  __shared__ int s_fill;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
  const int lx = txi * kRleTile, ly = tyi * kRleTile;
  const int ty1 = min(ly + kRleTile, H) - 1;
  const int x = lx + (tid & (kRleTile - 1)), y = ly + (tid >> 4);
  const bool inside = x < W && y < H;
  const bool full = lx + kRleTile <= W;
  for (int i = blockIdx.y; i < n; i += gridDim.y) {  // uniform over the block
    int r0, nr;
    rle_range(offs, n, i, r0, nr);
    const int* e = ends + r0;
    if (wave == 0) {
      int k = 0;
      const int cx = lx + (lane & (kRleTile - 1));
      const bool col = lane < 2 * kRleTile && cx < W;
      if (col) k = rle_runs_upto(e, nr, cx * H + (lane < kRleTile ? ly : ty1));  // < H * W: fits an int
      const int last = __shfl_xor(k, kRleTile);
      const unsigned long long crossed = __ballot(col && k != last);
      const unsigned long long odd = __ballot(col && (k & 1)), cols = __ballot(col);
      if (lane < kRleTile) s_k[lane] = k;
      if (lane == 0) s_fill = crossed ? -1 : odd == 0 ? 0 : odd == cols ? 1 : -1;
    }
    __syncthreads();
    const int fill = s_fill;
    bool flag = fill == 1;
    if (fill < 0 && inside) {
      const int p = x * H + y;
      int k = s_k[tid & (kRleTile - 1)];
      while (k < nr && e[k] <= p) ++k;
      flag = k & 1;
    }
    flag = flag && inside;
    const unsigned long long bal = __ballot(flag);
    const size_t pix = ((size_t)i * H + y) * W + x;  // used only where `inside`
    const size_t row0 = ((size_t)i * H + y) * W + lx;
    if (full && ((reinterpret_cast<uintptr_t>(mask) + row0) & 15) == 0) {  // uniform over the row's 16 lanes
      if ((lane & 15) == 0 && inside)
        *reinterpret_cast<uint4*>(mask + pix) = krrn_row_bytes((unsigned)(bal >> lane) & 0xffffu);
    } else if (inside) {
      mask[pix] = flag ? 1 : 0;
    }
    __syncthreads();  // the next mask rewrites s_k / s_fill
  }
}

}  // namespace

KRRN_API int krrn_rle_decode_u8(const int* counts, const int* offs, int n, int H, int W, int* ends,
                                unsigned char* mask, int* info, void* stream) {
  if (!counts || !offs || !ends || !mask || !info) return KRRN_EARG;
  if (n < 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffll) return KRRN_ESHAPE;
  if (n == 0) return KRRN_OK;
  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = krrn_cdiv(W, kRleTile), tiles_y = krrn_cdiv(H, kRleTile);  // tiles_x * tiles_y <= H * W
  hipLaunchKernelGGL(rle_scan_kernel, dim3(n), dim3(kRleThreads), 0, st, counts, offs, n, H, H * W, ends, info);
  hipLaunchKernelGGL(rle_tile_kernel, dim3(tiles_x * tiles_y, n < kRleMaxY ? n : kRleMaxY), dim3(kRleThreads), 0, st, offs, n, H,
                     W, tiles_x, ends, mask);
  return krrn_launch_status();
}
