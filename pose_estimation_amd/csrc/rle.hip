// krrn_rle_decode_u8: n COCO run-length encoded masks to u8 [n][H][W] planes of 0 / 1, with each mask's pixel
// count and tight box (include/krrn_hip.h states the definition; tests/rle_ref.py restates it in numpy). Integer
// work only: no floating point, no atomics, nothing that depends on an order. Two launches:
//   1. rle_scan_kernel, one block per mask: the inclusive prefix sums of the mask's runs into `ends` by
//      mask_scan_runs (krrn_mask.h). Every sum saturates at H * W, so `ends` is non-decreasing and never wraps
//      whatever the counts sum to; an entry at H * W is <= no pixel, which is what the definition gives it anyway.
//      The same pass takes the mask's info row from the runs themselves: an odd run [s, e) holds e - s pixels in
//      columns s / H .. (e - 1) / H, rows s % H .. (e - 1) % H when it stays inside one column and 0 .. H - 1 when it
//      does not; mask_info_row reduces count / min / max and writes the row. A mask's row depends on its own runs
//      alone.
//   2. rle_tile_kernel, one block per 16 x 16 tile of the frame and mask, in krrn_mask.h's tile layout. Pixels are
//      numbered column-major, so a tile column is 16 consecutive pixels: lanes 0 .. 15 of the first wave
//      binary-search `ends` (mask_upper_bound) for the number of runs that end at or before their column's first
//      pixel, lanes 16 .. 31 for its last pixel, and the first number goes through LDS to the column's 16 lanes, each
//      of which walks forward from it to its own pixel (a 16-pixel segment rarely crosses more than a few runs). When
//      every column of the tile starts and ends in the same run parity without a run ending in between, the tile is
//      filled with that parity without walking (most tiles of a frame that holds one object). The wave's ballot is
//      stored by mask_store_row. Every tile stores all its pixels: no memset.
// Both kernels read `counts` / `ends` only inside the mask's own range (mask_runs_range: a range that is negative,
// reversed or past offs[n] is empty, an all-zero mask).
#include "krrn_mask.h"

namespace {

constexpr int kRleThreads = kMaskThreads;
constexpr int kRleTile = kMaskTile;

__global__ __launch_bounds__(kRleThreads) void rle_scan_kernel(const int* __restrict__ counts,
                                                               const int* __restrict__ offs, int n, int H, int HW,
                                                               int* __restrict__ ends, int* __restrict__ info) {
  __shared__ long long s_tot[kMaskWaves];
  __shared__ int s_red[kMaskWaves][5];
  const int i = blockIdx.x, tid = threadIdx.x;
  int r0, nr;
  mask_runs_range(offs, n, 0x7fffffff, i, r0, nr);
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
  const long long total = mask_scan_runs(counts + r0, nr, HW, s_tot, [&](int k, long long s, long long e) {
    if (k < nr) {
      ends[r0 + k] = (int)e;
      if ((k & 1) && e > s) ones((int)s, (int)e);
    }
  });
  // a pixel at or past the runs' total takes the parity of the run count
  if (tid == 0 && (nr & 1) && total < HW) ones((int)total, HW);
  mask_info_row(cnt, xlo, xhi, ylo, yhi, s_red, info + (size_t)i * 5);
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
  for (int i = blockIdx.y; i < n; i += gridDim.y) {  // uniform over the block
    int r0, nr;
    mask_runs_range(offs, n, 0x7fffffff, i, r0, nr);
    const int* e = ends + r0;
    if (wave == 0) {
      int k = 0;
      const int cx = lx + (lane & (kRleTile - 1));
      const bool col = lane < 2 * kRleTile && cx < W;
      if (col) k = mask_upper_bound(e, nr, cx * H + (lane < kRleTile ? ly : ty1));  // < H * W: fits an int
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
    mask_store_row(bal, lane, inside, mask_row_fast(mask + (pix - (x - lx)), W - lx), mask, pix);
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
  hipLaunchKernelGGL(rle_tile_kernel, dim3(tiles_x * tiles_y, n < kMaskMaxY ? n : kMaskMaxY), dim3(kRleThreads), 0, st,
                     offs, n, H, W, tiles_x, ends, mask);
  return krrn_launch_status();
}
