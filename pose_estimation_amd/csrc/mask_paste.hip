// krrn_mask_paste_f32: the mask head's logits of B crops, each an S x S window of its frame, to u8 [B][H][W]
// full-frame planes of 0 / 1 with each plane's pixel count and tight box (include/krrn_hip.h states the definition;
// tests/paste_ref.py restates it in numpy). Comparisons and integer work only: no arithmetic on a logit, no atomics,
// nothing that depends on an order. Two launches:
//   1. mask_paste_tile_kernel, 16 x 16 tiles of the frame in krrn_mask.h's tile layout. A block takes kPasteSpan
//      tiles side by side of one crop, one after the other (a block per tile spent more time starting blocks than
//      storing: DESIGN.md section 3). A tile that the
//      crop's window cannot touch (or a crop whose chan selects nothing) stores zeros without reading a logit:
//      block-uniform, and most tiles of a frame; a whole span of them, when it is full width and its rows start on
//      16-byte boundaries, is zeroed by one 16-byte store per thread of two waves, 128 consecutive bytes a row. In a
//      touched tile each lane inside the window walks its pixel's C1 logits, channel stride S S: the 16 lanes of a
//      row read 64 consecutive bytes per channel. The wave's ballot is stored by mask_store_row. Every tile stores
//      all its pixels: no memset.
//   2. mask_paste_info_kernel, one block per crop: the set bytes of the plane inside the clipped window (no pixel
//      outside it can be set) reduced to count / min / max and written by mask_info_row. Wave w takes the window's
//      rows w, w + 4, ..; a lane its columns lane, lane + 64, ..
// The window's position is taken in 64-bit, so any rc reads and writes nothing out of bounds. Both kernels read only
// crop b's logits, chan and rc and write only its plane and info row.
#include "krrn_raster.h"  // Span / rast_overlap: the entry points' overlap check; brings krrn_mask.h

namespace {

constexpr int kPasteThreads = kMaskThreads;
constexpr int kPasteWaves = kMaskWaves;
constexpr int kPasteTile = kMaskTile;
constexpr int kPasteSpan = 8;      // tiles side by side per block: 128 columns, 8 stores of 16 bytes to a row
static_assert(kPasteSpan * kPasteTile == 8 * 16 && kPasteThreads >= 8 * kPasteTile, "the span's zero stores");

__global__ __launch_bounds__(kPasteThreads) void mask_paste_tile_kernel(const float* __restrict__ logits,
                                                                        long long ld_b, int C1, int S,
                                                                        const int* __restrict__ chan,
                                                                        const int* __restrict__ rc, int B, int H, int W,
                                                                        int spans_x, unsigned char* __restrict__ mask) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int tyi = blockIdx.x / spans_x, sxi = blockIdx.x - tyi * spans_x;
  const int ly = tyi * kPasteTile, y = ly + (tid >> 4);
  const size_t plane = (size_t)S * S;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {  // uniform over the block
    const int ch = chan[b];
    const long long rmin = rc[2 * b], cmin = rc[2 * b + 1];
    const bool rows_hit = ch >= 0 && ch < C1 && (long long)ly + kPasteTile > rmin && ly < rmin + S;
    // uniform: a whole span of full width that the window cannot touch, every row of it on a 16-byte boundary, is
    // zeroed by one 16-byte store per thread of the first two waves (8 threads to a row of 128 bytes)
    const long long sx0 = (long long)sxi * kPasteSpan * kPasteTile;
    unsigned char* span = mask + ((size_t)b * H + ly) * W + sx0;
    if (!(rows_hit && sx0 + kPasteSpan * kPasteTile > cmin && sx0 < cmin + S) && W - sx0 >= kPasteSpan * kPasteTile &&
        (W & 15) == 0 && (reinterpret_cast<uintptr_t>(span) & 15) == 0) {
      const int r = tid >> 3;
      if (r < kPasteTile && ly + r < H)
        *reinterpret_cast<uint4*>(span + (size_t)r * W + (tid & 7) * 16) = make_uint4(0u, 0u, 0u, 0u);
      continue;
    }
    for (int t = 0; t < kPasteSpan; ++t) {  // uniform over the block
      const long long lx64 = ((long long)sxi * kPasteSpan + t) * kPasteTile;
      if (lx64 >= W) break;
      const int lx = (int)lx64, x = lx + (tid & (kPasteTile - 1));
      const bool inside = x < W && y < H;
      // uniform: the tile's rows / columns against the window's rmin .. rmin + S - 1 / cmin .. cmin + S - 1
      const bool touched = rows_hit && (long long)lx + kPasteTile > cmin && lx < cmin + S;
      bool flag = false;
      if (touched && inside) {
        const long long i = y - rmin, j = x - cmin;
        if (i >= 0 && i < S && j >= 0 && j < S) {
          const float* l = logits + (size_t)b * (size_t)ld_b + (size_t)i * S + (size_t)j;
          int best = 0;
          float top = l[0];
          for (int c = 1; c < C1; ++c) {
            const float v = l[(size_t)c * plane];
            if (v > top) best = c, top = v;  // false for a NaN on either side: a NaN never wins, one in channel 0 stays
          }
          flag = ch == 0 ? best != 0 : best == ch;
        }
      }
      const unsigned long long bal = __ballot(flag);
      const size_t pix = ((size_t)b * H + y) * W + x;  // used only where `inside`
      mask_store_row(bal, lane, inside, mask_row_fast(mask + (pix - (x - lx)), W - lx), mask, pix);
    }
  }
}

__global__ __launch_bounds__(kPasteThreads) void mask_paste_info_kernel(const unsigned char* __restrict__ mask, int S,
                                                                        const int* __restrict__ rc, int B, int H, int W,
                                                                        int* __restrict__ info) {
  __shared__ int s_red[kPasteWaves][5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {  // uniform over the block
    const long long rmin = rc[2 * b], cmin = rc[2 * b + 1];
    // the window clipped to the frame: rows r0 .. r1 - 1, columns c0 .. c1 - 1 (at most S of each)
    const long long r0 = max(rmin, 0ll), r1 = min(rmin + S, (long long)H);
    const long long c0 = max(cmin, 0ll), c1 = min(cmin + S, (long long)W);
    const long long nr = r1 - r0, nc = c1 - c0;
    const long long total = nr > 0 && nc > 0 ? nr * nc : 0;  // <= S S: fits an int
    const unsigned char* p = mask + (size_t)b * H * W;
    int cnt = 0, xlo = 0x7fffffff, xhi = -1, ylo = 0x7fffffff, yhi = -1;
    if (total > 0) {
      const int rows = (int)nr, cols = (int)nc;
      for (int j = lane; j < cols; j += 64) {
        const int xx = (int)c0 + j;
        const unsigned char* q = p + (size_t)r0 * W + xx;
        int n = 0, lo = 0x7fffffff, hi = -1;  // of this column's rows wave, wave + 4, ..
#pragma unroll 8
        for (int r = wave; r < rows; r += kPasteWaves)
          if (q[(size_t)r * W]) ++n, lo = min(lo, r), hi = r;
        if (n) cnt += n, xlo = min(xlo, xx), xhi = max(xhi, xx), ylo = min(ylo, (int)r0 + lo), yhi = max(yhi, (int)r0 + hi);
      }
    }
    mask_info_row(cnt, xlo, xhi, ylo, yhi, s_red, info + (size_t)b * 5);
    __syncthreads();  // the next crop rewrites s_red
  }
}

}  // namespace

KRRN_API int krrn_mask_paste_f32(const float* logits, long long ld_b, int C1, int S, const int* chan, const int* rc,
                                 int B, int H, int W, unsigned char* mask, int* info, void* stream) {
  if (!logits || !chan || !rc || !mask || !info) return KRRN_EARG;
  if (B < 0 || C1 < 1 || S < 1 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffll ||
      (long long)S * S > 0x7fffffffll || (long long)C1 * S * S > 0x7fffffffll || ld_b < (long long)C1 * S * S)
    return KRRN_ESHAPE;
  const size_t b = (size_t)B, crop = (size_t)C1 * S * S;
  // the logits' extent, (B - 1) ld_b + C1 S S floats, cut off where the address space ends
  const size_t room = (~(size_t)0 - (size_t)(uintptr_t)logits) / 4;
  size_t elems = 0;
  if (b) {
    const size_t lim = room > crop ? (room - crop) / (b > 1 ? b - 1 : 1) : 0;
    elems = b > 1 && (size_t)ld_b > lim ? room : (b - 1) * (size_t)ld_b + crop;
    if (elems > room) elems = room;
  }
  const Span outs[2] = {{mask, b * H * W}, {info, 20 * b}};
  const Span ins[3] = {{logits, 4 * elems}, {chan, 4 * b}, {rc, 8 * b}};
  if (rast_overlap(outs, 2, ins, 3)) return KRRN_EARG;
  if (B == 0) return KRRN_OK;
  hipStream_t st = (hipStream_t)stream;
  const int tiles_y = (H - 1) / kPasteTile + 1;
  const int spans_x = (W - 1) / (kPasteTile * kPasteSpan) + 1;  // spans_x * tiles_y <= H * W
  hipLaunchKernelGGL(mask_paste_tile_kernel, dim3(spans_x * tiles_y, B < kMaskMaxY ? B : kMaskMaxY),
                     dim3(kPasteThreads), 0, st, logits, ld_b, C1, S, chan, rc, B, H, W, spans_x, mask);
  hipLaunchKernelGGL(mask_paste_info_kernel, dim3(B), dim3(kPasteThreads), 0, st, mask, S, rc, B, H, W, info);
  return krrn_launch_status();
}
