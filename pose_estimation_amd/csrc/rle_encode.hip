// krrn_rle_encode_u8: n u8 [H][W] planes (any non-zero byte is set) to COCO run lists, the inverse of rle.hip
// (include/krrn_hip.h states the definition; the host's rle.encode is the same thing in numpy). Integer work only:
// no floating point, no atomics, no block waits for another, nothing is read back. A stream compaction in three
// launches over a per-column workspace ws [n][kEncFields][W]:
//   1. rle_count_kernel, one wave per strip of 16 columns and mask (4 strips per block). Runs follow the pixels
//      column-major, so a wave walks its strip downwards, 64 rows per step: lane r loads the 16 bytes of row y0 + r
//      (one 16-byte load or byte loads: mask_row_fast of krrn_mask.h, the rule of the plane stores), and 16 ballots
//      ("byte c of my row is set") turn the 64 x 16 bytes into one 64-bit word of rows per column. Lane c < 16
//      keeps column x0 + c: its transitions are w ^ ((w << 1) | carry), carry = the pixel above the step's first
//      row, which at y = 0 is pixel (x - 1, H - 1) (0 for x = 0): a run that ends a column and begins the next is
//      one run. Rows past H are masked out. Per column: the number of transitions, the number of set pixels, the
//      lowest and highest set row, the position of the last transition.
//   2. rle_offsets_kernel, one block per mask: the exclusive prefix sum of the columns' transition counts (the index
//      of each column's first run) and the running "last transition before column x", the steps of krrn_mask.h's
//      mask_block_scan for the (sum, max) pair at once, in chunks of 256 columns with a carry (the helper scans one
//      value: two calls would take four barriers a chunk); mask_info_row for count / box; then
//      n_runs = T + 1, the final run H W - t_{T-1}, and zeros from n_runs to the end of the slot.
//   3. rle_emit_kernel, the walk of 1 again: lane c visits the set bits of its column's transition word in
//      increasing order and stores counts[j] = t_j - t_{j-1} at j = first[x] + rank while j < max_runs; the
//      predecessor is the bit before, else the column's last transition of an earlier step, else the scan's last
//      transition before the column (0 for j = 0).
// Every kernel reads and writes only mask i's plane, workspace rows and output slots, so a mask's outputs do not
// depend on the rest of the batch.
#include "krrn_mask.h"

namespace {

constexpr int kEncThreads = kMaskThreads;
constexpr int kEncWaves = kMaskWaves;  // strips per block in count / emit
constexpr int kEncCols = kMaskTile;    // columns per strip: the bytes of one 16-byte load
// ws fields, each [W] per mask
enum { kEncTrans = 0, kEncCount, kEncYlo, kEncYhi, kEncLast, kEncFirst, kEncPrev, kEncFields };
constexpr int kEncNone = 0x7fffffff;

__device__ __forceinline__ int* enc_ws(int* ws, int i, int field, int W) {
  return ws + ((size_t)i * kEncFields + field) * (size_t)W;
}

// the strip's 64 rows from y0 as one word of rows per column: lane c < 16 gets column x0 + c's (bit r = row y0 + r)
__device__ __forceinline__ unsigned long long enc_words(const unsigned char* __restrict__ plane, int H, int W, int x0,
                                                        int y0, int lane) {
  const int y = y0 + lane;
  uint4 q = make_uint4(0u, 0u, 0u, 0u);
  if (y < H) {
    const unsigned char* row = plane + (size_t)y * W + x0;
    if (mask_row_fast(row, W - x0)) {
      q = *reinterpret_cast<const uint4*>(row);
    } else {
      unsigned v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int c = 0; c < kEncCols; ++c)
        if (c < W - x0) v[c >> 2] |= (unsigned)row[c] << ((c & 3) * 8);
      q = make_uint4(v[0], v[1], v[2], v[3]);
    }
  }
  const unsigned v[4] = {q.x, q.y, q.z, q.w};
  unsigned long long w = 0;
#pragma unroll
  for (int c = 0; c < kEncCols; ++c) {  // every lane of the wave takes part in every ballot
    const unsigned long long b = __ballot(((v[c >> 2] >> ((c & 3) * 8)) & 0xffu) != 0);
    if (lane == c) w = b;
  }
  return w;
}

// the walk that count and emit share: f(y0, w, trans) per step for the lanes that own a column
template <class F>
__device__ __forceinline__ void enc_walk(const unsigned char* __restrict__ plane, int H, int W, int x0, int lane, F f) {
  const int x = x0 + (lane & (kEncCols - 1));
  const bool own = lane < kEncCols && lane < W - x0;
  unsigned long long carry = 0;  // the pixel before the step's first row, in pixel order
  if (own && x > 0) carry = plane[(size_t)(H - 1) * W + (x - 1)] != 0;
  for (int y0 = 0; y0 < H; y0 += 64) {  // uniform over the wave
    const int rows = min(64, H - y0);
    const unsigned long long w = enc_words(plane, H, W, x0, y0, lane);  // rows past H are 0 already
    const unsigned long long valid = rows == 64 ? ~0ull : (1ull << rows) - 1ull;
    const unsigned long long trans = (w ^ ((w << 1) | carry)) & valid;
    if (own) f(y0, w, trans);
    carry = (w >> (rows - 1)) & 1ull;
  }
}

__global__ __launch_bounds__(kEncThreads) void rle_count_kernel(const unsigned char* __restrict__ mask, int n, int H,
                                                                int W, int strips, int* __restrict__ ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int strip = blockIdx.x * kEncWaves + wave;
  if (strip >= strips) return;  // uniform over the wave; no barrier in this kernel
  const int x0 = strip * kEncCols, x = x0 + (lane & (kEncCols - 1));
  for (int i = blockIdx.y; i < n; i += gridDim.y) {
    const unsigned char* plane = mask + (size_t)i * H * W;
    int nt = 0, cnt = 0, ylo = kEncNone, yhi = -1, last = -1;
    enc_walk(plane, H, W, x0, lane, [&](int y0, unsigned long long w, unsigned long long trans) {
      nt += __popcll(trans), cnt += __popcll(w);
      if (w) ylo = min(ylo, y0 + __ffsll((long long)w) - 1), yhi = y0 + 63 - __clzll((long long)w);
      if (trans) last = x * H + y0 + 63 - __clzll((long long)trans);  // < H * W: fits an int
    });
    if (lane < kEncCols && lane < W - x0) {
      enc_ws(ws, i, kEncTrans, W)[x] = nt, enc_ws(ws, i, kEncCount, W)[x] = cnt;
      enc_ws(ws, i, kEncYlo, W)[x] = ylo, enc_ws(ws, i, kEncYhi, W)[x] = yhi;
      enc_ws(ws, i, kEncLast, W)[x] = last;
    }
  }
}

__global__ __launch_bounds__(kEncThreads) void rle_offsets_kernel(int n, int H, int W, int HW, int max_runs,
                                                                  int* __restrict__ ws, int* __restrict__ counts,
                                                                  int* __restrict__ n_runs, int* __restrict__ info) {
  __shared__ int s_sum[kEncWaves], s_max[kEncWaves];
  __shared__ int s_red[kEncWaves][5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {  // uniform over the block
    const int *c_trans = enc_ws(ws, i, kEncTrans, W), *c_count = enc_ws(ws, i, kEncCount, W);
    const int *c_ylo = enc_ws(ws, i, kEncYlo, W), *c_yhi = enc_ws(ws, i, kEncYhi, W);
    const int* c_last = enc_ws(ws, i, kEncLast, W);
    int *c_first = enc_ws(ws, i, kEncFirst, W), *c_prev = enc_ws(ws, i, kEncPrev, W);
    int total = 0, tlast = -1;  // uniform: the transitions, and the last one, of the chunks before this one
    int cnt = 0, xlo = kEncNone, xhi = -1, ylo = kEncNone, yhi = -1;
    for (long long base = 0; base < W; base += kEncThreads) {
      const bool in = base + tid < W;
      const int x = in ? (int)(base + tid) : 0;
      const int nt = in ? c_trans[x] : 0, lt = in ? c_last[x] : -1;
      // mask_block_scan's steps for the (sum, max) pair at once, so that a chunk takes two barriers, not four
      int v = nt, m = lt;  // inclusive sum / max over the wave
      for (int d = 1; d < 64; d <<= 1) {
        const int uv = __shfl_up(v, d), um = __shfl_up(m, d);
        if (lane >= d) v += uv, m = max(m, um);
      }
      if (lane == 63) s_sum[wave] = v, s_max[wave] = m;
      __syncthreads();
      int before = total, mbefore = tlast, all = 0, mall = -1;
      for (int w = 0; w < kEncWaves; ++w) {
        if (w < wave) before += s_sum[w], mbefore = max(mbefore, s_max[w]);
        all += s_sum[w], mall = max(mall, s_max[w]);
      }
      const int mup = __shfl_up(m, 1);
      if (in) {
        c_first[x] = before + v - nt;
        c_prev[x] = max(max(mbefore, lane ? mup : -1), 0);  // no transition before the column: its first run is j = 0
        const int c = c_count[x];
        if (c > 0) cnt += c, xlo = min(xlo, x), xhi = max(xhi, x), ylo = min(ylo, c_ylo[x]), yhi = max(yhi, c_yhi[x]);
      }
      total += all, tlast = max(tlast, mall);
      __syncthreads();  // the next chunk rewrites s_sum / s_max
    }
    mask_info_row(cnt, xlo, xhi, ylo, yhi, s_red, info + (size_t)i * 5);
    if (tid == 0) {
      n_runs[i] = total < 0x7fffffff ? total + 1 : 0x7fffffff;
      if (total < max_runs) counts[(size_t)i * max_runs + total] = HW - max(tlast, 0);
    }
    int* slot = counts + (size_t)i * max_runs;
    for (long long k = (long long)total + 1 + tid; k < max_runs; k += kEncThreads) slot[k] = 0;
    __syncthreads();  // the next mask rewrites s_red
  }
}

__global__ __launch_bounds__(kEncThreads) void rle_emit_kernel(const unsigned char* __restrict__ mask, int n, int H,
                                                               int W, int strips, int max_runs,
                                                               const int* __restrict__ ws, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int strip = blockIdx.x * kEncWaves + wave;
  if (strip >= strips) return;  // uniform over the wave; no barrier in this kernel
  const int x0 = strip * kEncCols, x = x0 + (lane & (kEncCols - 1));
  const bool own = lane < kEncCols && lane < W - x0;
  for (int i = blockIdx.y; i < n; i += gridDim.y) {
    const unsigned char* plane = mask + (size_t)i * H * W;
    int* slot = counts + (size_t)i * max_runs;
    int j = 0, pred = 0;
    if (own) {
      j = enc_ws(const_cast<int*>(ws), i, kEncFirst, W)[x];
      pred = enc_ws(const_cast<int*>(ws), i, kEncPrev, W)[x];
    }
    enc_walk(plane, H, W, x0, lane, [&](int y0, unsigned long long w, unsigned long long trans) {
      const int p0 = x * H + y0;
      while (trans && j < max_runs) {
        const int p = p0 + __ffsll((long long)trans) - 1;
        slot[j] = p - pred;
        pred = p, ++j;
        trans &= trans - 1;
      }
    });
  }
}

}  // namespace

KRRN_API int krrn_rle_encode_ws(int n, int W, long long* n_ints) {
  if (!n_ints) return KRRN_EARG;
  if (n < 0 || W <= 0) return KRRN_ESHAPE;
  *n_ints = (long long)kEncFields * n * W;
  return KRRN_OK;
}

KRRN_API int krrn_rle_encode_u8(const unsigned char* mask, int n, int H, int W, int max_runs, int* ws, int* counts,
                                int* n_runs, int* info, void* stream) {
  if (!mask || !ws || !counts || !n_runs || !info) return KRRN_EARG;
  if (n < 0 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffll || max_runs < 1) return KRRN_ESHAPE;
  if (n == 0) return KRRN_OK;
  hipStream_t st = (hipStream_t)stream;
  const int strips = (W - 1) / kEncCols + 1;
  const dim3 walk(krrn_cdiv(strips, kEncWaves), n < kMaskMaxY ? n : kMaskMaxY);
  hipLaunchKernelGGL(rle_count_kernel, walk, dim3(kEncThreads), 0, st, mask, n, H, W, strips, ws);
  hipLaunchKernelGGL(rle_offsets_kernel, dim3(n), dim3(kEncThreads), 0, st, n, H, W, H * W, max_runs, ws, counts, n_runs,
                     info);
  hipLaunchKernelGGL(rle_emit_kernel, walk, dim3(kEncThreads), 0, st, mask, n, H, W, strips, max_runs, ws, counts);
  return krrn_launch_status();
}
