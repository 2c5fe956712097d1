// krrn_rle_iou_f64: the intersection, areas and IoU of P (detection, ground truth) pairs of run-length encoded
// masks, taken from the run lists themselves: no plane is decoded (include/krrn_hip.h states the definition;
// tests/coco_ref.py restates it through decoded planes). Integer work plus one f64 division per pair: no atomics,
// nothing that depends on an order between threads, so a pair's result does not depend on the batch. Two launches:
//   1. rle_iou_scan_kernel, one block per mask: the inclusive prefix sums of the mask's runs into `ends` by
//      mask_scan_runs (krrn_mask.h; saturated at INT32_MAX) and, from the clipped lengths of the odd runs, a second
//      mask_block_scan into `s`: s[k] = the set pixels in runs 0 .. k. Thread 0 writes the mask's area, the last s.
//   2. rle_iou_pair_kernel, one wave per pair. The set pixels below p of a mask are F(p) = s[j - 1] + (j odd ? p -
//      ends[j - 1] : 0) with j = #{k : ends[k] <= p}, one mask_upper_bound. The lanes stride over the set
//      runs [lo, hi) of the list with fewer runs and add F_other(hi) - F_other(lo); a wave-wide integer add finishes
//      the pair. Intersection is symmetric, so which list is walked changes nothing but the work. A wave whose two
//      masks' set spans [ends[0], last odd end) do not overlap stores 0 without a search.
// Both kernels read counts / ends / s only inside a mask's own range; a range that is negative, reversed or past
// the counts is an empty mask, and a pair naming a mask outside [0, n) gives 0.
//
// krrn_box_iou_f64: the same for [x, y, w, h] boxes, one thread per pair, bop_scene._box_iou's arithmetic in f64
// with every operation rounded on its own (this file is built without FMA contraction).
#include "krrn_mask.h"

namespace {

constexpr int kIouThreads = kMaskThreads;
constexpr int kIouWaves = kMaskWaves;
constexpr long long kIouCap = 0x7fffffffll;

__global__ __launch_bounds__(kIouThreads) void rle_iou_scan_kernel(const int* __restrict__ counts,
                                                                   const int* __restrict__ offs, int n, int n_counts,
                                                                   int* __restrict__ ends, int* __restrict__ s,
                                                                   int* __restrict__ area) {
  __shared__ long long s_tot[kIouWaves];
  __shared__ int s_odd[kIouWaves];
  const int i = blockIdx.x;
  int r0, nr;
  mask_runs_range(offs, n, n_counts, i, r0, nr);
  int carry_s = 0;  // uniform: the set pixels of the steps before this one
  mask_scan_runs(counts + r0, nr, kIouCap, s_tot, [&](int k, long long e_prev, long long e) {
    // the clipped length of an odd run; the odd runs are disjoint in [0, INT32_MAX], so their sum fits an int
    int o = (k < nr && (k & 1)) ? (int)(e - e_prev) : 0, before_s, all_s;
    mask_block_scan(o, 0, [](int a, int b) { return a + b; }, s_odd, before_s, all_s);
    if (k < nr) {
      ends[r0 + k] = (int)e;
      s[r0 + k] = carry_s + before_s + o;
    }
    carry_s += all_s;  // s_odd is rewritten after the next step's first barrier
  });
  if (threadIdx.x == 0) area[i] = carry_s;
}

// F(p): the set pixels with index < p of the mask whose scans are e / s [0, nr)
__device__ __forceinline__ int iou_below(const int* __restrict__ e, const int* __restrict__ s, int nr, int p) {
  const int lo = mask_upper_bound(e, nr, p);  // the number of e[k] <= p
  if (lo >= nr) return nr > 0 ? s[nr - 1] : 0;
  if (lo == 0) return 0;
  return s[lo - 1] + ((lo & 1) ? p - e[lo - 1] : 0);
}

__device__ __forceinline__ double iou_ratio(long long num, long long den) {
  return den > 0 ? (double)num / (double)den : 0.0;
}

__global__ __launch_bounds__(kIouThreads) void rle_iou_pair_kernel(const int* __restrict__ offs, int n, int n_counts,
                                                                   const int* __restrict__ pair,
                                                                   const unsigned char* __restrict__ crowd, int P,
                                                                   const int* __restrict__ ends,
                                                                   const int* __restrict__ s,
                                                                   const int* __restrict__ area,
                                                                   int* __restrict__ inter, double* __restrict__ iou) {
  const int lane = threadIdx.x & 63;
  const long long p64 = (long long)blockIdx.x * kIouWaves + (threadIdx.x >> 6);
  if (p64 >= P) return;  // uniform over the wave; no barrier below
  const int p = (int)p64;
  const int a = pair[2 * (size_t)p], b = pair[2 * (size_t)p + 1];
  int sum = 0;
  long long area_a = 0, area_b = 0;
  if (a >= 0 && a < n && b >= 0 && b < n) {
    int ra, na, rb, nb;
    mask_runs_range(offs, n, n_counts, a, ra, na);
    mask_runs_range(offs, n, n_counts, b, rb, nb);
    area_a = area[a], area_b = area[b];
    if (na >= 2 && nb >= 2) {  // fewer runs than two: no set run
      // walk w's set runs, search in o
      const bool a_walks = na <= nb;
      const int* we = ends + (a_walks ? ra : rb);
      const int nw = a_walks ? na : nb;
      const int* oe = ends + (a_walks ? rb : ra);
      const int* os = s + (a_walks ? rb : ra);
      const int no = a_walks ? nb : na;
      const int w_last = we[((nw - 1) & 1) ? nw - 1 : nw - 2], o_last = oe[((no - 1) & 1) ? no - 1 : no - 2];
      if (max(we[0], oe[0]) < min(w_last, o_last)) {  // the set spans overlap
        for (int k = 2 * lane + 1; k < nw; k += 128) {
          const int lo = we[k - 1], hi = we[k];
          if (hi > lo) sum += iou_below(oe, os, no, hi) - iou_below(oe, os, no, lo);
        }
      }
    }
  } else {
    area_a = area_b = 0;
  }
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
  if (lane == 0) {
    const bool in_range = a >= 0 && a < n && b >= 0 && b < n;
    const bool c = crowd && crowd[p];
    inter[p] = sum;
    iou[p] = !in_range ? 0.0 : c ? iou_ratio(sum, area_a) : iou_ratio(sum, area_a + area_b - sum);
  }
}

// Python's max / min of two floats, which bop_scene._box_iou uses: the first argument unless the second beats it
__device__ __forceinline__ double box_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double box_min(double a, double b) { return b < a ? b : a; }

__global__ __launch_bounds__(kIouThreads) void box_area_kernel(const double* __restrict__ box, int n,
                                                               double* __restrict__ area) {
  const long long i = (long long)blockIdx.x * kIouThreads + threadIdx.x;
  if (i < n) area[i] = box_max(box[4 * i + 2], 0.0) * box_max(box[4 * i + 3], 0.0);
}

__global__ __launch_bounds__(kIouThreads) void box_iou_kernel(const double* __restrict__ box, int n,
                                                              const int* __restrict__ pair,
                                                              const unsigned char* __restrict__ crowd, int P,
                                                              double* __restrict__ iou) {
  const long long p = (long long)blockIdx.x * kIouThreads + threadIdx.x;
  if (p >= P) return;
  const int a = pair[2 * p], b = pair[2 * p + 1];
  double r = 0.0;
  if (a >= 0 && a < n && b >= 0 && b < n) {
    const double ax = box[4 * (size_t)a], ay = box[4 * (size_t)a + 1], aw = box[4 * (size_t)a + 2], ah = box[4 * (size_t)a + 3];
    const double bx = box[4 * (size_t)b], by = box[4 * (size_t)b + 1], bw = box[4 * (size_t)b + 2], bh = box[4 * (size_t)b + 3];
    const double iw = box_max(0.0, box_min(ax + aw, bx + bw) - box_max(ax, bx));
    const double ih = box_max(0.0, box_min(ay + ah, by + bh) - box_max(ay, by));
    const double in = iw * ih;
    const double area_a = box_max(aw, 0.0) * box_max(ah, 0.0);
    const double den = (crowd && crowd[p]) ? area_a : area_a + box_max(bw, 0.0) * box_max(bh, 0.0) - in;
    r = den > 0.0 ? in / den : 0.0;
  }
  iou[p] = r;
}

// blocks of `per` items for n items (n up to INT32_MAX: no int overflow)
inline unsigned iou_blocks(int n, int per) { return (unsigned)(((long long)n + per - 1) / per); }

}  // namespace

KRRN_API int krrn_rle_iou_ws(int n_counts, long long* n_ints) {
  if (!n_ints) return KRRN_EARG;
  if (n_counts < 0) return KRRN_ESHAPE;
  *n_ints = 2ll * n_counts;  // ends, then s
  return KRRN_OK;
}

KRRN_API int krrn_rle_iou_f64(const int* counts, int n_counts, const int* offs, int n, const int* pair,
                              const unsigned char* crowd, int P, int* ws, int* inter, double* iou, int* area,
                              void* stream) {
  if (!counts || !offs || !pair || !ws || !inter || !iou || !area) return KRRN_EARG;
  if (n < 0 || P < 0 || n_counts < 0) return KRRN_ESHAPE;
  if (P == 0 && n == 0) return KRRN_OK;
  hipStream_t st = (hipStream_t)stream;
  int* ends = ws;
  int* s = ws + n_counts;
  if (n > 0)
    hipLaunchKernelGGL(rle_iou_scan_kernel, dim3(n), dim3(kIouThreads), 0, st, counts, offs, n, n_counts, ends, s, area);
  if (P > 0)
    hipLaunchKernelGGL(rle_iou_pair_kernel, dim3(iou_blocks(P, kIouWaves)), dim3(kIouThreads), 0, st, offs, n, n_counts,
                       pair, crowd, P, ends, s, area, inter, iou);
  return krrn_launch_status();
}

KRRN_API int krrn_box_iou_f64(const double* box, int n, const int* pair, const unsigned char* crowd, int P,
                              double* iou, double* area, void* stream) {
  if (!box || !pair || !iou || !area) return KRRN_EARG;
  if (n < 0 || P < 0) return KRRN_ESHAPE;
  if (P == 0 && n == 0) return KRRN_OK;
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) hipLaunchKernelGGL(box_area_kernel, dim3(iou_blocks(n, kIouThreads)), dim3(kIouThreads), 0, st, box, n, area);
  if (P > 0)
    hipLaunchKernelGGL(box_iou_kernel, dim3(iou_blocks(P, kIouThreads)), dim3(kIouThreads), 0, st, box, n, pair, crowd, P, iou);
  return krrn_launch_status();
}
