// krrn_coco_match_f64: COCO's per-image matching (pycocotools' published COCOeval.evaluateImg) for G (scene, image,
// category) groups at once, one independent matching per (group, area range, IoU threshold) cell (include/krrn_hip.h
// states the definition; tests/coco_ref.py restates it in numpy). Comparisons only: no arithmetic on the IoUs, the
// areas or the scores, no atomics, nothing that depends on an order between threads or blocks, so the result is
// bit-reproducible and a group's outputs do not depend on the rest of the batch. One launch, one block per group,
// laid out like bop_match_kernel:
//   1. the block ranks the group's detections into LDS by counting (a higher score, or the same score and a lower
//      index, precedes; a NaN score counts as -inf) and stores `rank`; the ground truths' flags and areas go to LDS.
//   2. every owned (ground truth, area range) element of gt_ig is stored from global memory by the threads in stride.
//   3. the threads stride over the group's A * T cells, consecutive lanes taking consecutive thresholds of one area
//      range. A cell holds three 128-bit sets in 64-bit scalars (ignored, crowd, matched: a per-lane array indexed
//      by j would live in scratch). COCO walks the ground truths "non-ignored first, then ignored" and stops at the
//      first ignored one once it holds a non-ignored match: that is one pass over the non-ignored j and, only if it
//      matched nothing, one pass over the ignored j. The lanes that share a detection read the same iou element (a
//      broadcast), and their dt_match / dt_ig stores are contiguous.
// Every (detection, cell) element is stored exactly once: by the walk for the first min(n_det, max_det) detections
// in rank order, as (-1, 1) for the rest. A group whose ranges break a stated limit is matched as an empty one: the
// detections and ground truths its ranges own inside the buffers get rank -1, (-1, 1) and their gt_ig.
#include "krrn_common.h"

namespace {

constexpr int kCocoThreads = 256;
constexpr int kCocoMax = 128;  // detections and ground truths per group
constexpr int kCocoMaxA = 8;
constexpr int kCocoMaxT = 16;

__device__ __forceinline__ bool coco_bit(unsigned long long b0, unsigned long long b1, int j) {
  return ((j < 64 ? b0 : b1) >> (j & 63)) & 1ull;
}

__global__ __launch_bounds__(kCocoThreads) void coco_match_kernel(
    const double* __restrict__ score, int Dtot, const int* __restrict__ det_range, const int* __restrict__ gt_range,
    const int* __restrict__ pair_off, const double* __restrict__ iou, long long Ptot,
    const double* __restrict__ det_area, const double* __restrict__ gt_area, const int* __restrict__ gt_flags, int GTtot,
    const double* __restrict__ area_rng, int A, const double* __restrict__ iou_thr, int T, int max_det, int lim_det,
    int lim_gt, int* __restrict__ dt_match, unsigned char* __restrict__ dt_ig, unsigned char* __restrict__ gt_ig,
    int* __restrict__ rank) {
  __shared__ double s_score[kCocoMax];
  __shared__ int s_order[kCocoMax];
  __shared__ double s_garea[kCocoMax];
  __shared__ int s_gflag[kCocoMax];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int d0 = det_range[2 * g], nd_in = det_range[2 * g + 1];
  const int g0 = gt_range[2 * g], ng_in = gt_range[2 * g + 1];
  const long long p0 = pair_off[g];
  // uniform over the block. What the group owns: its ranges where they lie inside the buffers
  const bool det_own = d0 >= 0 && nd_in >= 0 && (long long)d0 + nd_in <= Dtot;
  const bool gt_own = g0 >= 0 && ng_in >= 0 && (long long)g0 + ng_in <= GTtot;
  const int nd_own = det_own ? nd_in : 0, ng_own = gt_own ? ng_in : 0;
  const bool ok = det_own && gt_own && nd_in <= lim_det && ng_in <= lim_gt && p0 >= 0 &&
                  p0 + (long long)nd_in * ng_in <= Ptot;
  const int n_det = ok ? nd_in : 0, n_gt = ok ? ng_in : 0;
  const int n_use = min(n_det, max_det);
  const int cells = A * T;

  if (tid < n_det) {
    const double s = score[d0 + tid];
    s_score[tid] = s != s ? -INFINITY : s;
  }
  if (tid < n_gt) s_garea[tid] = gt_area[g0 + tid], s_gflag[tid] = gt_flags[g0 + tid];
  __syncthreads();
  if (tid < n_det) {
    const double s = s_score[tid];
    int r = 0;
    for (int o = 0; o < n_det; ++o) {
      const double q = s_score[o];
      r += (q > s || (q == s && o < tid)) ? 1 : 0;
    }
    s_order[r] = tid;
    rank[d0 + tid] = r < max_det ? r : -1;
  }
  if (!ok)
    for (int d = tid; d < nd_own; d += kCocoThreads) rank[d0 + d] = -1;
  for (long long x = tid; x < (long long)ng_own * A; x += kCocoThreads) {  // from global memory: ng_own may pass the LDS arrays
    const int j = (int)(x / A), a = (int)(x - (long long)j * A);
    const double ar = gt_area[g0 + j];
    gt_ig[(size_t)(g0 + j) * A + a] = (gt_flags[g0 + j] != 0 || ar < area_rng[2 * a] || ar > area_rng[2 * a + 1]) ? 1 : 0;
  }
  __syncthreads();

  for (int cell = tid; cell < cells; cell += kCocoThreads) {
    const int a = cell / T, t = cell - a * T;
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    const double thr_t = iou_thr[t], cap = 1.0 - 1e-10;
    const double thr = cap < thr_t ? cap : thr_t;  // min(thr_t, 1 - 1e-10)
    unsigned long long ig0 = 0ull, ig1 = 0ull, cr0 = 0ull, cr1 = 0ull, m0 = 0ull, m1 = 0ull;
    for (int j = 0; j < n_gt; ++j) {
      const double ar = s_garea[j];
      const int f = s_gflag[j];
      const unsigned long long bit = 1ull << (j & 63);
      if (f != 0 || ar < lo || ar > hi) { if (j < 64) ig0 |= bit; else ig1 |= bit; }
      if (f & 1) { if (j < 64) cr0 |= bit; else cr1 |= bit; }
    }
    for (int r = 0; r < n_use; ++r) {
      const int d = s_order[r];
      const double* row = iou + (size_t)p0 + (size_t)d * n_gt;
      double best = thr;
      int m = -1;
      for (int pass = 0; pass < 2 && m < 0; ++pass) {  // the non-ignored ground truths, then the ignored ones
        for (int j = 0; j < n_gt; ++j) {
          if (coco_bit(ig0, ig1, j) != (pass == 1)) continue;
          if (coco_bit(m0, m1, j) && !coco_bit(cr0, cr1, j)) continue;
          const double v = row[j];
          if (!(v >= best)) continue;  // below the best so far, or NaN
          best = v, m = j;
        }
      }
      const size_t out = (size_t)(d0 + d) * cells + cell;
      if (m >= 0) {
        const unsigned long long bit = 1ull << (m & 63);
        if (m < 64) m0 |= bit; else m1 |= bit;
        dt_match[out] = g0 + m;
        dt_ig[out] = coco_bit(ig0, ig1, m) ? 1 : 0;
      } else {
        const double ar = det_area[d0 + d];
        dt_match[out] = -1;
        dt_ig[out] = (ar < lo || ar > hi) ? 1 : 0;
      }
    }
    for (int r = n_use; r < n_det; ++r) {  // past max_det
      const size_t out = (size_t)(d0 + s_order[r]) * cells + cell;
      dt_match[out] = -1, dt_ig[out] = 1;
    }
    if (!ok)
      for (int d = 0; d < nd_own; ++d) {
        const size_t out = (size_t)(d0 + d) * cells + cell;
        dt_match[out] = -1, dt_ig[out] = 1;
      }
  }
}

}  // namespace

KRRN_API int krrn_coco_match_f64(const double* score, int Dtot, const int* det_range, const int* gt_range,
                                 const int* pair_off, const double* iou, long long Ptot, const double* det_area,
                                 const double* gt_area, const int* gt_flags, int GTtot, const double* area_rng, int A,
                                 const double* iou_thr, int T, int max_det, int lim_det, int lim_gt, int G,
                                 int* dt_match, unsigned char* dt_ig, unsigned char* gt_ig, int* rank, void* stream) {
  if (!det_range || !gt_range || !pair_off || !area_rng || !iou_thr) return KRRN_EARG;
  if (((!score || !det_area || !dt_match || !dt_ig || !rank) && Dtot > 0) || (!iou && Ptot > 0) ||
      ((!gt_area || !gt_flags || !gt_ig) && GTtot > 0))
    return KRRN_EARG;
  if (G < 0 || Dtot < 0 || GTtot < 0 || Ptot < 0 || Ptot > 0x7fffffffll || A < 1 || A > kCocoMaxA || T < 1 ||
      T > kCocoMaxT || max_det < 0 || max_det > kCocoMax || lim_det < 0 || lim_det > kCocoMax || lim_gt < 0 ||
      lim_gt > kCocoMax)
    return KRRN_ESHAPE;
  if (G == 0) return KRRN_OK;
  hipLaunchKernelGGL(coco_match_kernel, dim3(G), dim3(kCocoThreads), 0, (hipStream_t)stream, score, Dtot, det_range,
                     gt_range, pair_off, iou, Ptot, det_area, gt_area, gt_flags, GTtot, area_rng, A, iou_thr, T,
                     max_det, lim_det, lim_gt, dt_match, dt_ig, gt_ig, rank);
  return krrn_launch_status();
}
