// krrn_coco_match_f64: COCO's per-image matching (pycocotools' published COCOeval.evaluateImg) for G (scene, image,
// category) groups at once, one independent matching per (group, area range, IoU threshold) cell (include/krrn_hip.h
// states the definition; tests/coco_ref.py restates it in numpy). Comparisons only: no arithmetic on the IoUs, the
// areas or the scores, no atomics, nothing that depends on an order between threads or blocks, so the result is
// bit-reproducible and a group's outputs do not depend on the rest of the batch. One launch, one block per group,
// built from krrn_match.h:
//   1. the block reads its ranges (match_group), ranks the group's detections into LDS by counting (match_rank: a
//      higher score, or the same score and a lower index, precedes; a NaN score counts as -inf) and stores `rank`;
//      the ground truths' flags and areas go to LDS.
//   2. every owned (ground truth, area range) element of gt_ig is stored from global memory by the threads in stride.
//   3. the threads stride over the group's A * T cells, consecutive lanes taking consecutive thresholds of one area
//      range. A cell holds three Bits128 sets (ignored, crowd, matched). COCO walks the ground truths "non-ignored
//      first, then ignored" and stops at the first ignored one once it holds a non-ignored match: that is one pass
//      over the non-ignored j and, only if it matched nothing, one pass over the ignored j. The lanes that share a
//      detection read the same iou element (a broadcast), and their dt_match / dt_ig stores are contiguous.
// Every (detection, cell) element is stored exactly once: by the walk for the first min(n_det, max_det) detections
// in rank order, as (-1, 1) for the rest. A group whose ranges break a stated limit is matched as an empty one: the
// detections and ground truths its ranges own inside the buffers get rank -1, (-1, 1) and their gt_ig.
#include "krrn_match.h"

namespace {

constexpr int kCocoThreads = kMatchThreads;
constexpr int kCocoMaxA = 8;
constexpr int kCocoMaxT = 16;

__global__ __launch_bounds__(kCocoThreads) void coco_match_kernel(
    const double* __restrict__ score, int Dtot, const int* __restrict__ det_range, const int* __restrict__ gt_range,
    const int* __restrict__ pair_off, const double* __restrict__ iou, long long Ptot,
    const double* __restrict__ det_area, const double* __restrict__ gt_area, const int* __restrict__ gt_flags, int GTtot,
    const double* __restrict__ area_rng, int A, const double* __restrict__ iou_thr, int T, int max_det, int lim_det,
    int lim_gt, int* __restrict__ dt_match, unsigned char* __restrict__ dt_ig, unsigned char* __restrict__ gt_ig,
    int* __restrict__ rank) {
  __shared__ double s_score[kMatchMax];
  __shared__ int s_order[kMatchMax];
  __shared__ double s_garea[kMatchMax];
  __shared__ int s_gflag[kMatchMax];
  const int g = blockIdx.x, tid = threadIdx.x;
  const MatchGroup grp = match_group(det_range, gt_range, pair_off, g, Dtot, GTtot, lim_det, lim_gt, Ptot);
  const int d0 = grp.a0, g0 = grp.b0;
  const long long p0 = grp.p0;
  const bool ok = grp.ok;
  // both sides have output rows here: the detections' rank / dt_match / dt_ig and the ground truths' gt_ig
  const int nd_own = grp.na_own, ng_own = grp.nb_own;
  const int n_det = ok ? grp.na : 0, n_gt = ok ? grp.nb : 0;
  const int n_use = min(n_det, max_det);
  const int cells = A * T;

  if (tid < n_gt) s_garea[tid] = gt_area[g0 + tid], s_gflag[tid] = gt_flags[g0 + tid];
  const int r = match_rank(score, d0, n_det, s_score, s_order);
  if (tid < n_det) rank[d0 + tid] = r < max_det ? r : -1;
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
    Bits128 ignored, crowd, matched;
    for (int j = 0; j < n_gt; ++j) {
      const double ar = s_garea[j];
      const int f = s_gflag[j];
      if (f != 0 || ar < lo || ar > hi) ignored.set(j);
      if (f & 1) crowd.set(j);
    }
    for (int r = 0; r < n_use; ++r) {
      const int d = s_order[r];
      const double* row = iou + (size_t)p0 + (size_t)d * n_gt;
      double best = thr;
      int m = -1;
      for (int pass = 0; pass < 2 && m < 0; ++pass) {  // the non-ignored ground truths, then the ignored ones
        for (int j = 0; j < n_gt; ++j) {
          if (ignored.test(j) != (pass == 1)) continue;
          if (matched.test(j) && !crowd.test(j)) continue;
          const double v = row[j];
          if (!(v >= best)) continue;  // below the best so far, or NaN
          best = v, m = j;
        }
      }
      const size_t out = (size_t)(d0 + d) * cells + cell;
      if (m >= 0) {
        matched.set(m);
        dt_match[out] = g0 + m;
        dt_ig[out] = ignored.test(m) ? 1 : 0;
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
      T > kCocoMaxT || max_det < 0 || max_det > kMatchMax || lim_det < 0 || lim_det > kMatchMax || lim_gt < 0 ||
      lim_gt > kMatchMax)
    return KRRN_ESHAPE;
  if (G == 0) return KRRN_OK;
  hipLaunchKernelGGL(coco_match_kernel, dim3(G), dim3(kCocoThreads), 0, (hipStream_t)stream, score, Dtot, det_range,
                     gt_range, pair_off, iou, Ptot, det_area, gt_area, gt_flags, GTtot, area_rng, A, iou_thr, T,
                     max_det, lim_det, lim_gt, dt_match, dt_ig, gt_ig, rank);
  return krrn_launch_status();
}
