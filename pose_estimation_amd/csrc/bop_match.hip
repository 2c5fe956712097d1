// krrn_bop_match_f64: the BOP toolkit's greedy match_poses for G (scene, image, object) targets at once, one
// independent matching per (group, error function, threshold of correctness) cell (include/krrn_hip.h states the
// definition; tests/bop_match_ref.py restates it in numpy). Comparisons only: no arithmetic on the errors or the
// scores, no atomics, nothing that depends on an order between threads or blocks, so the result is bit-reproducible
// and a group's outputs do not depend on the rest of the batch. One launch, one block per group:
//   1. the block reads its ranges (match_group of krrn_match.h) and ranks the group's estimates into LDS by
//      counting (match_rank: a higher score, or the same score and a lower index, precedes; a NaN score counts as
//      -inf), s_order[rank] = e.
//   2. the threads stride over the group's C * NT cells, consecutive lanes taking consecutive thresholds k of one
//      error function c. A cell walks the first n_top estimates in rank order and, per estimate, the group's
//      instances in index order, keeping the lowest error below the threshold (strict <, so an error tie keeps the
//      lowest instance and a NaN never matches). The instances already taken are a Bits128. The lanes of a wave
//      that share c read the same err element (a broadcast), and their match / tp stores are contiguous.
// Every (instance, cell) element of `match` is stored exactly once: the estimate's index when the cell matches the
// instance, -1 in the cell's closing pass over the instances left over. A group whose ranges break a stated
// limit is matched as a group without estimates.
#include "krrn_match.h"

namespace {

constexpr int kMatchMaxC = 18;   // kBopMaxT + 2 error functions
constexpr int kMatchMaxNT = 16;  // thresholds of correctness

__global__ __launch_bounds__(kMatchThreads) void bop_match_kernel(
    const double* __restrict__ score, int Etot, const double* __restrict__ err, long long Ptot,
    const int* __restrict__ est_range, const int* __restrict__ gt_range, const int* __restrict__ pair_off,
    const double* __restrict__ thr, const int* __restrict__ n_top, int GTtot, int C, int NT, int max_est, int max_gt,
    int* __restrict__ match, int* __restrict__ tp) {
  __shared__ double s_score[kMatchMax];
  __shared__ int s_order[kMatchMax];
  const int g = blockIdx.x, tid = threadIdx.x;
  const MatchGroup grp = match_group(est_range, gt_range, pair_off, g, Etot, GTtot, max_est, max_gt, Ptot);
  const int e0 = grp.a0, g0 = grp.b0;
  const long long p0 = grp.p0;
  const int n_own = grp.nb_own;  // only the instances have output rows here: the match rows this group must store
  const int n_est = grp.ok ? grp.na : 0, n_gt = grp.ok ? grp.nb : 0;
  const int top = n_top[g];
  const int n_use = top <= 0 ? n_est : min(top, n_est);

  match_rank(score, e0, n_est, s_score, s_order);
  __syncthreads();

  const int cells = C * NT;
  for (int cell = tid; cell < cells; cell += kMatchThreads) {
    const int c = cell / NT;
    const double t = thr[(size_t)g * cells + cell];
    Bits128 taken;  // the instances already matched
    int n_tp = 0;
    for (int r = 0; r < n_use; ++r) {
      const int e = s_order[r];
      const double* row = err + ((size_t)p0 + (size_t)e * n_gt) * C + c;
      double best = 0.0;
      int best_j = -1;
      for (int j = 0; j < n_gt; ++j) {
        const double v = row[(size_t)j * C];
        if (!taken.test(j) && v < t && (best_j < 0 || v < best)) best = v, best_j = j;
      }
      if (best_j >= 0) {
        taken.set(best_j);
        match[(size_t)(g0 + best_j) * cells + cell] = e0 + e;
        ++n_tp;
      }
    }
    for (int j = 0; j < n_own; ++j)  // n_own == n_gt, or the group is matched as an empty one (nothing taken)
      if (j >= kMatchMax || !taken.test(j)) match[(size_t)(g0 + j) * cells + cell] = -1;
    tp[(size_t)g * cells + cell] = n_tp;
  }
}

}  // namespace

KRRN_API int krrn_bop_match_f64(const double* score, int Etot, const double* err, long long Ptot, int C,
                                const int* est_range, const int* gt_range, const int* pair_off, const double* thr,
                                int NT, const int* n_top, int G, int GTtot, int max_est, int max_gt, int* match,
                                int* tp, void* stream) {
  if (!est_range || !gt_range || !pair_off || !thr || !n_top || !tp) return KRRN_EARG;
  if ((!score && Etot > 0) || (!err && Ptot > 0) || (!match && GTtot > 0)) return KRRN_EARG;
  if (G < 0 || Etot < 0 || GTtot < 0 || Ptot < 0 || Ptot > 0x7fffffffll || C < 3 || C > kMatchMaxC || NT < 1 ||
      NT > kMatchMaxNT || max_est < 0 || max_est > kMatchMax || max_gt < 0 || max_gt > kMatchMax)
    return KRRN_ESHAPE;
  if (G == 0) return KRRN_OK;
  hipLaunchKernelGGL(bop_match_kernel, dim3(G), dim3(kMatchThreads), 0, (hipStream_t)stream, score, Etot, err, Ptot,
                     est_range, gt_range, pair_off, thr, n_top, GTtot, C, NT, max_est, max_gt, match, tp);
  return krrn_launch_status();
}
