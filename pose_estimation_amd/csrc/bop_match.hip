// krrn_bop_match_f64: the BOP toolkit's greedy match_poses for G (scene, image, object) targets at once, one
// independent matching per (group, error function, threshold of correctness) cell (include/krrn_hip.h states the
// definition; tests/bop_match_ref.py restates it in numpy). Comparisons only: no arithmetic on the errors or the
// scores, no atomics, nothing that depends on an order between threads or blocks, so the result is bit-reproducible
// and a group's outputs do not depend on the rest of the batch. One launch, one block per group:
//   1. the block ranks the group's estimates into LDS by counting: estimate e's rank is the number of estimates
//      that precede it (a higher score, or the same score and a lower index; a NaN score counts as -inf), and
//      s_order[rank] = e. At most 128 estimates: 128 threads each walk the 128 scores in LDS, no sort network.
//   2. the threads stride over the group's C * NT cells, consecutive lanes taking consecutive thresholds k of one
//      error function c. A cell walks the first n_top estimates in rank order and, per estimate, the group's
//      instances in index order, keeping the lowest error below the threshold (strict <, so an error tie keeps the
//      lowest instance and a NaN never matches). The instances already taken are 128 bits in two 64-bit scalars
//      (a per-lane array indexed by j would live in scratch). The lanes of a wave that share c read the same err
//      element (a broadcast), and their match / tp stores are contiguous.
// Every (instance, cell) element of `match` is stored exactly once: the estimate's index when the cell matches the
// instance, -1 in the cell's closing pass over the instances left over. A group whose ranges break a stated
// limit is matched as a group without estimates.
#include "krrn_common.h"

namespace {

constexpr int kMatchThreads = 256;
constexpr int kMatchMax = 128;   // estimates and instances per group
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
  const int e0 = est_range[2 * g], ne_in = est_range[2 * g + 1];
  const int g0 = gt_range[2 * g], ng_in = gt_range[2 * g + 1];
  const long long p0 = pair_off[g];
  // uniform over the block. The instances whose match rows this group owns: its range clipped to [0, GTtot)
  const bool gt_ok = g0 >= 0 && ng_in >= 0 && (long long)g0 + ng_in <= GTtot;
  const int n_own = gt_ok ? ng_in : 0;
  const bool ok = gt_ok && ng_in <= max_gt && e0 >= 0 && ne_in >= 0 && ne_in <= max_est &&
                  (long long)e0 + ne_in <= Etot && p0 >= 0 && p0 + (long long)ne_in * ng_in <= Ptot;
  const int n_est = ok ? ne_in : 0, n_gt = ok ? ng_in : 0;
  const int top = n_top[g];
  const int n_use = top <= 0 ? n_est : min(top, n_est);

  if (tid < n_est) {
    const double s = score[e0 + tid];
    s_score[tid] = s != s ? -INFINITY : s;
  }
  __syncthreads();
  if (tid < n_est) {
    const double s = s_score[tid];
    int rank = 0;
    for (int o = 0; o < n_est; ++o) {
      const double q = s_score[o];
      rank += (q > s || (q == s && o < tid)) ? 1 : 0;
    }
    s_order[rank] = tid;
  }
  __syncthreads();

  const int cells = C * NT;
  for (int cell = tid; cell < cells; cell += kMatchThreads) {
    const int c = cell / NT;
    const double t = thr[(size_t)g * cells + cell];
    unsigned long long m0 = 0ull, m1 = 0ull;  // instances 0..63 / 64..127 already matched
    int n_tp = 0;
    for (int r = 0; r < n_use; ++r) {
      const int e = s_order[r];
      const double* row = err + ((size_t)p0 + (size_t)e * n_gt) * C + c;
      double best = 0.0;
      int best_j = -1;
      for (int j = 0; j < n_gt; ++j) {
        const unsigned long long taken = ((j < 64 ? m0 : m1) >> (j & 63)) & 1ull;
        const double v = row[(size_t)j * C];
        if (!taken && v < t && (best_j < 0 || v < best)) best = v, best_j = j;
      }
      if (best_j >= 0) {
        const unsigned long long bit = 1ull << (best_j & 63);
        if (best_j < 64) m0 |= bit; else m1 |= bit;
        match[(size_t)(g0 + best_j) * cells + cell] = e0 + e;
        ++n_tp;
      }
    }
    for (int j = 0; j < n_own; ++j) {  // n_own == n_gt, or the group is matched as an empty one (m0 = m1 = 0)
      const unsigned long long taken = ((j < 64 ? m0 : m1) >> (j & 63)) & 1ull;
      if (j >= kMatchMax || !taken) match[(size_t)(g0 + j) * cells + cell] = -1;
    }
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
