// Batched point-to-point ICP: a pose (R, t), model -> camera, polished against the crop's depth cloud.
// The reference project has no ICP; the definition is this project's own (DESIGN.md section 3,
// tests/icp_ref.py is its numpy restatement). Per crop, with R, t starting at R0, t0, pass k = 0, 1, ...:
//
//   q_i  = R^T (p_i - t)                                  every cloud point in the object frame
//   j(i) = argmin_j |q_i - m_j|^2, d^2 = (dx dx + dy dy) + dz dz, the lowest j among equal distances
//   pair i kept iff d_i^2 < max_dist^2; K = #kept, err_k = sum of kept d_i^2 / K
//   stop:  K < min_pairs -> STARVED;  k >= 1 and |err_{k-1} - err_k| <= tol err_{k-1} -> CONVERGED;
//          k == max_iter -> MAX_ITER                      (in this order; R, t are the result)
//   else:  Kabsch on the kept pairs m_j(i) -> p_i: centroids, Cov = sum (p - mp)(m - mm)^T / K (two-pass),
//          R = U diag(1, 1, sign) V^T (umeyama_solve's R), t = mp - R mm; a non-finite R or t keeps the
//          pose from before the update and stops with DEGENERATE.
//
// All arithmetic in f64 on the f32 inputs, built without FMA contraction (the two fma() of the distance
// are written out). One block of 512 threads per crop and the whole loop in one launch: the model
// points staged once in LDS (f32), thread `tid` owns the cloud points i = tid + s * 512 in registers and
// walks all M model points for them (every lane reads the same LDS address: a broadcast), keeping its
// own best (d^2, j). Counts, err, centroids and covariance: per-thread partials in increasing i, a wave
// butterfly, then the 8 waves in order (block_sum). No atomics; a block reads its own crop only and
// waits for no other block; every loop is bounded by max_iter <= 64 and M, N <= 4096.
#include <math.h>

#include "krrn_common.h"
#include "krrn_sim3.h"

namespace {

constexpr int kIcpMaxN = 4096;
constexpr int kIcpMaxM = 4096;
constexpr int kIcpMaxIter = 64;
constexpr int kIcpThreads = 512;
constexpr int kIcpWaves = kIcpThreads / 64;
constexpr int kIcpSlots = kIcpMaxN / kIcpThreads;  // cloud points per thread at N = 4096
constexpr int kIcpRedBytes = kIcpWaves * 9 * (int)sizeof(double);  // block_sum's workspace, a multiple of 16

enum { ICP_CONVERGED = 0, ICP_MAX_ITER = 1, ICP_STARVED = 2, ICP_DEGENERATE = 3 };

// nearest model point of the thread's first P cloud points q (a NaN q never wins: d^2 = inf, j = -1; nor does a
// non-finite model point: its d^2 is NaN or inf, and `<` is strict and false for NaN)
template <int P>
__device__ __forceinline__ void icp_nearest(const float* sm, int M, const double (&q)[kIcpSlots][3],
                                            double (&bd)[kIcpSlots], int (&bj)[kIcpSlots]) {
#pragma unroll 4
  for (int j = 0; j < M; ++j) {
    const double mx = (double)sm[3 * j], my = (double)sm[3 * j + 1], mz = (double)sm[3 * j + 2];
#pragma unroll
    for (int s = 0; s < P; ++s) {
      const double dx = q[s][0] - mx, dy = q[s][1] - my, dz = q[s][2] - mz;
      const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
      const bool lt = d2 < bd[s];  // strict: the lowest j keeps an exact tie
      bd[s] = lt ? d2 : bd[s];
      bj[s] = lt ? j : bj[s];
    }
  }
}

__device__ __forceinline__ bool icp_finite(double x) { return fabs(x) < INFINITY; }  // false for NaN

__global__ __launch_bounds__(kIcpThreads) void icp_refine_kernel(
    const float* __restrict__ R0, const float* __restrict__ t0, const float* __restrict__ cloud, int N,
    const float* __restrict__ model, int M, const float* __restrict__ max_dist, int max_iter, double tol,
    int min_pairs, float* __restrict__ Rout, float* __restrict__ tout, int* __restrict__ passes,
    int* __restrict__ pairs, float* __restrict__ rmse, int* __restrict__ status, int* __restrict__ nn_idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char icp_smem[];
  double* sred = reinterpret_cast<double*>(icp_smem);
  float* sm = reinterpret_cast<float*>(icp_smem + kIcpRedBytes);
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* mb = model + (long long)b * M * 3;
  const float* cb = cloud + (long long)b * N * 3;
  for (int i = tid; i < 3 * M; i += kIcpThreads) sm[i] = mb[i];
  float p[kIcpSlots][3];
#pragma unroll
  for (int s = 0; s < kIcpSlots; ++s) {
    const int i = tid + s * kIcpThreads;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[s][k] = i < N ? cb[3 * i + k] : NAN;  // a slot past N pairs with nothing
  }
  double R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = (double)R0[9 * b + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = (double)t0[3 * b + i];
  const double md = (double)max_dist[b];
  const double md2 = md * md;
  const int slots = krrn_cdiv(N, kIcpThreads);
  __syncthreads();

  double err_prev = 0.0;
  for (int k = 0; k <= max_iter; ++k) {
    double q[kIcpSlots][3], bd[kIcpSlots];
    int bj[kIcpSlots];
#pragma unroll
    for (int s = 0; s < kIcpSlots; ++s) {
      const double x = (double)p[s][0] - t[0], y = (double)p[s][1] - t[1], z = (double)p[s][2] - t[2];
      q[s][0] = R[0] * x + R[3] * y + R[6] * z;
      q[s][1] = R[1] * x + R[4] * y + R[7] * z;
      q[s][2] = R[2] * x + R[5] * y + R[8] * z;
      bd[s] = INFINITY;
      bj[s] = -1;
    }
    switch (slots) {  // block-uniform; the point arrays keep compile-time indices
      case 1: icp_nearest<1>(sm, M, q, bd, bj); break;
      case 2: icp_nearest<2>(sm, M, q, bd, bj); break;
      case 3: icp_nearest<3>(sm, M, q, bd, bj); break;
      case 4: icp_nearest<4>(sm, M, q, bd, bj); break;
      case 5: icp_nearest<5>(sm, M, q, bd, bj); break;
      case 6: icp_nearest<6>(sm, M, q, bd, bj); break;
      case 7: icp_nearest<7>(sm, M, q, bd, bj); break;
      default: icp_nearest<8>(sm, M, q, bd, bj); break;
    }
    // count, err and the centroids of the kept pairs (a kept pair has 0 <= j < M)
    bool keep[kIcpSlots];
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < kIcpSlots; ++s) {
      keep[s] = bd[s] < md2;  // strict; false for NaN
      if (keep[s]) {
        a[0] += 1.0;
        a[1] += bd[s];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          a[2 + c] += (double)sm[3 * bj[s] + c];
          a[5 + c] += (double)p[s][c];
        }
      }
    }
    block_sum<8, kIcpWaves>(a, sred);
    const double K = a[0];
    const double err = a[1] / K;
    int st = -1;
    if (K < (double)min_pairs) st = ICP_STARVED;
    else if (k >= 1 && fabs(err_prev - err) <= tol * err_prev) st = ICP_CONVERGED;
    else if (k == max_iter) st = ICP_MAX_ITER;
    double Rn[9], tn[3];
    if (st < 0) {
      double mm[3], mp[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        mm[c] = a[2 + c] / K;
        mp[c] = a[5 + c] / K;
      }
      double cv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < kIcpSlots; ++s) {
        if (!keep[s]) continue;
        double dm[3], dp[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          dm[c] = (double)sm[3 * bj[s] + c] - mm[c];
          dp[c] = (double)p[s][c] - mp[c];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) cv[3 * r + c] += dp[r] * dm[c];
      }
      block_sum<9, kIcpWaves>(cv, sred);
      double Cov[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) Cov[i] = cv[i] / K;
      Sim sim;
      umeyama_solve(mm, mp, Cov, 1.0, sim);  // its R only (the scale and its t are not used)
      bool ok = true;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        Rn[i] = sim.R[i];
        ok &= icp_finite(Rn[i]);
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        tn[r] = mp[r] - (Rn[3 * r] * mm[0] + Rn[3 * r + 1] * mm[1] + Rn[3 * r + 2] * mm[2]);
        ok &= icp_finite(tn[r]);
      }
      if (!ok) st = ICP_DEGENERATE;
    }
    if (st >= 0) {  // block-uniform: every thread holds the same sums
      if (tid == 0) {
        // a stop in pass 0 hands the input back bit for bit (a NaN's payload included)
        for (int i = 0; i < 9; ++i) Rout[9 * b + i] = k == 0 ? R0[9 * b + i] : (float)R[i];
        for (int i = 0; i < 3; ++i) tout[3 * b + i] = k == 0 ? t0[3 * b + i] : (float)t[i];
        passes[b] = k + 1;
        pairs[b] = (int)K;
        rmse[b] = K > 0.0 ? (float)sqrt(err) : INFINITY;
        status[b] = st;
      }
      if (nn_idx) {
#pragma unroll
        for (int s = 0; s < kIcpSlots; ++s) {
          const int i = tid + s * kIcpThreads;
          if (i < N) nn_idx[(long long)b * N + i] = keep[s] ? bj[s] : -1;
        }
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rn[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = tn[i];
    err_prev = err;
  }
}

}  // namespace

KRRN_API int krrn_icp_refine_f32(const float* R0, const float* t0, const float* cloud, int N, const float* model,
                                 int M, const float* max_dist, int max_iter, double tol, int min_pairs, float* R,
                                 float* t, int* passes, int* pairs, float* rmse, int* status, int* nn_idx, int B,
                                 void* stream) {
  if (!R0 || !t0 || !cloud || !model || !max_dist || !R || !t || !passes || !pairs || !rmse || !status)
    return KRRN_EARG;
  if (N < 3 || N > kIcpMaxN || M < 1 || M > kIcpMaxM || max_iter < 0 || max_iter > kIcpMaxIter || min_pairs < 3 ||
      B < 1)
    return KRRN_ESHAPE;
  const size_t lds = (size_t)kIcpRedBytes + sizeof(float) * 3 * (size_t)M;  // <= 48.6 KiB
  hipLaunchKernelGGL(icp_refine_kernel, dim3(B), dim3(kIcpThreads), lds, (hipStream_t)stream, R0, t0, cloud, N, model,
                     M, max_dist, max_iter, tol, min_pairs, R, t, passes, pairs, rmse, status, nn_idx);
  return krrn_launch_status();
}
