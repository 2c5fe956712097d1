// The closed-form similarity fit of the 3D-3D pose kernels, stated once: umeyama.hip solves every
// hypothesis and every refit with it, icp.hip every Kabsch update (through krrn_sim3.h). f64 throughout.
// Self-contained: compiles as device code under hipcc and as plain host C++ (tests/sim3_host_main.cpp
// runs it on the CPU, tests/test_sim3_host.py holds it to a bound). Build without FMA contraction
// (-ffp-contract=off), as both kernels are: the same inputs then give the same bits everywhere.
//
// The 3x3 SVD is a one-sided (Hestenes) Jacobi: the columns of Cov are rotated until orthogonal,
// Cov V = [s1 u1, s2 u2, s3 u3]. Only u1 and u2 are normalised; the third direction is u3 = u1 x u2
// and the third singular value is signed, det(V) * (u3 . Cov v3): the reference's rule (det(U) det(Vh)
// < 0: negate D[-1] and U[:, -1]) without a division by a vanishing s3, so a rank-2 covariance (planar
// points) has a finite, proper rotation.
//
// A covariance of rank below 2 (exactly: the zero matrix, diag(1, 0, 0)) has no second direction:
// s2 = 0 (or s1 = s2 = 0), u2 = 0 / 0, and every entry of R, s and t come back NaN. The callers rest
// on that and test it: a hypothesis whose scale is not finite and positive counts 0 (umeyama.hip
// pass_thr2), an ICP update whose R or t is not finite stops with DEGENERATE and keeps the pose from
// before (icp.hip). Nothing here traps or reads out of bounds on such input; the loop is bounded by
// 30 sweeps.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KRRN_SIM3_FN __device__ __forceinline__
#else
#define KRRN_SIM3_FN static inline
#endif

namespace {

struct Sim {
  double s;      // scale (may be NaN / inf / <= 0: the caller checks)
  double R[9];   // rotation, row-major
  double sR[9];  // s * R
  double t[3];
};

// estimateSimilarityUmeyama (:67-98) from the centroids mS / mT, Cov = Tc Sc^T / n (row-major) and
// varP = sum of the per-axis population variances of the source points
KRRN_SIM3_FN void umeyama_solve(const double (&mS)[3], const double (&mT)[3], const double (&Cov)[9], double varP,
                                Sim& o) {
  double A[9], V[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    A[i] = Cov[i];
    V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool any = false;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        const double al = A[p] * A[p] + A[3 + p] * A[3 + p] + A[6 + p] * A[6 + p];
        const double be = A[q] * A[q] + A[3 + q] * A[3 + q] + A[6 + q] * A[6 + q];
        const double ga = A[p] * A[q] + A[3 + p] * A[3 + q] + A[6 + p] * A[6 + q];
        const bool rot = fabs(ga) > 1e-15 * sqrt(al * be) && fabs(ga) > 1e-300;
        any |= rot;
        const double zeta = (be - al) / (2.0 * (rot ? ga : 1.0));
        const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
        const double c = rot ? 1.0 / sqrt(tt * tt + 1.0) : 1.0;
        const double sn = rot ? tt * c : 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double ap = A[3 * r + p], aq = A[3 * r + q];
          A[3 * r + p] = c * ap - sn * aq;
          A[3 * r + q] = sn * ap + c * aq;
          const double vp = V[3 * r + p], vq = V[3 * r + q];
          V[3 * r + p] = c * vp - sn * vq;
          V[3 * r + q] = sn * vp + c * vq;
        }
      }
    }
    if (!any) break;
  }
  double n2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) n2[i] = A[i] * A[i] + A[3 + i] * A[3 + i] + A[6 + i] * A[6 + i];
  // columns in descending order of their norm (compare-exchange, every index compile-time)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = i + 1; j < 3; ++j) {
      const bool sw = n2[j] > n2[i];
      const double ni = n2[i], nj = n2[j];
      n2[i] = sw ? nj : ni;
      n2[j] = sw ? ni : nj;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double ai = A[3 * r + i], aj = A[3 * r + j];
        A[3 * r + i] = sw ? aj : ai;
        A[3 * r + j] = sw ? ai : aj;
        const double vi = V[3 * r + i], vj = V[3 * r + j];
        V[3 * r + i] = sw ? vj : vi;
        V[3 * r + j] = sw ? vi : vj;
      }
    }
  }
  const double s1 = sqrt(n2[0]), s2 = sqrt(n2[1]);
  double u1[3], u2[3], u3[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    u1[r] = A[3 * r] / s1;
    u2[r] = A[3 * r + 1] / s2;
  }
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
  u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
  u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  const double detV = V[0] * (V[4] * V[8] - V[5] * V[7]) - V[1] * (V[3] * V[8] - V[5] * V[6]) +
                      V[2] * (V[3] * V[7] - V[4] * V[6]);
  const double sg = detV < 0 ? -1.0 : 1.0;
  const double d3 = sg * (u3[0] * A[2] + u3[1] * A[5] + u3[2] * A[8]);  // signed third singular value
  const double sumD = s1 + s2 + d3;
  o.s = 1.0 / varP * sumD;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o.R[3 * j + k] = u1[j] * V[3 * k] + u2[j] * V[3 * k + 1] + sg * u3[j] * V[3 * k + 2];
      o.sR[3 * j + k] = o.s * o.R[3 * j + k];
    }
#pragma unroll
  for (int j = 0; j < 3; ++j)
    o.t[j] = mT[j] - (mS[0] * o.sR[3 * j] + mS[1] * o.sR[3 * j + 1] + mS[2] * o.sR[3 * j + 2]);
}

}  // namespace
