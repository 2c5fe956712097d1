// The SO(3) log map of an f32 rotation matrix, stated once: csrc/bpnp.hip turns the RANSAC
// rotation into the angle-axis start of its Levenberg-Marquardt with it. f64 arithmetic on the
// f32 entries. Self-contained: compiles as device code under hipcc and as plain host C++
// (tests/so3_host_main.cpp runs it on the CPU, tests/test_so3_host.py holds it to a bound).
//
// An f32 matrix carries about 1e-7 of rounding per entry. Near theta = pi the trace is flat in
// theta (d cos = -sin d theta), so an angle taken from acos of the trace alone is off by about
// sqrt(2e-7) there while the skew part v = 2 sin(theta) n is still exact; a branch chosen from
// sin(acos(c)) then pairs a wrong angle with a right v. Here no branch rests on the trace alone:
//   theta = atan2(|v| / 2, c): well conditioned everywhere (near 0 and pi it follows |v|, near
//           pi / 2 it follows c);
//   axis  = v / |v| while c >= -0.5 (|v| / 2 >= 0.86 there unless theta is small, and for small
//           theta w = theta / (|v| / 2) * v / 2 -> v / 2 smoothly, |v| = 0 included);
//           for c < -0.5 (theta > 120 deg) from the symmetric part (R + R^T) / 2 = c I +
//           (1 - c) n n^T: the column of the largest diagonal entry (n_k^2 >= 1/3), normalised,
//           its sign from v (any sign is the same rotation where v = 0, theta = pi exactly).
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KRRN_SO3_FN __host__ __device__ inline
#else
#define KRRN_SO3_FN static inline
#endif

// Rf: row-major [3][3]; w: the angle-axis vector, |w| in [0, pi]
KRRN_SO3_FN void krrn_rot_log(const float* Rf, double (&w)[3]) {
  double R[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) R[a][b] = (double)Rf[3 * a + b];
  const double c = (R[0][0] + R[1][1] + R[2][2] - 1.0) * 0.5;
  const double v[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};
  const double sn = 0.5 * sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double th = atan2(sn, c);
  if (c >= -0.5) {
    const double f = sn > 0.0 ? th / (2.0 * sn) : 0.5;
    for (int a = 0; a < 3; ++a) w[a] = f * v[a];
    return;
  }
  int k = 0;
  for (int a = 1; a < 3; ++a)
    if (R[a][a] > R[k][k]) k = a;
  double n[3];
  // column k of (R + R^T) / 2 - c I = (1 - c) n_k n: only its direction is used
  for (int a = 0; a < 3; ++a) n[a] = 0.5 * (R[a][k] + R[k][a]) - (a == k ? c : 0.0);
  const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  const double sg = (n[0] * v[0] + n[1] * v[1] + n[2] * v[2]) < 0.0 ? -1.0 : 1.0;
  for (int a = 0; a < 3; ++a) w[a] = sg * th * n[a] / nn;
}
