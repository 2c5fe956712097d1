// f64 building blocks shared by the 3D-3D pose kernels (umeyama.hip, icp.hip): fixed-order block sums
// and (krrn_umeyama.h, which also compiles on the host) the closed-form similarity fit with its 3x3
// one-sided Jacobi SVD. Both files are built without FMA contraction, so the same inputs give the same
// bits in either.
#pragma once
#include <math.h>

#include "krrn_common.h"
#include "krrn_umeyama.h"  // Sim, umeyama_solve

namespace {

__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const int lo = __shfl_xor((int)(unsigned)b, m), hi = __shfl_xor((int)(unsigned)(b >> 32), m);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// butterfly sum: the same bits in every lane (a + b == b + a)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += shfl_xor_f64(v, off);
  return v;
}

// v[k] <- sum over the block of W waves, fixed order (wave butterfly, then waves 0..W-1); sred: W * K doubles
template <int K, int W = 4>
__device__ __forceinline__ void block_sum(double (&v)[K], double* sred) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double x = wave_sum(v[k]);
    if (lane == 0) sred[w * K + k] = x;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double x = sred[k];
#pragma unroll
    for (int ww = 1; ww < W; ++ww) x += sred[ww * K + k];
    v[k] = x;
  }
  __syncthreads();
}

}  // namespace
