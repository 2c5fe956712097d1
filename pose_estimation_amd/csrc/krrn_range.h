// The guard on a (first, count) range that lives in device memory, stated once for the kernels that take per-object
// vertex, face or symmetry ranges (csrc/models.hip, csrc/surface.hip).
#pragma once
#include <hip/hip_runtime.h>

// a (first, count) range of device memory: negative, longer than the caller's bound or reaching past `total` is an
// empty range (not cut: a range that leaves the array is the caller's mistake, and half an object has no diameter)
__device__ __forceinline__ void mod_range(const int* range, int o, int total, int bound, long long& first, int& count) {
  first = range[2 * o];
  const long long n = range[2 * o + 1];
  const bool ok = first >= 0 && n >= 0 && n <= bound && first + n <= total;
  count = ok ? (int)n : 0;
}
