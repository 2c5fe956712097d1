// The counter-based generator of the device draws, stated once: csrc/rng.hip (permutations, RANSAC subsets) and
// csrc/surface.hip (surface samples) draw from it, and tests/draws_ref.py restates it in numpy.uint64.
// Value number i of (seed, stream, row) is the high half of a splitmix64 step of a per-row base plus i; integer
// arithmetic modulo 2^64 only, so the bits are the same on every device and on the host.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned int rand32(unsigned long long seed, unsigned int stream, unsigned int row,
                                               unsigned int i) {
  const unsigned long long a = mix64(seed ^ (0xD1B54A32D192ED03ull * (stream + 1)));
  const unsigned long long b = mix64(a + 0x632BE59BD9B4E019ull * (row + 1));
  return (unsigned int)(mix64(b + i) >> 32);
}
