// The building blocks of the two greedy matching kernels (bop_match.hip, coco_match.hip), stated once. One block of
// kMatchThreads threads per group; a group pairs side a (the scored rows that are ranked: estimates, detections)
// with side b (the ground truths), at most kMatchMax of each. Comparisons and integer code only, so a per-file
// -ffp-contract flag cannot change what a helper computes. Every helper is __device__ __forceinline__.
#pragma once
#include "krrn_common.h"

namespace {

constexpr int kMatchThreads = 256;
constexpr int kMatchMax = 128;  // rows per side and group: the LDS arrays below, the bits of a Bits128
static_assert(kMatchMax <= kMatchThreads, "one thread ranks one row");

// A set of j in [0, kMatchMax) in two 64-bit scalars: a per-lane array indexed by j would live in scratch.
struct Bits128 {
  unsigned long long lo = 0ull, hi = 0ull;
  __device__ __forceinline__ bool test(int j) const { return ((j < 64 ? lo : hi) >> (j & 63)) & 1ull; }
  __device__ __forceinline__ void set(int j) {
    const unsigned long long bit = 1ull << (j & 63);
    if (j < 64) lo |= bit; else hi |= bit;
  }
};

// One group's ranges as given, (first, count) of each side and the offset of its na x nb pair block. A side is owned
// when its range lies inside its buffer [0, tot): the group stores the output rows of an owned side whatever else
// is wrong. `ok`: both owned, neither count past its limit, the pair block inside [0, Ptot); a group that is not ok
// is matched as an empty one. Uniform over the block.
struct MatchGroup {
  int a0, na, b0, nb;  // as given
  int na_own, nb_own;  // na / nb where the side is owned, else 0
  long long p0;
  bool ok;
};

__device__ __forceinline__ MatchGroup match_group(const int* __restrict__ a_range, const int* __restrict__ b_range,
                                                  const int* __restrict__ pair_off, int g, int a_tot, int b_tot,
                                                  int a_lim, int b_lim, long long Ptot) {
  MatchGroup m;
  m.a0 = a_range[2 * g], m.na = a_range[2 * g + 1];
  m.b0 = b_range[2 * g], m.nb = b_range[2 * g + 1];
  m.p0 = pair_off[g];
  const bool a_own = m.a0 >= 0 && m.na >= 0 && (long long)m.a0 + m.na <= a_tot;
  const bool b_own = m.b0 >= 0 && m.nb >= 0 && (long long)m.b0 + m.nb <= b_tot;
  m.na_own = a_own ? m.na : 0, m.nb_own = b_own ? m.nb : 0;
  m.ok = a_own && b_own && m.na <= a_lim && m.nb <= b_lim && m.p0 >= 0 && m.p0 + (long long)m.na * m.nb <= Ptot;
  return m;
}

// Rank by counting: row i of score[first .. first + n), n <= kMatchMax, precedes row o when its score is higher, or
// the same and i < o; a NaN score counts as -inf. Thread i < n walks the n scores in LDS (no sort network), stores
// s_order[rank] = i and returns its rank; the other threads return -1. One barrier inside, after the scores (and
// whatever the caller put into LDS before the call) are stored; the caller adds the one before s_order is read.
__device__ __forceinline__ int match_rank(const double* __restrict__ score, int first, int n, double* s_score,
                                          int* s_order) {
  const int tid = threadIdx.x;
  if (tid < n) {
    const double s = score[first + tid];
    s_score[tid] = s != s ? -INFINITY : s;
  }
  __syncthreads();
  int rank = -1;
  if (tid < n) {
    const double s = s_score[tid];
    rank = 0;
    for (int o = 0; o < n; ++o) {
      const double q = s_score[o];
      rank += (q > s || (q == s && o < tid)) ? 1 : 0;
    }
    s_order[rank] = tid;
  }
  return rank;
}

}  // namespace
