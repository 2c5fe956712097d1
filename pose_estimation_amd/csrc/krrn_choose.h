// The `choose` selection of the input kernels, stated once: inputs.hip's krrn_choose_points (crops at their own
// size) and krrn_choose_points_resize (crops resampled to one size) pick the same pixels of a u8 mask row through
// the one choose_points_kernel. One workgroup of kChooseThreads threads per
// crop: block-wide ballot scans keep the row-major order, and the random subset is the N smallest of per-rank
// 32-bit hash keys found by a 4-pass radix select (ties broken by rank), so no sort and no workspace. Integer and
// comparison code only, so the per-file -ffp-contract flags of the Makefile cannot change what a helper computes.
#pragma once
#include "krrn_common.h"

namespace {

constexpr int kChooseThreads = 1024;
constexpr int kChooseWaves = kChooseThreads / 64;
constexpr int kChooseStreamMax = 65534;

__device__ __forceinline__ unsigned mix32(unsigned long long x) {
  // splitmix64 finaliser, high half
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (unsigned)(x >> 32);
}

// the key base of crop b: rank r of its mask pixels gets the key mix32(base + r)
__device__ __forceinline__ unsigned long long choose_key_base(const long long* __restrict__ seed, int stream_id, int b) {
  return ((unsigned long long)seed[0] * 0x9E3779B97F4A7C15ull) ^ ((unsigned long long)(stream_id + 1) << 48) ^
         ((unsigned long long)b << 24);
}

// exclusive prefix of a 0/1 flag over the block (thread order), and the block total
__device__ __forceinline__ int block_excl_scan(bool flag, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(flag);
  const int in_wave = __popcll(bal & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) wsum[wave] = __popcll(bal);
  __syncthreads();
  int before = 0;
  total = 0;
  for (int w = 0; w < kChooseWaves; ++w) {
    const int v = wsum[w];
    before += (w < wave) ? v : 0;
    total += v;
  }
  return before + in_wave;
}

// The selection over one crop's mask mb[0 .. npix), by the whole block: returns the number of mask pixels (the
// same value in every thread) and, when there are any, fills cb[0 .. N) with the chosen pixel indices: all of them
// in row-major order, the N of smallest (key, rank) when there are more than N, wrap-padded when fewer. cb is
// complete and visible to every thread on return. An empty mask writes nothing.
__device__ __forceinline__ int choose_select(const unsigned char* __restrict__ mb, int npix, int N,
                                             unsigned long long base, long long* __restrict__ cb) {
  __shared__ int wsum[kChooseWaves];
  __shared__ int hist[256];
  __shared__ int sel_state[2];  // threshold key, ties to take
  const int tid = threadIdx.x;

  // pass A: number of mask pixels
  int count = 0;
  for (int p0 = 0; p0 < npix; p0 += kChooseThreads) {
    const int p = p0 + tid;
    int tot;
    block_excl_scan(p < npix && mb[p] != 0, wsum, tot);
    count += tot;
  }
  if (count == 0) return 0;

  // radix select: the N-th smallest key over ranks [0, count)
  unsigned thr = 0xFFFFFFFFu;
  int need = N;
  const bool subset = count > N;
  if (subset) {
    unsigned prefix = 0, pmask = 0;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      for (int i = tid; i < 256; i += kChooseThreads) hist[i] = 0;
      __syncthreads();
      for (int i = tid; i < count; i += kChooseThreads) {
        const unsigned k = mix32(base + (unsigned long long)i);
        if ((k & pmask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int acc = 0, d = 0;
        for (; d < 256; ++d) {
          if (acc + hist[d] >= need) break;
          acc += hist[d];
        }
        sel_state[0] = d;
        sel_state[1] = need - acc;
      }
      __syncthreads();
      prefix |= (unsigned)sel_state[0] << shift;
      pmask |= 255u << shift;
      need = sel_state[1];
      __syncthreads();
    }
    thr = prefix;  // keys < thr all taken, plus the first `need` ranks with key == thr
  }

  // pass B: selected mask pixels in row-major order
  int rank0 = 0, tie0 = 0, out0 = 0;
  for (int p0 = 0; p0 < npix; p0 += kChooseThreads) {
    const int p = p0 + tid;
    const bool m = p < npix && mb[p] != 0;
    int tot;
    const int r = rank0 + block_excl_scan(m, wsum, tot);
    rank0 += tot;
    bool take = m, tie = false;
    unsigned k = 0;
    if (subset && m) {
      k = mix32(base + (unsigned long long)r);
      take = k < thr;
      tie = k == thr;
    }
    int ttot;
    const int tr = tie0 + block_excl_scan(tie, wsum, ttot);
    tie0 += ttot;
    take = take || (tie && tr < need);
    int stot;
    const int slot = out0 + block_excl_scan(take, wsum, stot);
    out0 += stot;
    if (take && slot < N) cb[slot] = p;
  }
  __syncthreads();
  // wrap padding (np.pad(..., 'wrap')): slot j >= count repeats slot j % count
  for (int j = count + tid; j < N; j += kChooseThreads) cb[j] = cb[j % count];
  __syncthreads();
  return count;
}

// the outputs of a crop without a mask pixel (the reference drops such a sample, choose error, :679-681): zeros
__device__ __forceinline__ void choose_zero_outputs(int b, int N, long long* __restrict__ choose,
                                                    float* __restrict__ cloud, float* __restrict__ xmap,
                                                    float* __restrict__ ymap) {
  for (int j = threadIdx.x; j < N; j += kChooseThreads) {
    choose[(size_t)b * N + j] = 0;
    xmap[(size_t)b * N + j] = 0.f;
    ymap[(size_t)b * N + j] = 0.f;
    cloud[((size_t)b * N + j) * 3 + 0] = 0.f;
    cloud[((size_t)b * N + j) * 3 + 1] = 0.f;
    cloud[((size_t)b * N + j) * 3 + 2] = 0.f;
  }
}

}  // namespace
