// Batched Umeyama-RANSAC on 3D-3D correspondences: estimateSimilarityTransform
// (lib/transform/umeyama.py:8-98) as tools/script/eval.py:128,151 calls it on
// (model coordinates of the chosen pixels, cloud).
//
//   InlierT = inlier_frac * 2 * max_i |src_i - mean(src)|                       (:16-20)
//   hypothesis h: Umeyama on the 5 pairs subsets[b][h] (:67-98) -> (s, R, t);
//     count_h = #{ i : |dst_i - (s R src_i + t)| < s InlierT }                  (:33-38)
//   selection: the reference's loop over h in order on the counts scored in parallel: a strictly
//     larger count becomes the best; stop after iteration i once 1 - (1 - best^5)^i > conf (:41-49)
//   best < min_ratio: failure (the reference's None, :50-52) -> scale 1, R = I, t = 0, inliers 0
//   refit: Umeyama on every inlier of the best hypothesis (:54-56)
//
// All arithmetic in f64 on the f32 inputs (numpy promotes the reference's hstack([source, ones])),
// built without FMA contraction. Two launches:
//   ume_score_kernel   grid (B, ceil(H / 64)), 4 waves: the crop's points staged once in LDS (f32);
//                      a wave solves 16 hypotheses, one per lane of a 16-lane group, the 3x3 matrices
//                      in registers (compile-time indices only), then scores them one after the other
//                      with its lanes striding over the LDS points and one wave reduction per count.
//   ume_refit_kernel   one block per crop: the selection loop (one thread, counts in LDS), the best
//                      hypothesis solved again (the same code, so the same bits), and the inlier sums
//                      reduced in a fixed order: per-thread strided partials, a wave butterfly, then
//                      the 4 waves in order. No atomics; a crop never reads another crop's data.
//
// The 3x3 SVD is a one-sided (Hestenes) Jacobi: the columns of Cov are rotated until orthogonal,
// Cov V = [s1 u1, s2 u2, s3 u3]. Only u1 and u2 are normalised; the third direction is
// u3 = u1 x u2 and the signed third singular value det(V) * (u3 . Cov v3), which is what the
// reference's rule (det(U) det(Vh) < 0: negate D[-1] and U[:, -1]) yields, without dividing by a
// vanishing s3 (planar model points give rank-2 covariances).
#include <math.h>

#include "krrn_common.h"
#include "krrn_sim3.h"  // shfl_xor_f64, wave_sum, block_sum, Sim, umeyama_solve

namespace {

constexpr int kUmeMaxN = 4096;
constexpr int kUmeMaxH = 8192;
constexpr int kUmeThreads = 256;
constexpr int kUmeWaves = kUmeThreads / 64;
constexpr int kUmeHypPerWave = 16;
constexpr int kUmeHypPerBlock = kUmeHypPerWave * kUmeWaves;

// Umeyama on the 5 sampled pairs (indices clamped into [0, N): a bad index never leaves the crop)
__device__ __forceinline__ void hyp_solve(const float* sp, const float* dp, const int* ids, int N, Sim& o) {
  double S[5][3], T[5][3];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    int id = ids[i];
    id = id < 0 ? 0 : (id > N - 1 ? N - 1 : id);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      S[i][k] = (double)sp[3 * id + k];
      T[i][k] = (double)dp[3 * id + k];
    }
  }
  double mS[3], mT[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mS[k] = (S[0][k] + S[1][k] + S[2][k] + S[3][k] + S[4][k]) / 5.0;
    mT[k] = (T[0][k] + T[1][k] + T[2][k] + T[3][k] + T[4][k]) / 5.0;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      S[i][k] -= mS[k];
      T[i][k] -= mT[k];
    }
  double Cov[9], varP = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < 5; ++i) a += T[i][j] * S[i][k];
      Cov[3 * j + k] = a / 5.0;
    }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) a += S[i][k] * S[i][k];
    varP += a / 5.0;
  }
  umeyama_solve(mS, mT, Cov, varP, o);
}

// (s InlierT)^2, or -1 (nothing passes) for a scale that is not finite and positive
__device__ __forceinline__ double pass_thr2(double s, double inlierT) {
  const bool ok = s > 0.0 && s < INFINITY;
  const double th = s * inlierT;
  return ok ? th * th : -1.0;
}

// |dst - (sR src + t)|^2 < thr2 (strict; false for NaN)
__device__ __forceinline__ bool ume_inlier(const double* sR, const double* t, double thr2, const float* s,
                                           const float* d) {
  const double x = (double)s[0], y = (double)s[1], z = (double)s[2];
  const double dx = (double)d[0] - (sR[0] * x + sR[1] * y + sR[2] * z + t[0]);
  const double dy = (double)d[1] - (sR[3] * x + sR[4] * y + sR[5] * z + t[1]);
  const double dz = (double)d[2] - (sR[6] * x + sR[7] * y + sR[8] * z + t[2]);
  return dx * dx + dy * dy + dz * dz < thr2;
}

// Stage crop b's points in LDS and return InlierT (the same bits in every thread and in both kernels)
__device__ __forceinline__ double stage_points(const float* __restrict__ src, const float* __restrict__ dst, int b,
                                               int N, double inlier_frac, float* sp, float* dp, double* sred) {
  const float* s = src + (long long)b * N * 3;
  const float* d = dst + (long long)b * N * 3;
  for (int i = threadIdx.x; i < 3 * N; i += kUmeThreads) {
    sp[i] = s[i];
    dp[i] = d[i];
  }
  __syncthreads();
  double m[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < N; i += kUmeThreads) {
    m[0] += (double)sp[3 * i];
    m[1] += (double)sp[3 * i + 1];
    m[2] += (double)sp[3 * i + 2];
  }
  block_sum(m, sred);
#pragma unroll
  for (int k = 0; k < 3; ++k) m[k] /= (double)N;
  double r2 = 0.0;
  for (int i = threadIdx.x; i < N; i += kUmeThreads) {
    const double x = (double)sp[3 * i] - m[0], y = (double)sp[3 * i + 1] - m[1], z = (double)sp[3 * i + 2] - m[2];
    r2 = fmax(r2, x * x + y * y + z * z);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) r2 = fmax(r2, shfl_xor_f64(r2, off));
  if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = r2;
  __syncthreads();
  r2 = sred[0];
#pragma unroll
  for (int w = 1; w < kUmeWaves; ++w) r2 = fmax(r2, sred[w]);
  __syncthreads();
  return 2.0 * sqrt(r2) * inlier_frac;
}

__global__ __launch_bounds__(kUmeThreads) void ume_score_kernel(const float* __restrict__ src,
                                                                const float* __restrict__ dst, int N,
                                                                const int* __restrict__ subsets, int H,
                                                                double inlier_frac, int* __restrict__ hyp_counts) {
  extern __shared__ float ume_pts[];
  __shared__ double sred[kUmeWaves * 12];
  __shared__ double shyp[kUmeWaves][kUmeHypPerWave][13];
  float* sp = ume_pts;
  float* dp = ume_pts + 3 * N;
  const int b = blockIdx.x;
  const double inlierT = stage_points(src, dst, b, N, inlier_frac, sp, dp, sred);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane & (kUmeHypPerWave - 1);
  const int h0 = blockIdx.y * kUmeHypPerBlock + w * kUmeHypPerWave;
  const int h = h0 + g;
  const int hs = h < H ? h : H - 1;  // a tail lane solves a duplicate, nothing of it is read
  {
    int ids[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) ids[i] = subsets[((long long)b * H + hs) * 5 + i];
    Sim sim;
    hyp_solve(sp, dp, ids, N, sim);
    if (lane < kUmeHypPerWave) {
      double* o = shyp[w][g];
#pragma unroll
      for (int i = 0; i < 9; ++i) o[i] = sim.sR[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) o[9 + i] = sim.t[i];
      o[12] = pass_thr2(sim.s, inlierT);
    }
  }
  __syncthreads();
  for (int j = 0; j < kUmeHypPerWave && h0 + j < H; ++j) {
    double p[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) p[i] = shyp[w][j][i];
    int cnt = 0;
    for (int i = lane; i < N; i += 64) cnt += ume_inlier(p, p + 9, p[12], sp + 3 * i, dp + 3 * i) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) hyp_counts[(long long)b * H + h0 + j] = cnt;
  }
}

__global__ __launch_bounds__(kUmeThreads) void ume_refit_kernel(
    const float* __restrict__ src, const float* __restrict__ dst, int N, const int* __restrict__ subsets, int H,
    double inlier_frac, double conf, double min_ratio, const int* __restrict__ hyp_counts, float* __restrict__ scale,
    float* __restrict__ Rout, float* __restrict__ tout, int* __restrict__ inliers, int* __restrict__ best_hyp,
    unsigned char* __restrict__ inlier_mask) {
  extern __shared__ float ume_pts[];
  __shared__ double sred[kUmeWaves * 12];
  __shared__ int ssel[2];
  float* sp = ume_pts;
  float* dp = ume_pts + 3 * N;
  int* scnt = reinterpret_cast<int*>(ume_pts + 6 * N);
  const int b = blockIdx.x;
  for (int i = threadIdx.x; i < H; i += kUmeThreads) scnt[i] = hyp_counts[(long long)b * H + i];
  const double inlierT = stage_points(src, dst, b, N, inlier_frac, sp, dp, sred);  // (barriers inside)
  if (threadIdx.x == 0) {
    // the reference's loop (:31-49) over the scored hypotheses
    int best_h = -1, best_cnt = 0;
    double r5 = 0.0;
    for (int i = 0; i < H; ++i) {
      const int c = scnt[i];
      if (c > best_cnt) {
        best_cnt = c;
        best_h = i;
        r5 = pow((double)c / (double)N, 5.0);
      }
      if (1.0 - pow(1.0 - r5, (double)i) > conf) break;
    }
    const bool ok = best_h >= 0 && !((double)best_cnt / (double)N < min_ratio);
    ssel[0] = ok ? best_h : -1;
    ssel[1] = ok ? best_cnt : 0;
  }
  __syncthreads();
  const int best_h = ssel[0];
  if (best_h < 0) {
    if (threadIdx.x == 0) {
      scale[b] = 1.f;
      for (int i = 0; i < 9; ++i) Rout[9 * b + i] = (i % 4 == 0) ? 1.f : 0.f;
      for (int i = 0; i < 3; ++i) tout[3 * b + i] = 0.f;
      inliers[b] = 0;
      if (best_hyp) best_hyp[b] = -1;
    }
    if (inlier_mask)
      for (int i = threadIdx.x; i < N; i += kUmeThreads) inlier_mask[(long long)b * N + i] = 0;
    return;
  }
  double hp[13];
  {
    int ids[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) ids[i] = subsets[((long long)b * H + best_h) * 5 + i];
    Sim sim;
    hyp_solve(sp, dp, ids, N, sim);
#pragma unroll
    for (int i = 0; i < 9; ++i) hp[i] = sim.sR[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) hp[9 + i] = sim.t[i];
    hp[12] = pass_thr2(sim.s, inlierT);
  }
  // pass 1: inlier count and centroids
  double a[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < N; i += kUmeThreads) {
    const bool in = ume_inlier(hp, hp + 9, hp[12], sp + 3 * i, dp + 3 * i);
    if (inlier_mask) inlier_mask[(long long)b * N + i] = in ? 1 : 0;
    if (in) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a[k] += (double)sp[3 * i + k];
        a[3 + k] += (double)dp[3 * i + k];
      }
      a[6] += 1.0;
    }
  }
  block_sum(a, sred);
  const double n = a[6];
  double mS[3], mT[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mS[k] = a[k] / n;
    mT[k] = a[3 + k] / n;
  }
  // pass 2: covariance and source variance
  double c[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < N; i += kUmeThreads) {
    if (!ume_inlier(hp, hp + 9, hp[12], sp + 3 * i, dp + 3 * i)) continue;
    double S[3], T[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      S[k] = (double)sp[3 * i + k] - mS[k];
      T[k] = (double)dp[3 * i + k] - mT[k];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) c[3 * j + k] += T[j] * S[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[9 + k] += S[k] * S[k];
  }
  block_sum(c, sred);
  double Cov[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Cov[i] = c[i] / n;
  const double varP = c[9] / n + c[10] / n + c[11] / n;
  Sim sim;
  umeyama_solve(mS, mT, Cov, varP, sim);
  if (threadIdx.x == 0) {
    scale[b] = (float)sim.s;
#pragma unroll
    for (int i = 0; i < 9; ++i) Rout[9 * b + i] = (float)sim.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tout[3 * b + i] = (float)sim.t[i];
    inliers[b] = ssel[1];
    if (best_hyp) best_hyp[b] = best_h;
  }
}

__global__ void model_points_kernel(const float* __restrict__ xyz, int HW, const long long* __restrict__ choose, int N,
                                    const double* __restrict__ extent, const double* __restrict__ lfb,
                                    float* __restrict__ out, int total) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int b = e / N;
  const long long pix = choose[e];
  const bool ok = pix >= 0 && pix < HW;  // a pixel outside the map is never read: NaN
  const float* xb = xyz + (long long)b * 3 * HW + (ok ? pix : 0);
#pragma unroll
  for (int k = 0; k < 3; ++k)
    out[3LL * e + k] = ok ? (float)((double)xb[(long long)k * HW] * extent[3 * b + k] + lfb[3 * b + k]) : NAN;
}

}  // namespace

KRRN_API int krrn_model_points_f32(const float* xyz, int HW, const long long* choose, int N, const double* extent,
                                   const double* lfborder, float* out, int B, void* stream) {
  if (!xyz || !choose || !extent || !lfborder || !out) return KRRN_EARG;
  if (B < 1 || N < 1 || HW < 1 || (long long)B * N > 0x7fffffffLL / 3) return KRRN_ESHAPE;
  const int total = B * N;
  hipLaunchKernelGGL(model_points_kernel, dim3(krrn_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, xyz, HW,
                     choose, N, extent, lfborder, out, total);
  return krrn_launch_status();
}

KRRN_API int krrn_umeyama_ransac_f32(const float* src, const float* dst, int N, const int* subsets, int H,
                                     double inlier_frac, double conf, double min_ratio, int* hyp_counts, float* scale,
                                     float* R, float* t, int* inliers, int* best_hyp, unsigned char* inlier_mask, int B,
                                     void* stream) {
  if (!src || !dst || !subsets || !hyp_counts || !scale || !R || !t || !inliers) return KRRN_EARG;
  if (N < 5 || N > kUmeMaxN || H < 1 || H > kUmeMaxH || B < 1) return KRRN_ESHAPE;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds1 = sizeof(float) * 6 * (size_t)N;
  const size_t lds2 = lds1 + sizeof(int) * (size_t)H;
  if (lds1 > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)ume_score_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1);
    if (e != hipSuccess) return (int)e;
  }
  if (lds2 > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)ume_refit_kernel,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(ume_score_kernel, dim3(B, krrn_cdiv(H, kUmeHypPerBlock)), dim3(kUmeThreads), lds1, s, src, dst, N,
                     subsets, H, inlier_frac, hyp_counts);
  hipLaunchKernelGGL(ume_refit_kernel, dim3(B), dim3(kUmeThreads), lds2, s, src, dst, N, subsets, H, inlier_frac, conf,
                     min_ratio, hyp_counts, scale, R, t, inliers, best_hyp, inlier_mask);
  return krrn_launch_status();
}
