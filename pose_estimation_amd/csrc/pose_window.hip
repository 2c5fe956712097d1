// The zoom-in pass's window: from a pose estimate, the object's model points and the camera, the
// square window of the frame that the next pass crops, computed on the device so that it can feed
// krrn_crop_inputs_resize_u8 / krrn_choose_points_resize (which read rc[b] and side[b] from device memory) without a
// read-back. This project's own rule; all f64, integer results:
//
//   per point   X = ((R00 x + R01 y) + R02 z) + t0 (Y, Z alike), u = (fx X) / Z + cx, v = (fy Y) / Z + cy;
//               the point is bad unless Z > 0 and u and v are finite (tested per point: NaN fails `Z > 0`)
//   status 1    any bad point; status 2: the points' box [umin, umax] x [vmin, vmax] misses the frame
//   status 0    e = max(umax - umin, vmax - vmin) pad, S = clamp(ceil(e), min_side, min(H, W)),
//               c0 = clamp(floor((umin + umax) 0.5 - S 0.5 + 1.0), 0, W - S), r0 alike with H: clamped in f64
//               before the conversion to int (a garbage pose gives e ~ 1e300), shifted into the frame, never shrunk
//   otherwise   the previous window (rc_in, side_in) is kept
//
// One block of 256 threads per crop: the threads stride over the points with four extremes and a bad flag in
// registers, the waves reduce by shuffles, the four waves through LDS, thread 0 finishes and stores. Min and max are
// order-free, so the result does not depend on the reduction's order. Compiled without FMA contraction: every f64
// product and sum is rounded on its own, as the numpy restatement's are.
#include "krrn_common.h"

#include <math.h>

namespace {

constexpr int kWinThreads = 256;
constexpr int kWinWaves = kWinThreads / 64;

__device__ __forceinline__ double wave_min_f64(double v) {
  for (int m = 32; m >= 1; m >>= 1) {
    const double o = __shfl_xor(v, m);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ double wave_max_f64(double v) {
  for (int m = 32; m >= 1; m >>= 1) {
    const double o = __shfl_xor(v, m);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ double clamp_f64(double x, double lo, double hi) {
  x = x < lo ? lo : x;
  return x > hi ? hi : x;
}

__global__ __launch_bounds__(kWinThreads) void pose_windows_kernel(
    const float* __restrict__ pts, int P, const double* __restrict__ R, const double* __restrict__ t,
    const float* __restrict__ K4, int H, int W, int T, double pad, int min_side, const int* rc_in, const int* side_in,
    int* rc, int* side, float* __restrict__ bbox, float* __restrict__ scale, float* __restrict__ intr,
    int* __restrict__ status) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* Rb = R + 9 * (size_t)b;
  const double r00 = Rb[0], r01 = Rb[1], r02 = Rb[2], r10 = Rb[3], r11 = Rb[4], r12 = Rb[5], r20 = Rb[6], r21 = Rb[7],
               r22 = Rb[8];
  const double t0 = t[3 * (size_t)b], t1 = t[3 * (size_t)b + 1], t2 = t[3 * (size_t)b + 2];
  const double fx = (double)K4[4 * b], fy = (double)K4[4 * b + 1], cx = (double)K4[4 * b + 2],
               cy = (double)K4[4 * b + 3];
  const float* pb = pts + (size_t)b * P * 3;
  double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
  int bad = 0;
  for (int i = tid; i < P; i += kWinThreads) {
    const double x = (double)pb[3 * (size_t)i], y = (double)pb[3 * (size_t)i + 1], z = (double)pb[3 * (size_t)i + 2];
    const double X = ((r00 * x + r01 * y) + r02 * z) + t0;
    const double Y = ((r10 * x + r11 * y) + r12 * z) + t1;
    const double Z = ((r20 * x + r21 * y) + r22 * z) + t2;
    const double u = (fx * X) / Z + cx, v = (fy * Y) / Z + cy;
    if (!(Z > 0.0) || !isfinite(u) || !isfinite(v)) {
      bad = 1;
      continue;
    }
    umin = u < umin ? u : umin;
    umax = u > umax ? u : umax;
    vmin = v < vmin ? v : vmin;
    vmax = v > vmax ? v : vmax;
  }
  umin = wave_min_f64(umin);
  umax = wave_max_f64(umax);
  vmin = wave_min_f64(vmin);
  vmax = wave_max_f64(vmax);
  for (int m = 32; m >= 1; m >>= 1) bad |= __shfl_xor(bad, m);
  __shared__ double ext[kWinWaves][4];
  __shared__ int flag[kWinWaves];
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    ext[w][0] = umin;
    ext[w][1] = umax;
    ext[w][2] = vmin;
    ext[w][3] = vmax;
    flag[w] = bad;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < kWinWaves; ++w) {
    umin = ext[w][0] < umin ? ext[w][0] : umin;
    umax = ext[w][1] > umax ? ext[w][1] : umax;
    vmin = ext[w][2] < vmin ? ext[w][2] : vmin;
    vmax = ext[w][3] > vmax ? ext[w][3] : vmax;
    bad |= flag[w];
  }
  int st = 0;
  if (bad)
    st = 1;
  else if (umax < 0.0 || umin > (double)(W - 1) || vmax < 0.0 || vmin > (double)(H - 1))
    st = 2;
  int S = side_in[b], r0 = rc_in[2 * b], c0 = rc_in[2 * b + 1];
  if (st == 0) {
    const double du = umax - umin, dv = vmax - vmin;
    const double e = (du > dv ? du : dv) * pad;
    const double s = clamp_f64(ceil(e), (double)min_side, (double)(H < W ? H : W));
    const double c = clamp_f64(floor(((umin + umax) * 0.5 - s * 0.5) + 1.0), 0.0, (double)W - s);
    const double r = clamp_f64(floor(((vmin + vmax) * 0.5 - s * 0.5) + 1.0), 0.0, (double)H - s);
    S = (int)s;
    c0 = (int)c;
    r0 = (int)r;
  }
  rc[2 * b] = r0;
  rc[2 * b + 1] = c0;
  side[b] = S;
  status[b] = st;
  bbox[4 * b + 0] = (float)r0;
  bbox[4 * b + 1] = (float)(r0 + S);
  bbox[4 * b + 2] = (float)c0;
  bbox[4 * b + 3] = (float)(c0 + S);
  // dataset.resize_intrinsic's formula in f64 from the f32 K4, cast once
  const double sc = (double)S / (double)T;
  scale[b] = (float)sc;
  intr[4 * b + 0] = (float)(fx / sc);
  intr[4 * b + 1] = (float)(fy / sc);
  intr[4 * b + 2] = (float)(((cx - (double)c0) + 0.5) / sc - 0.5);
  intr[4 * b + 3] = (float)(((cy - (double)r0) + 0.5) / sc - 0.5);
}

}  // namespace

KRRN_API int krrn_pose_windows_f64(const float* pts, int P, const double* R, const double* t, const float* K4, int H,
                                   int W, int T, double pad, int min_side, const int* rc_in, const int* side_in, int B,
                                   int* rc, int* side, float* bbox, float* scale, float* intr, int* status,
                                   void* stream) {
  if (!pts || !R || !t || !K4 || !rc_in || !side_in || !rc || !side || !bbox || !scale || !intr || !status)
    return KRRN_EARG;
  if (B < 1 || B > 65535 || P < 1 || T < 1 || H < 1 || W < 1) return KRRN_ESHAPE;
  if (min_side < 1 || min_side > (H < W ? H : W)) return KRRN_ESHAPE;
  if (!(pad > 0.0) || !std::isfinite(pad)) return KRRN_ESHAPE;
  hipLaunchKernelGGL(pose_windows_kernel, dim3(B), dim3(kWinThreads), 0, (hipStream_t)stream, pts, P, R, t, K4, H, W,
                     T, pad, min_side, rc_in, side_in, rc, side, bbox, scale, intr, status);
  return krrn_launch_status();
}
