// What the kernels that compare a render with the observed depth frame share (bop.hip: VSD and the GT
// visibility; verify.hip: the pose-candidate score): the observed distance of a pixel, the projected bounding
// box of a crop's faces under a pose, and the f64 wave min / max. Stated once, on top of krrn_raster.h; f64
// without FMA contraction like everything there (FLAGS_bop / FLAGS_verify).
#pragma once
#include "krrn_raster.h"

namespace {

constexpr int kBopBoxEmptyLo = 1, kBopBoxEmptyHi = 0;
constexpr double kBopBoxClamp = 1e9;

__device__ __forceinline__ double bop_wave_min(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m));
  return v;
}

__device__ __forceinline__ double bop_wave_max(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  return v;
}

// ray = the distance per unit depth of pixel (pu, pv); obs = the observed distance there (0 for a frame index
// outside [0, F), and for a zero, negative or NaN sample)
__device__ __forceinline__ void bop_observe(const RastCam& cam, double pu, double pv, const float* __restrict__ depth,
                                            int F, int H, int W, int fr, int x, int y, double depth_scale,
                                            double& ray, double& obs) {
  const double xn = (pu - cam.cx) / cam.fx, yn = (pv - cam.cy) / cam.fy;
  ray = sqrt((xn * xn + yn * yn) + 1.0);
  double d_obs = 0.0;
  if (fr >= 0 && fr < F) d_obs = (double)depth[((size_t)fr * H + y) * W + x] / depth_scale;
  obs = d_obs > 0.0 ? d_obs * ray : 0.0;
}

// the bounding box of the projected vertices of crop b's faces under `cam` (vertices with z > 1e-3 only), as 4
// ints rounded outwards in o[0..3] = (u lo, u hi, v lo, v hi), lo > hi = no vertex. All threads of the block
// call it; thread 0 writes.
__device__ __forceinline__ void bop_project_box(const RastCam& cam, const float* __restrict__ verts, int Vtot,
                                                const int* __restrict__ faces, int Ftot,
                                                const int* __restrict__ face_range, int b, double (*s_box)[4],
                                                int* __restrict__ o) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long f0;
  int nf;
  rast_range(face_range, b, Ftot, f0, nf);
  double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
  for (int fi = tid; fi < nf; fi += kRastThreads) {
    const int* fv = faces + (size_t)(f0 + fi) * 3;
    for (int k = 0; k < 3; ++k) {
      const int i = fv[k];
      if (i < 0 || i >= Vtot) continue;
      double c[3];
      rast_camera(cam, verts + (size_t)i * 3, c);
      if (!(c[2] > kRastNear)) continue;
      const double u = cam.fx * c[0] / c[2] + cam.cx;  // the walk's own projection: the same bits
      const double v = cam.fy * c[1] / c[2] + cam.cy;
      umin = fmin(umin, u), umax = fmax(umax, u);      // fmin / fmax drop a NaN: its face is skipped (A)
      vmin = fmin(vmin, v), vmax = fmax(vmax, v);
    }
  }
  umin = bop_wave_min(umin), umax = bop_wave_max(umax);
  vmin = bop_wave_min(vmin), vmax = bop_wave_max(vmax);
  if (lane == 0) s_box[wave][0] = umin, s_box[wave][1] = umax, s_box[wave][2] = vmin, s_box[wave][3] = vmax;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kRastWaves; ++w) {
      umin = fmin(umin, s_box[w][0]), umax = fmax(umax, s_box[w][1]);
      vmin = fmin(vmin, s_box[w][2]), vmax = fmax(vmax, s_box[w][3]);
    }
    const bool any = umin <= umax && vmin <= vmax;
    auto lo = [](double x) { return (int)fmax(fmin(floor(x), kBopBoxClamp), -kBopBoxClamp); };
    auto hi = [](double x) { return (int)fmax(fmin(ceil(x), kBopBoxClamp), -kBopBoxClamp); };
    o[0] = any ? lo(umin) : kBopBoxEmptyLo, o[1] = any ? hi(umax) : kBopBoxEmptyHi;
    o[2] = any ? lo(vmin) : kBopBoxEmptyLo, o[3] = any ? hi(vmax) : kBopBoxEmptyHi;
  }
}

}  // namespace
