// The rasteriser's depth definition, stated once for the kernels that render a mesh under a pose
// (raster.hip: the GT maps; bop.hip: the two depth images of VSD). include/krrn_hip.h
// (krrn_raster_maps_f32) and the head of raster.hip give the definition; tests/raster_ref.py restates it.
// Everything here is f64 and must be compiled without FMA contraction (FLAGS_raster / FLAGS_bop).
#pragma once
#include <math.h>

#include "krrn_mask.h"  // the 16 x 16 tile layout (integer code only)

namespace {

constexpr int kRastTile = kMaskTile;
constexpr int kRastThreads = kMaskThreads;  // one thread per pixel of the tile; also the face chunk
constexpr int kRastWaves = kMaskWaves;
constexpr int kRastSetup = 14;                       // doubles per compacted face
constexpr double kRastNear = 1e-3;

struct RastCam {
  double r[9], t[3], fx, fy, cx, cy;
};

// the winner of one pixel: depth, the q_k = w_k / z_k of the winning face, its index in the crop's range
struct RastHit {
  double z, q0, q1, q2;
  int f;
};

__device__ __forceinline__ void rast_load_cam(RastCam& cam, const double* R, const double* t, const float* K4,
                                              int b) {
  for (int i = 0; i < 9; ++i) cam.r[i] = R[9 * b + i];
  for (int i = 0; i < 3; ++i) cam.t[i] = t[3 * b + i];
  cam.fx = (double)K4[4 * b + 0];
  cam.fy = (double)K4[4 * b + 1];
  cam.cx = (double)K4[4 * b + 2];
  cam.cy = (double)K4[4 * b + 3];
}

__device__ __forceinline__ void rast_camera(const RastCam& cam, const float* v, double (&c)[3]) {
  const double x = (double)v[0], y = (double)v[1], z = (double)v[2];
  c[0] = ((cam.r[0] * x + cam.r[1] * y) + cam.r[2] * z) + cam.t[0];
  c[1] = ((cam.r[3] * x + cam.r[4] * y) + cam.r[5] * z) + cam.t[1];
  c[2] = ((cam.r[6] * x + cam.r[7] * y) + cam.r[8] * z) + cam.t[2];
}

__device__ __forceinline__ double rast_edge(double au, double av, double bu, double bv, double pu, double pv) {
  return (bu - au) * (pv - av) - (bv - av) * (pu - au);
}

// a (first, count) range of device memory, clamped to [0, total): nothing on the host saw it. A negative
// first or count, or a first beyond the array, is an empty range; a range is cut at `total`.
__device__ __forceinline__ void rast_range(const int* range, int b, int total, long long& first, int& count) {
  first = range[2 * b];
  long long n = range[2 * b + 1];
  if (first < 0 || n < 0 || first > total) n = 0;
  if (first + n > total) n = total - first;
  count = (int)n;
}

// The depth walk of one 16 x 16 tile (all 256 threads of the block call it, with block-uniform cam, f0,
// nf and tile bounds): the crop's faces in chunks of 256; thread i projects face chunk + i and tests its
// bounding box against the tile's sample points [tu0, tu1] x [tv0, tv1]; the survivors are compacted into
// LDS in face order (wave ballot + prefix, then the four waves in order) with their edge setup; then every
// thread with `inside` walks the list for its sample point (pu, pv) with a strict < on depth, so ties go
// to the lowest face index. hit.f = -1 (hit.z = +inf) when no face covers the point. Ends with a barrier:
// the caller may reuse the three LDS arrays at once.
__device__ __forceinline__ void rast_depth_walk(const RastCam& cam, const float* __restrict__ verts, int Vtot,
                                                const int* __restrict__ faces, long long f0, int nf, double tu0,
                                                double tu1, double tv0, double tv1, double pu, double pv,
                                                bool inside, double* s_setup, int* s_id, int* s_wcnt,
                                                RastHit& hit) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  hit.z = INFINITY, hit.q0 = 0.0, hit.q1 = 0.0, hit.q2 = 0.0, hit.f = -1;
  for (int base = 0; base < nf; base += kRastThreads) {  // nf is uniform over the block
    const int fi = base + tid;
    bool keep = false;
    double su[3], sv[3], sz[3], A = 0.0, umin = 0.0, umax = 0.0, vmin = 0.0, vmax = 0.0;
    if (fi < nf) {
      const int* fv = faces + (size_t)(f0 + fi) * 3;
      const int i0 = fv[0], i1 = fv[1], i2 = fv[2];
      if (i0 >= 0 && i0 < Vtot && i1 >= 0 && i1 < Vtot && i2 >= 0 && i2 < Vtot) {
        const int iv[3] = {i0, i1, i2};
        bool front = true;
        for (int k = 0; k < 3; ++k) {
          double c[3];
          rast_camera(cam, verts + (size_t)iv[k] * 3, c);
          front = front && (c[2] > kRastNear);  // false for NaN too
          su[k] = cam.fx * c[0] / c[2] + cam.cx;
          sv[k] = cam.fy * c[1] / c[2] + cam.cy;
          sz[k] = c[2];
        }
        A = rast_edge(su[0], sv[0], su[1], sv[1], su[2], sv[2]);
        umin = fmin(fmin(su[0], su[1]), su[2]);
        umax = fmax(fmax(su[0], su[1]), su[2]);
        vmin = fmin(fmin(sv[0], sv[1]), sv[2]);
        vmax = fmax(fmax(sv[0], sv[1]), sv[2]);
        keep = front && A != 0.0 && isfinite(A) && umax >= tu0 && umin <= tu1 && vmax >= tv0 && vmin <= tv1;
      }
    }
    // order-preserving compaction: the wave's ballot gives the rank inside the wave, the waves go in order
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, total = 0;
    for (int w = 0; w < kRastWaves; ++w) {
      const int c = s_wcnt[w];
      off += w < wave ? c : 0;
      total += c;
    }
    if (keep) {
      const int slot = off + __popcll(bal & ((1ull << lane) - 1ull));  // < 256
      double* s = s_setup + slot * kRastSetup;
      s[0] = su[0], s[1] = sv[0], s[2] = su[1], s[3] = sv[1], s[4] = su[2], s[5] = sv[2];
      s[6] = sz[0], s[7] = sz[1], s[8] = sz[2], s[9] = A;
      s[10] = umin, s[11] = umax, s[12] = vmin, s[13] = vmax;
      s_id[slot] = fi;
    }
    __syncthreads();
    if (inside) {
      for (int j = 0; j < total; ++j) {
        const double* s = s_setup + j * kRastSetup;
        if (!(pu >= s[10] && pu <= s[11] && pv >= s[12] && pv <= s[13])) continue;
        const double a = s[9];
        const double w0 = rast_edge(s[2], s[3], s[4], s[5], pu, pv) / a;
        const double w1 = rast_edge(s[4], s[5], s[0], s[1], pu, pv) / a;
        const double w2 = rast_edge(s[0], s[1], s[2], s[3], pu, pv) / a;
        if (!(w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0)) continue;
        const double q0 = w0 / s[6], q1 = w1 / s[7], q2 = w2 / s[8];
        const double z = 1.0 / ((q0 + q1) + q2);
        if (z < hit.z) {
          hit.z = z, hit.f = s_id[j];
          hit.q0 = q0, hit.q1 = q1, hit.q2 = q2;
        }
      }
    }
    __syncthreads();  // the next chunk (or the caller) rewrites the list
  }
}

// The camera-frame normal of the face with vertex indices fv[0..2] (all inside [0, Vtot): a face the walk kept),
// as raster.hip defines it: (c1 - c0) x (c2 - c0), normalised, negated if n . c0 > 0 (towards the camera). False,
// and n = 0, for a zero or non-finite cross product.
__device__ __forceinline__ bool rast_face_normal(const RastCam& cam, const float* __restrict__ verts, const int* fv,
                                                 double (&n)[3]) {
  double c0[3], c1[3], c2[3];
  rast_camera(cam, verts + (size_t)fv[0] * 3, c0);
  rast_camera(cam, verts + (size_t)fv[1] * 3, c1);
  rast_camera(cam, verts + (size_t)fv[2] * 3, c2);
  const double e1[3] = {c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]};
  const double e2[3] = {c2[0] - c0[0], c2[1] - c0[1], c2[2] - c0[2]};
  n[0] = e1[1] * e2[2] - e1[2] * e2[1];
  n[1] = e1[2] * e2[0] - e1[0] * e2[2];
  n[2] = e1[0] * e2[1] - e1[1] * e2[0];
  const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  const bool ok = len > 0.0 && isfinite(len);
  for (int k = 0; k < 3; ++k) n[k] = ok ? n[k] / len : 0.0;
  if ((n[0] * c0[0] + n[1] * c0[1]) + n[2] * c0[2] > 0.0)
    for (int k = 0; k < 3; ++k) n[k] = -n[k];
  return ok;
}

struct Span {
  const void* p;
  size_t n;
};

// true when a non-null output span overlaps any other span
static bool rast_overlap(const Span* outs, int no, const Span* ins, int ni) {
  auto hit = [](const Span& a, const Span& b) {
    if (!a.p || !b.p) return false;
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + b.n && b0 < a0 + a.n;
  };
  for (int i = 0; i < no; ++i) {
    for (int j = i + 1; j < no; ++j)
      if (hit(outs[i], outs[j])) return true;
    for (int j = 0; j < ni; ++j)
      if (hit(outs[i], ins[j])) return true;
  }
  return false;
}

}  // namespace
