// What BOP's calc_model_info script computes per object model, and a check of the symmetries a models_info.json
// declares, for O objects at once (include/krrn_hip.h states both definitions; tests/models_ref.py restates them in
// numpy f64 with the same operation order). Everything is f64 without FMA contraction (FLAGS_models): every product
// and sum is rounded on its own, so the kernels and the restatement agree bit for bit.
//
// krrn_model_extent_f64: the squared diameter (the maximum over all vertex pairs of the squared distance, O(V^2)) and
// the axis-aligned box. Two launches:
//   1. extent_box_kernel, one block per object: the box by a strided walk and a block reduction (< / > comparisons
//      only); it also stores d2[o] = 0.0, the start of the pair walk.
//   2. extent_pair_kernel, gridDim.x blocks per object striding over the object's row tiles of kExtRows vertices:
//      a thread keeps one row vertex in registers as f64; the column vertices come through LDS kExtCols at a time,
//      widened to f64 once, and every lane reads the same LDS address each step (a broadcast). The pair set is
//      symmetric, so a column tile that ends below the row tile's first vertex is skipped. The block's maximum is
//      folded into d2[o] with an integer atomicMax on the double's bit pattern: the terms are sums of squares, so
//      never negative, and the bit patterns of the non-negative doubles (+inf included) order like the values. A NaN
//      term never passes the thread's own >, so it never reaches the fold.
// krrn_symmetry_residual_f64: per declared symmetry S the maximum over the object's vertices p of the distance from
// S p to the object's surface (the minimum over its triangles of the closest-point distance). Two launches:
//   1. resid_init_kernel, one thread per symmetry: finds the object that owns it and stores the value that the walk
//      starts from (0.0), or the whole answer where there is nothing to walk (no vertices: 0.0; no faces: +inf).
//   2. resid_kernel, one block per (symmetry, vertex tile of kResRows), gridDim.y tiles striding: a thread keeps its
//      transformed vertex in registers; the faces' nine f64 coordinates come through LDS kResFaces at a time (a face
//      with a vertex index outside [0, Vtot) is staged as NaNs, whose distance never passes the <); the block's
//      maximum is folded with the same integer atomicMax.
// max and min do not depend on order, and no floating-point value is ever added across threads: the results are
// bit-reproducible, and an object's or a symmetry's do not depend on what else is in the batch.
#include <math.h>

#include "krrn_range.h"   // mod_range
#include "krrn_raster.h"  // Span, rast_overlap

namespace {

constexpr int kExtRows = 256;      // row tile = the block: one row vertex per thread (models.py EXTENT_R)
constexpr int kExtCols = 1024;     // column tile staged in LDS as f64 [kExtCols][3] (24 KiB) (models.py EXTENT_C)
constexpr int kExtMaxBlocks = 512; // blocks per object of the pair walk, striding over the row tiles
constexpr int kResRows = 256;      // vertex tile of the residual (models.py RESIDUAL_R)
constexpr int kResFaces = 256;     // face tile staged in LDS as f64 [kResFaces][9] (18 KiB) (models.py RESIDUAL_C)
constexpr int kResMaxTiles = 256;  // vertex-tile blocks per symmetry, striding
constexpr int kModWaves = 4;

__device__ __forceinline__ double mod_shfl_down(double v, int off) {
  return __longlong_as_double(__shfl_down(__double_as_longlong(v), off));
}

// the block's maximum of non-negative, non-NaN values (s_red: kModWaves doubles); valid in thread 0
__device__ __forceinline__ double mod_block_max(double m, double* s_red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int off = 32; off > 0; off >>= 1) {
    const double other = mod_shfl_down(m, off);
    if (other > m) m = other;
  }
  if (lane == 0) s_red[wave] = m;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < kModWaves; ++w)
      if (s_red[w] > m) m = s_red[w];
  return m;
}

// order-free fold of a non-negative double into *dst (bit patterns of the non-negative doubles order like the values)
__device__ __forceinline__ void mod_fold_max(double* dst, double m) {
  atomicMax(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)__double_as_longlong(m));
}

__global__ __launch_bounds__(kExtRows) void extent_box_kernel(const float* __restrict__ verts, int Vtot,
                                                              const int* __restrict__ vert_range, int max_v,
                                                              double* __restrict__ d2, double* __restrict__ box) {
  __shared__ double s_box[kModWaves][6];
  const int o = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long v0;
  int nv;
  mod_range(vert_range, o, Vtot, max_v, v0, nv);
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = tid; i < nv; i += kExtRows) {
    const float* p = verts + (size_t)(v0 + i) * 3;
    for (int k = 0; k < 3; ++k) {
      const double c = (double)p[k];
      if (c < lo[k]) lo[k] = c;  // a NaN coordinate passes neither test
      if (c > hi[k]) hi[k] = c;
    }
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int k = 0; k < 3; ++k) {
      const double l = mod_shfl_down(lo[k], off), h = mod_shfl_down(hi[k], off);
      if (l < lo[k]) lo[k] = l;
      if (h > hi[k]) hi[k] = h;
    }
  if (lane == 0)
    for (int k = 0; k < 3; ++k) s_box[wave][k] = lo[k], s_box[wave][3 + k] = hi[k];
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kModWaves; ++w)
      for (int k = 0; k < 3; ++k) {
        if (s_box[w][k] < lo[k]) lo[k] = s_box[w][k];
        if (s_box[w][3 + k] > hi[k]) hi[k] = s_box[w][3 + k];
      }
    for (int k = 0; k < 3; ++k) box[(size_t)o * 6 + k] = lo[k], box[(size_t)o * 6 + 3 + k] = hi[k];
    d2[o] = 0.0;  // the pair walk's start; the launch after this one folds into it
  }
}

__global__ __launch_bounds__(kExtRows) void extent_pair_kernel(const float* __restrict__ verts, int Vtot,
                                                               const int* __restrict__ vert_range, int max_v,
                                                               double* __restrict__ d2) {
  __shared__ double s_col[kExtCols * 3];
  __shared__ double s_red[kModWaves];
  const int o = blockIdx.y, tid = threadIdx.x;
  long long v0;
  int nv;
  mod_range(vert_range, o, Vtot, max_v, v0, nv);
  if (nv < 2) return;  // uniform over the block
  const float* base = verts + (size_t)v0 * 3;
  const int row_tiles = krrn_cdiv(nv, kExtRows);
  double best = 0.0;
  for (int rt = blockIdx.x; rt < row_tiles; rt += gridDim.x) {
    const int row0 = rt * kExtRows, i = row0 + tid;
    // a thread past the object's last vertex holds NaNs: none of its terms passes the >
    double x = NAN, y = NAN, z = NAN;
    if (i < nv) x = (double)base[(size_t)i * 3], y = (double)base[(size_t)i * 3 + 1], z = (double)base[(size_t)i * 3 + 2];
    for (int c0 = (row0 / kExtCols) * kExtCols; c0 < nv; c0 += kExtCols) {  // the tiles below the diagonal are skipped
      const int nc = min(kExtCols, nv - c0);
      __syncthreads();  // the previous tile has been read
      for (int k = tid; k < nc * 3; k += kExtRows) s_col[k] = (double)base[(size_t)c0 * 3 + k];
      __syncthreads();
      for (int j = 0; j < nc; ++j) {
        const double dx = x - s_col[3 * j], dy = y - s_col[3 * j + 1], dz = z - s_col[3 * j + 2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d > best) best = d;
      }
    }
  }
  __syncthreads();
  best = mod_block_max(best, s_red);
  if (tid == 0 && best > 0.0) mod_fold_max(d2 + o, best);
}

struct Vec3 {
  double x, y, z;
};

__device__ __forceinline__ Vec3 v_sub(const Vec3& a, const Vec3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double v_dot(const Vec3& a, const Vec3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// a + t d
__device__ __forceinline__ Vec3 v_at(const Vec3& a, double t, const Vec3& d) {
  return {a.x + t * d.x, a.y + t * d.y, a.z + t * d.z};
}

// the squared distance from p to the triangle (a, b, c): the closest point by the region tests in the header's order,
// the first test that holds deciding. A NaN anywhere fails every test and ends in the last case with a NaN result.
__device__ __forceinline__ double tri_dist2(const Vec3& p, const Vec3& a, const Vec3& b, const Vec3& c) {
  const Vec3 ab = v_sub(b, a), ac = v_sub(c, a), ap = v_sub(p, a);
  const double d1 = v_dot(ab, ap), d2 = v_dot(ac, ap);
  Vec3 q;
  if (d1 <= 0.0 && d2 <= 0.0) {
    q = a;
  } else {
    const Vec3 bp = v_sub(p, b);
    const double d3 = v_dot(ab, bp), d4 = v_dot(ac, bp);
    const double vc = d1 * d4 - d3 * d2;
    if (d3 >= 0.0 && d4 <= d3) {
      q = b;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
      q = v_at(a, d1 / (d1 - d3), ab);
    } else {
      const Vec3 cp = v_sub(p, c);
      const double d5 = v_dot(ab, cp), d6 = v_dot(ac, cp);
      const double vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
      const double e43 = d4 - d3, e56 = d5 - d6;
      if (d6 >= 0.0 && d5 <= d6) {
        q = c;
      } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        q = v_at(a, d2 / (d2 - d6), ac);
      } else if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {
        q = v_at(b, e43 / (e43 + e56), v_sub(c, b));
      } else {
        const double den = 1.0 / ((va + vb) + vc);
        const double v = vb * den, w = vc * den;
        q = {(a.x + ab.x * v) + ac.x * w, (a.y + ab.y * v) + ac.y * w, (a.z + ab.z * v) + ac.z * w};
      }
    }
  }
  const Vec3 d = v_sub(p, q);
  return v_dot(d, d);
}

// the object that owns symmetry s: the lowest o whose (guarded) sym_range holds it, or -1
__device__ __forceinline__ int resid_owner(const int* sym_range, int O, int NStot, int s) {
  for (int o = 0; o < O; ++o) {
    long long s0;
    int ns;
    mod_range(sym_range, o, NStot, NStot, s0, ns);
    if (s >= s0 && s < s0 + ns) return o;
  }
  return -1;
}

__global__ void resid_init_kernel(const int* __restrict__ vert_range, int Vtot, const int* __restrict__ face_range,
                                  int Ftot, const int* __restrict__ sym_range, int NStot, int O, int max_v, int max_f,
                                  double* __restrict__ res2) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= NStot) return;
  const int o = resid_owner(sym_range, O, NStot, s);
  if (o < 0) return;  // a symmetry that no object owns keeps what the buffer held
  long long v0, f0;
  int nv, nf;
  mod_range(vert_range, o, Vtot, max_v, v0, nv);
  mod_range(face_range, o, Ftot, max_f, f0, nf);
  res2[s] = (nv > 0 && nf == 0) ? INFINITY : 0.0;
}

__global__ __launch_bounds__(kResRows) void resid_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ vert_range, const int* __restrict__ face_range, const double* __restrict__ syms, int NStot,
    const int* __restrict__ sym_range, int O, int max_v, int max_f, double* __restrict__ res2) {
  __shared__ double s_face[kResFaces * 9];
  __shared__ double s_red[kModWaves];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int o = resid_owner(sym_range, O, NStot, s);  // uniform over the block
  if (o < 0) return;
  long long v0, f0;
  int nv, nf;
  mod_range(vert_range, o, Vtot, max_v, v0, nv);
  mod_range(face_range, o, Ftot, max_f, f0, nf);
  if (nv == 0 || nf == 0) return;  // resid_init_kernel stored the answer
  const double* S = syms + (size_t)s * 12;
  const int tiles = krrn_cdiv(nv, kResRows);
  double worst = 0.0;
  for (int vt = blockIdx.y; vt < tiles; vt += gridDim.y) {
    const int i = vt * kResRows + tid;
    const bool live = i < nv;
    Vec3 p = {0.0, 0.0, 0.0};
    if (live) {
      const float* v = verts + (size_t)(v0 + i) * 3;
      const double x = (double)v[0], y = (double)v[1], z = (double)v[2];
      p.x = ((S[0] * x + S[1] * y) + S[2] * z) + S[9];
      p.y = ((S[3] * x + S[4] * y) + S[5] * z) + S[10];
      p.z = ((S[6] * x + S[7] * y) + S[8] * z) + S[11];
    }
    double nearest = INFINITY;
    for (int c0 = 0; c0 < nf; c0 += kResFaces) {
      const int nc = min(kResFaces, nf - c0);
      __syncthreads();  // the previous tile has been read
      if (tid < nc) {
        const int* fv = faces + (size_t)(f0 + c0 + tid) * 3;
        const int i0 = fv[0], i1 = fv[1], i2 = fv[2];
        const bool ok = i0 >= 0 && i0 < Vtot && i1 >= 0 && i1 < Vtot && i2 >= 0 && i2 < Vtot;
        const int iv[3] = {i0, i1, i2};
        for (int k = 0; k < 3; ++k)
          for (int c = 0; c < 3; ++c) s_face[tid * 9 + k * 3 + c] = ok ? (double)verts[(size_t)iv[k] * 3 + c] : NAN;
      }
      __syncthreads();
      if (live)
        for (int j = 0; j < nc; ++j) {
          const double* t = s_face + j * 9;
          const double d = tri_dist2(p, {t[0], t[1], t[2]}, {t[3], t[4], t[5]}, {t[6], t[7], t[8]});
          if (d < nearest) nearest = d;
        }
    }
    if (live && nearest > worst) worst = nearest;  // a vertex without a finite distance kept +inf
  }
  __syncthreads();
  worst = mod_block_max(worst, s_red);
  if (tid == 0 && worst > 0.0) mod_fold_max(res2 + s, worst);
}

}  // namespace

KRRN_API int krrn_model_extent_f64(const float* verts, int Vtot, const int* vert_range, int O, int max_v, double* d2,
                                   double* box, void* stream) {
  if (!verts || !vert_range || !d2 || !box) return KRRN_EARG;
  if (O < 1 || O > 65535 || Vtot < 1 || max_v < 1) return KRRN_ESHAPE;
  const size_t n = (size_t)O;
  const Span outs[2] = {{d2, 8 * n}, {box, 48 * n}};
  const Span ins[2] = {{verts, 12 * (size_t)Vtot}, {vert_range, 8 * n}};
  if (rast_overlap(outs, 2, ins, 2)) return KRRN_EARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(extent_box_kernel, dim3(O), dim3(kExtRows), 0, st, verts, Vtot, vert_range, max_v, d2, box);
  const int blocks = min(krrn_cdiv(max_v, kExtRows), kExtMaxBlocks);
  hipLaunchKernelGGL(extent_pair_kernel, dim3(blocks, O), dim3(kExtRows), 0, st, verts, Vtot, vert_range, max_v, d2);
  return krrn_launch_status();
}

KRRN_API int krrn_symmetry_residual_f64(const float* verts, int Vtot, const int* faces, int Ftot,
                                        const int* vert_range, const int* face_range, const double* syms, int NStot,
                                        const int* sym_range, int O, int max_v, int max_f, double* res2,
                                        void* stream) {
  if (!verts || !vert_range || !face_range || !syms || !sym_range || !res2 || (!faces && Ftot > 0)) return KRRN_EARG;
  if (O < 1 || Vtot < 1 || Ftot < 0 || NStot < 1 || max_v < 1 || max_f < 1) return KRRN_ESHAPE;
  const int tiles = min(krrn_cdiv(max_v, kResRows), kResMaxTiles);
  if ((long long)NStot * tiles > (1ll << 23)) return KRRN_ESHAPE;  // blocks x 256 threads stay below 2^32
  const size_t n = (size_t)O;
  const Span outs[1] = {{res2, 8 * (size_t)NStot}};
  const Span ins[6] = {{verts, 12 * (size_t)Vtot}, {faces, 12 * (size_t)Ftot}, {vert_range, 8 * n},
                       {face_range, 8 * n},        {syms, 96 * (size_t)NStot}, {sym_range, 8 * n}};
  if (rast_overlap(outs, 1, ins, 6)) return KRRN_EARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(resid_init_kernel, dim3(krrn_cdiv(NStot, 256)), dim3(256), 0, st, vert_range, Vtot, face_range,
                     Ftot, sym_range, NStot, O, max_v, max_f, res2);
  hipLaunchKernelGGL(resid_kernel, dim3(NStot, tiles), dim3(kResRows), 0, st, verts, Vtot, faces, Ftot, vert_range,
                     face_range, syms, NStot, sym_range, O, max_v, max_f, res2);
  return krrn_launch_status();
}
