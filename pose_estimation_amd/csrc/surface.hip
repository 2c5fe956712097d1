// Points drawn uniformly on the surface of O triangle meshes at once (krrn_surface_sample_f64; include/krrn_hip.h
// states the definition, tests/surface_ref.py restates it in numpy f64 with the same operation order): a face is
// chosen with probability proportional to its area, and a point on it by the square-root barycentric map. Everything
// is f64 without FMA contraction (FLAGS_surface): every product and sum is rounded on its own, so the kernels and the
// restatement agree bit for bit. Three launches:
//   1. surf_weight_kernel, a thread per face: w_k = |e1 x e2| (twice the face's area; 0 for a degenerate face, a
//      non-finite one or an index outside [0, Vtot)) stored into the object's cum row, coalesced.
//   2. surf_scan_kernel, one block per object, a thread per tile of kSurfTile faces: the thread sums its tile in face
//      order in place (cum[k] = run), thread 0 then walks the tile totals in tile order to form the bases, and the
//      block adds each tile's base to its faces. An object with more tiles than the block has threads takes them
//      kSurfTile tiles at a time, the base carried on. The order of every sum is fixed by (face, tile), not by the
//      launch. Thread 0 also stores status (1 when the total is 0).
//   3. surf_sample_kernel, a thread per sample: four draws of the generator (krrn_rng.h), a binary search for the first
//      cum[k] > target, the point and the face's flat normal recomputed from its corners.
// No atomics, no floating-point value combined across lanes, no workspace beyond cum, no read-back: an object's
// outputs depend on its own faces, its row_id and the seed only.
#include <math.h>

#include "krrn_common.h"
#include "krrn_range.h"  // mod_range
#include "krrn_rng.h"    // rand32

namespace {

constexpr int kSurfTile = 256;  // faces per tile of the cumulative sum = threads per block (tests/surface_ref.py TILE)

// The face's corners widened to f64, N = e1 x e2 and w = |N| by the header's expressions. Returns false (w = 0, N and
// the corners untouched or meaningless) for an index outside [0, Vtot); a degenerate or non-finite face has w = 0.
__device__ __forceinline__ bool surf_face(const float* __restrict__ verts, int Vtot, const int* __restrict__ fv,
                                          double a[3], double b[3], double c[3], double N[3], double& w) {
  const int i0 = fv[0], i1 = fv[1], i2 = fv[2];
  w = 0.0;
  if (!(i0 >= 0 && i0 < Vtot && i1 >= 0 && i1 < Vtot && i2 >= 0 && i2 < Vtot)) return false;
  for (int k = 0; k < 3; ++k) {
    a[k] = (double)verts[(size_t)i0 * 3 + k];
    b[k] = (double)verts[(size_t)i1 * 3 + k];
    c[k] = (double)verts[(size_t)i2 * 3 + k];
  }
  const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
  const double e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
  N[0] = e1y * e2z - e1z * e2y;
  N[1] = e1z * e2x - e1x * e2z;
  N[2] = e1x * e2y - e1y * e2x;
  const double A2 = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2];
  if (A2 > 0.0 && A2 < INFINITY) w = sqrt(A2);  // a NaN passes neither comparison
  return true;
}

__global__ __launch_bounds__(kSurfTile) void surf_weight_kernel(const float* __restrict__ verts, int Vtot,
                                                                const int* __restrict__ faces, int Ftot,
                                                                const int* __restrict__ face_range, int max_f,
                                                                double* __restrict__ cum) {
  const int o = blockIdx.y, k = blockIdx.x * kSurfTile + threadIdx.x;
  long long f0;
  int nf;
  mod_range(face_range, o, Ftot, max_f, f0, nf);
  if (k >= nf) return;
  double a[3], b[3], c[3], N[3], w;
  surf_face(verts, Vtot, faces + (size_t)(f0 + k) * 3, a, b, c, N, w);
  cum[(size_t)o * max_f + k] = w;
}

__global__ __launch_bounds__(kSurfTile) void surf_scan_kernel(const int* __restrict__ face_range, int Ftot, int max_f,
                                                              double* __restrict__ cum, int* __restrict__ status) {
  __shared__ double s_base[kSurfTile];  // in: a tile's last run; out: the tile's base
  __shared__ double s_carry;            // the base of the next chunk's first tile
  const int o = blockIdx.x, tid = threadIdx.x;
  long long f0;
  int nf;
  mod_range(face_range, o, Ftot, max_f, f0, nf);
  double* row = cum + (size_t)o * max_f;
  const int tiles = nf > 0 ? (nf - 1) / kSurfTile + 1 : 0;
  if (tid == 0) s_carry = 0.0;
  for (int t0 = 0; t0 < tiles; t0 += kSurfTile) {  // uniform over the block
    const int j = t0 + tid;
    double run = 0.0;
    if (j < tiles) {
      const int k0 = j * kSurfTile, k1 = k0 + min(kSurfTile, nf - k0);
      for (int k = k0; k < k1; ++k) {
        run = run + row[k];
        row[k] = run;
      }
    }
    s_base[tid] = run;
    __syncthreads();  // the runs are stored (row: global writes of this block, read back below) and s_carry is set
    if (tid == 0) {
      double base = s_carry;
      const int nt = min(kSurfTile, tiles - t0);
      for (int t = 0; t < nt; ++t) {
        const double last = s_base[t];
        s_base[t] = base;
        base = base + last;
      }
      s_carry = base;
    }
    __syncthreads();
    const long long k0 = (long long)t0 * kSurfTile, k1 = min((long long)nf, k0 + kSurfTile * kSurfTile);
    for (long long k = k0 + tid; k < k1; k += kSurfTile) row[k] = s_base[(k - k0) / kSurfTile] + row[k];
    __syncthreads();  // s_base is free for the next chunk
  }
  __syncthreads();
  if (tid == 0) status[o] = s_carry == 0.0 ? 1 : 0;
}

__global__ __launch_bounds__(kSurfTile) void surf_sample_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ face_range, const int* __restrict__ row_id, int max_f, int n, unsigned long long seed,
    unsigned int stream_id, const double* __restrict__ cum, float* __restrict__ pts, float* __restrict__ nrm,
    int* __restrict__ face) {
  const int o = blockIdx.y, i = blockIdx.x * kSurfTile + threadIdx.x;
  if (i >= n) return;
  long long f0;
  int nf;
  mod_range(face_range, o, Ftot, max_f, f0, nf);
  const double* row = cum + (size_t)o * max_f;
  const double total = nf > 0 ? row[nf - 1] : 0.0;
  const size_t e = (size_t)o * n + i;
  float p[3] = {0.f, 0.f, 0.f}, q[3] = {0.f, 0.f, 0.f};
  int chosen = -1;
  if (total != 0.0) {
    const unsigned int row_o = (unsigned int)row_id[o], c0 = 4u * (unsigned int)i;
    const unsigned int r0 = rand32(seed, stream_id, row_o, c0), r1 = rand32(seed, stream_id, row_o, c0 + 1);
    const unsigned int r2 = rand32(seed, stream_id, row_o, c0 + 2), r3 = rand32(seed, stream_id, row_o, c0 + 3);
    const unsigned long long m = (((unsigned long long)r0 << 32) | r1) >> 11;
    const double target = ((double)m * 0x1p-53) * total;
    int lo = 0, hi = nf;  // the first k with cum[k] > target (cum is non-decreasing), nf if none
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (row[mid] > target) hi = mid; else lo = mid + 1;
    }
    chosen = lo < nf ? lo : nf - 1;
    double a[3], b[3], c[3], N[3], w;
    // a chosen face has w > 0; only the `none` case (a total that is not finite) can land on one with a bad index,
    // whose point and normal stay 0
    if (surf_face(verts, Vtot, faces + (size_t)(f0 + chosen) * 3, a, b, c, N, w)) {
      const double u1 = (double)r2 * 0x1p-32, u2 = (double)r3 * 0x1p-32, s = sqrt(u1);
      const double wa = 1.0 - s, wb = s * (1.0 - u2), wc = s * u2;
      for (int k = 0; k < 3; ++k) {
        p[k] = (float)((wa * a[k] + wb * b[k]) + wc * c[k]);
        q[k] = (float)(N[k] / w);
      }
    }
  }
  for (int k = 0; k < 3; ++k) pts[e * 3 + k] = p[k], nrm[e * 3 + k] = q[k];
  face[e] = chosen;
}

}  // namespace

KRRN_API int krrn_surface_sample_f64(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                                     const int* row_id, int O, int max_f, int n, long long seed,
                                     unsigned int stream_id, double* cum, float* pts, float* nrm, int* face,
                                     int* status, void* stream) {
  if (!verts || !face_range || !row_id || !cum || !pts || !nrm || !face || !status || (!faces && Ftot > 0))
    return KRRN_EARG;
  if (O < 1 || O > 65535 || Vtot < 1 || Ftot < 0 || max_f < 1 || n < 1 || n > (1 << 28)) return KRRN_ESHAPE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(surf_weight_kernel, dim3((max_f - 1) / kSurfTile + 1, O), dim3(kSurfTile), 0, st, verts, Vtot,
                     faces, Ftot, face_range, max_f, cum);
  hipLaunchKernelGGL(surf_scan_kernel, dim3(O), dim3(kSurfTile), 0, st, face_range, Ftot, max_f, cum, status);
  hipLaunchKernelGGL(surf_sample_kernel, dim3(krrn_cdiv(n, kSurfTile), O), dim3(kSurfTile), 0, st, verts, Vtot, faces,
                     Ftot, face_range, row_id, max_f, n, (unsigned long long)seed, stream_id, cum, pts, nrm, face);
  return krrn_launch_status();
}
