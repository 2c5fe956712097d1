// Ground-truth map rendering: a z-buffered triangle rasteriser that turns (mesh, GT pose, K, crop window)
// into the per-pixel maps the eval-time KRRNLoss compares against (model coordinate, normal, region label,
// coverage), batched over the crops of one size. The reference project unpickles these maps from an
// offline renderer that is not in its tree (dataset/linemod/batchdataset.py:200-210); the definition is
// this project's own (include/krrn_hip.h; tests/raster_ref.py restates it in numpy).
// Per crop b and face f of its range, all in f64 on the f32 inputs, without FMA contraction:
//
//   c_k = ((r0 x + r1 y) + r2 z) + t                       camera vertex k = 0, 1, 2 of the face
//   skip the face if a vertex index is outside [0, Vtot) or any c_k.z is not > 1e-3 (no clipping)
//   u_k = fx c_k.x / c_k.z + cx,  v_k = fy c_k.y / c_k.z + cy
//   E(a, b, p) = (b.u - a.u)(p.v - a.v) - (b.v - a.v)(p.u - a.u);  A = E(v0, v1, v2); skip if A == 0 or not finite
//   pixel p = (cmin + x, rmin + y) (integer sample points, the loader's xmap / ymap convention) is tested
//   iff it lies in the face's bounding box [min u, max u] x [min v, max v] (inclusive);
//   w0 = E(v1, v2, p) / A, w1 = E(v2, v0, p) / A, w2 = E(v0, v1, p) / A; covered iff all three >= 0
//   q_k = w_k / z_k;  z = 1 / ((q0 + q1) + q2)             perspective-correct depth
//   the winner has the smallest z (strict <, faces in increasing index: the lowest index among equal z)
//   m = z ((q0 vert_0 + q1 vert_1) + q2 vert_2)            model coordinate
//   n = normalize((c1 - c0) x (c2 - c0)), negated if n . c0 > 0 (towards the camera)
//   region = 1 + argmin_j ((dx dx + dy dy) + dz dz) of m against region_pts[b][j], the lowest j on ties
//
// One launch. A 256-thread block owns one 16 x 16 pixel tile of one crop and walks the crop's faces in
// chunks of 256: thread i projects face chunk + i and tests its bounding box against the tile; the
// survivors are compacted into LDS in face order (wave ballot + prefix, then the four waves in order)
// with their edge setup (14 doubles: 28 KiB a chunk, which is what bounds the chunk at 256); then every
// thread, one per pixel, walks the compacted list (all lanes read one LDS address: a broadcast) with a
// strict < on depth. Face order is preserved, so ties go to the lowest index with no atomics, and a
// block reads only its own crop: the result does not depend on the batch or on the launch geometry.
// The vertices are projected per (tile, face), not once per (crop, vertex) into a workspace: the face
// indices are global and a batch mixes objects, so that workspace would be B x Vtot, and the redundant
// projections (about 6 f64 divisions a face and tile) are cheaper than its traffic. The winner's
// vertices are projected once more for the normal: the same operations give the same bits.
// The depth part (camera transform, edge function, face setup, compaction, per-pixel walk) lives in
// krrn_raster.h, shared with the VSD kernel of bop.hip.
#include "krrn_raster.h"

namespace {

constexpr int kRastMaxS = 480;
constexpr int kRastMaxNR = 256;

__global__ __launch_bounds__(kRastThreads) void raster_maps_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ face_range, const double* __restrict__ R, const double* __restrict__ t,
    const float* __restrict__ K4, const int* __restrict__ rc, int S, const float* __restrict__ region_pts, int NR,
    int* __restrict__ face_out, float* __restrict__ depth, float* __restrict__ coord, float* __restrict__ normal,
    int* __restrict__ region, unsigned char* __restrict__ cover_frame, int H, int W) {
  __shared__ double s_setup[kRastThreads * kRastSetup];
  __shared__ double s_rp[kRastMaxNR * 3];
  __shared__ int s_id[kRastThreads];
  __shared__ int s_wcnt[kRastWaves];

  const int b = blockIdx.z, tid = threadIdx.x;
  const int x = blockIdx.x * kRastTile + (tid & (kRastTile - 1));
  const int y = blockIdx.y * kRastTile + (tid >> 4);
  const bool inside = x < S && y < S;

  RastCam cam;
  rast_load_cam(cam, R, t, K4, b);
  const int rmin = rc[2 * b], cmin = rc[2 * b + 1];
  // the crop's faces, clamped to the face array (face_range is device memory: nothing on the host saw it)
  long long f0;
  int nf;
  rast_range(face_range, b, Ftot, f0, nf);

  for (int i = tid; i < NR * 3; i += kRastThreads) s_rp[i] = (double)region_pts[(size_t)b * NR * 3 + i];

  const double pu = (double)(cmin + x), pv = (double)(rmin + y);
  // the tile's sample points span [tu0, tu1] x [tv0, tv1]
  const int lx = blockIdx.x * kRastTile, ly = blockIdx.y * kRastTile;
  const double tu0 = (double)(cmin + lx), tu1 = (double)(cmin + min(lx + kRastTile, S) - 1);
  const double tv0 = (double)(rmin + ly), tv1 = (double)(rmin + min(ly + kRastTile, S) - 1);

  RastHit hit;  // krrn_raster.h: the chunked, order-preserving compaction and the per-pixel walk
  rast_depth_walk(cam, verts, Vtot, faces, f0, nf, tu0, tu1, tv0, tv1, pu, pv, inside, s_setup, s_id, s_wcnt, hit);
  const double best_z = hit.z, bq0 = hit.q0, bq1 = hit.q1, bq2 = hit.q2;
  const int best_f = hit.f;
  __syncthreads();  // s_rp (also when the crop has no face)
  if (!inside) return;

  const size_t HW = (size_t)S * S, pix = (size_t)y * S + x, o1 = (size_t)b * HW + pix, o3 = (size_t)b * 3 * HW + pix;
  double m[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};
  int reg = 0;
  if (best_f >= 0) {
    const int* fv = faces + (size_t)(f0 + best_f) * 3;  // in range: it passed the test above
    const float* p0 = verts + (size_t)fv[0] * 3;
    const float* p1 = verts + (size_t)fv[1] * 3;
    const float* p2 = verts + (size_t)fv[2] * 3;
    for (int k = 0; k < 3; ++k) m[k] = best_z * ((bq0 * (double)p0[k] + bq1 * (double)p1[k]) + bq2 * (double)p2[k]);
    double c0[3], c1[3], c2[3];
    rast_camera(cam, p0, c0);
    rast_camera(cam, p1, c1);
    rast_camera(cam, p2, c2);
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
    double bd = INFINITY;
    for (int j = 0; j < NR; ++j) {
      const double dx = m[0] - s_rp[3 * j], dy = m[1] - s_rp[3 * j + 1], dz = m[2] - s_rp[3 * j + 2];
      const double d = (dx * dx + dy * dy) + dz * dz;
      if (d < bd) bd = d, reg = j + 1;
    }
  }
  face_out[o1] = best_f;
  depth[o1] = best_f >= 0 ? (float)best_z : 0.f;
  region[o1] = reg;
  for (int k = 0; k < 3; ++k) {
    coord[o3 + k * HW] = (float)m[k];
    normal[o3 + k * HW] = (float)n[k];
  }
  if (cover_frame) {
    const int row = rmin + y, col = cmin + x;  // rc is device memory too: a pixel off the frame is not written
    if (row >= 0 && row < H && col >= 0 && col < W) cover_frame[((size_t)b * H + row) * W + col] = best_f >= 0;
  }
}

// The pointwise masking of batchdataset.py:663-671, 689-694, 755-759 on the rendered maps.
__global__ void gt_maps_finish_kernel(const float* __restrict__ coord, const int* __restrict__ region_raw,
                                      const int* __restrict__ face, const unsigned char* __restrict__ point_mask,
                                      const long long* __restrict__ cls, const double* __restrict__ extent,
                                      const double* __restrict__ lfborder, int HW, float* __restrict__ xyz,
                                      float* __restrict__ normal, long long* __restrict__ region,
                                      float* __restrict__ mask, long long* __restrict__ multi_cls_mask,
                                      float* __restrict__ mask_obj) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= HW) return;
  const size_t o1 = (size_t)b * HW + p, o3 = (size_t)b * 3 * HW + p;
  const bool on = point_mask[o1] != 0;
  for (int k = 0; k < 3; ++k) {
    const size_t o = o3 + (size_t)k * HW;
    xyz[o] = on ? (float)(((double)coord[o] - lfborder[3 * b + k]) / extent[3 * b + k]) : 0.f;
    if (!on) normal[o] = 0.f;
  }
  region[o1] = on ? (long long)region_raw[o1] : 0;
  mask[o1] = on ? 1.f : 0.f;
  multi_cls_mask[o1] = on ? cls[b] + 1 : 0;
  if (mask_obj) mask_obj[o1] = face[o1] >= 0 ? 1.f : 0.f;
}

}  // namespace

KRRN_API int krrn_raster_maps_f32(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                                  const double* R, const double* t, const float* K4, const int* rc, int S,
                                  const float* region_pts, int NR, int B, int* face, float* depth, float* coord,
                                  float* normal, int* region, unsigned char* cover_frame, int H, int W,
                                  void* stream) {
  if (!verts || !faces || !face_range || !R || !t || !K4 || !rc || !region_pts || !face || !depth || !coord ||
      !normal || !region)
    return KRRN_EARG;
  if (S < 1 || S > kRastMaxS || NR < 1 || NR > kRastMaxNR || B < 1 || B > 65535 || Vtot < 1 || Ftot < 0)
    return KRRN_ESHAPE;
  if (cover_frame && (H < S || W < S)) return KRRN_ESHAPE;  // no window of S x S fits the frame
  const size_t b = (size_t)B, hw = (size_t)S * S;
  const Span outs[6] = {{face, 4 * b * hw},   {depth, 4 * b * hw},  {coord, 12 * b * hw},
                        {normal, 12 * b * hw}, {region, 4 * b * hw}, {cover_frame, cover_frame ? b * H * W : 0}};
  const Span ins[8] = {{verts, 12 * (size_t)Vtot}, {faces, 12 * (size_t)Ftot}, {face_range, 8 * b}, {R, 72 * b},
                       {t, 24 * b},                {K4, 16 * b},               {rc, 8 * b},
                       {region_pts, 12 * b * NR}};
  if (rast_overlap(outs, 6, ins, 8)) return KRRN_EARG;
  const int tiles = krrn_cdiv(S, kRastTile);
  hipLaunchKernelGGL(raster_maps_kernel, dim3(tiles, tiles, B), dim3(kRastThreads), 0, (hipStream_t)stream, verts,
                     Vtot, faces, Ftot, face_range, R, t, K4, rc, S, region_pts, NR, face, depth, coord, normal, region,
                     cover_frame, H, W);
  return krrn_launch_status();
}

KRRN_API int krrn_gt_maps_finish_f32(const float* coord, const int* region_raw, const int* face,
                                     const unsigned char* point_mask, const long long* cls, const double* extent,
                                     const double* lfborder, int B, int HW, float* xyz, float* normal,
                                     long long* region, float* mask, long long* multi_cls_mask, float* mask_obj,
                                     void* stream) {
  if (!coord || !region_raw || !point_mask || !cls || !extent || !lfborder || !xyz || !normal || !region || !mask ||
      !multi_cls_mask || (mask_obj && !face))
    return KRRN_EARG;
  if (B < 1 || B > 65535 || HW < 1 || HW > kRastMaxS * kRastMaxS) return KRRN_ESHAPE;
  const size_t n = (size_t)B * HW;
  const Span outs[6] = {{xyz, 12 * n}, {normal, 12 * n}, {region, 8 * n}, {mask, 4 * n}, {multi_cls_mask, 8 * n},
                        {mask_obj, mask_obj ? 4 * n : 0}};
  const Span ins[7] = {{coord, 12 * n}, {region_raw, 4 * n}, {face, face ? 4 * n : 0}, {point_mask, n},
                       {cls, 8 * (size_t)B}, {extent, 24 * (size_t)B}, {lfborder, 24 * (size_t)B}};
  if (rast_overlap(outs, 6, ins, 7)) return KRRN_EARG;
  hipLaunchKernelGGL(gt_maps_finish_kernel, dim3(krrn_cdiv(HW, 256), B), dim3(256), 0, (hipStream_t)stream, coord,
                     region_raw, face, point_mask, cls, extent, lfborder, HW, xyz, normal, region, mask, multi_cls_mask,
                     mask_obj);
  return krrn_launch_status();
}
