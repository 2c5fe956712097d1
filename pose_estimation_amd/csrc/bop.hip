// The BOP-19 pose errors (Hodan et al., ECCV-W 2020) of a batch of estimates against their GT poses:
// VSD (krrn_bop_vsd_f32) and MSSD / MSPD (krrn_bop_mssd_mspd_f32). Written from the published definition;
// include/krrn_hip.h states it, tests/bop_ref.py restates it in numpy f64 with the same operation order.
// Everything is f64 without FMA contraction (FLAGS_bop).
//
// VSD renders the mesh twice per crop, under the estimated and the GT pose, over the whole H x W frame with
// the GT-map rasteriser's depth walk (krrn_raster.h: the same face test, skip rules, strict < and
// lowest-index tie rule), and compares both with the observed depth frame. Three launches:
//   1. bop_box_kernel, one block per (crop, pose): the bounding box of the projected vertices of the crop's
//      faces (vertices with z > 1e-3 only: a face with a nearer vertex is skipped whole, so the box holds
//      every drawn face), as 4 ints rounded outwards; it also zeroes the crop's counts.
//   2. bop_vsd_kernel, one block per 16 x 16 tile of the frame and crop: a tile outside both boxes returns
//      after reading the 8 ints (most of a 640 x 480 frame's 1200 tiles for a LineMOD object); otherwise
//      the depth walk runs for the poses whose box touches the tile, reusing one LDS face list, each
//      thread keeps its pixel's two depths in registers, reads the observed depth, and the block's 2 + T
//      counts (wave ballots, then LDS) are added to the crop's with integer atomicAdd. Neither depth image
//      is written to memory.
//   3. bop_vsd_finish_kernel: e_vsd from the counts.
// Integer addition is associative, so the counts do not depend on the order in which the tiles arrive: the
// result is deterministic, bit for bit, and a crop's does not depend on the rest of the batch.
//
// MSSD / MSPD: kBopSymSplit blocks per crop, block g walking the g-th contiguous slice of the crop's
// symmetries in order (a continuous axis gives 315 of them: one block would walk 315 x V pairs alone while
// the rest of the chip idles). Per symmetry every thread takes the maximum over its share of the vertices,
// the block reduces it (max does not depend on order), and thread 0 keeps the slice's running minimum with a
// strict <; a second one-thread-per-crop launch takes the minimum over the slices in order, again with a
// strict <, i.e. the lowest symmetry index on ties. With one symmetry (every object of a stock LineMOD tree)
// the other blocks of the crop return at once.
#include "krrn_raster.h"

namespace {

constexpr int kBopMaxT = 16;
constexpr int kBopCounts = 2 + kBopMaxT;
constexpr int kBopSymSplit = 16;  // blocks per crop of the MSSD / MSPD kernel
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

// ws int32 [B][2][4] = (u lo, u hi, v lo, v hi) of pose 0 (estimate) and 1 (GT); lo > hi = no vertex
__global__ __launch_bounds__(kRastThreads) void bop_box_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ face_range, const double* __restrict__ R_est, const double* __restrict__ t_est,
    const double* __restrict__ R_gt, const double* __restrict__ t_gt, const float* __restrict__ K4, int NC,
    int* __restrict__ ws, int* __restrict__ counts) {
  __shared__ double s_box[kRastWaves][4];
  const int b = blockIdx.x, pose = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  if (pose == 0 && tid < NC) counts[(size_t)b * NC + tid] = 0;
  RastCam cam;
  rast_load_cam(cam, pose ? R_gt : R_est, pose ? t_gt : t_est, K4, b);
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
    int* o = ws + ((size_t)b * 2 + pose) * 4;
    const bool any = umin <= umax && vmin <= vmax;
    auto lo = [](double x) { return (int)fmax(fmin(floor(x), kBopBoxClamp), -kBopBoxClamp); };
    auto hi = [](double x) { return (int)fmax(fmin(ceil(x), kBopBoxClamp), -kBopBoxClamp); };
    o[0] = any ? lo(umin) : kBopBoxEmptyLo, o[1] = any ? hi(umax) : kBopBoxEmptyHi;
    o[2] = any ? lo(vmin) : kBopBoxEmptyLo, o[3] = any ? hi(vmax) : kBopBoxEmptyHi;
  }
}

__global__ __launch_bounds__(kRastThreads) void bop_vsd_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ face_range, const double* __restrict__ R_est, const double* __restrict__ t_est,
    const double* __restrict__ R_gt, const double* __restrict__ t_gt, const float* __restrict__ K4,
    const float* __restrict__ depth, int F, int H, int W, const int* __restrict__ frame, double depth_scale,
    const double* __restrict__ diameter, double delta, const double* __restrict__ taus, int T,
    const int* __restrict__ ws, int* __restrict__ counts) {
  __shared__ double s_setup[kRastThreads * kRastSetup];
  __shared__ int s_id[kRastThreads];
  __shared__ int s_wcnt[kRastWaves];
  __shared__ int s_cnt[kBopCounts];

  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
  const int lx = blockIdx.x * kRastTile, ly = blockIdx.y * kRastTile;
  const int tx1 = min(lx + kRastTile, W) - 1, ty1 = min(ly + kRastTile, H) - 1;
  const int* bx = ws + (size_t)b * 8;
  const bool touch_e = bx[0] <= tx1 && bx[1] >= lx && bx[2] <= ty1 && bx[3] >= ly;
  const bool touch_g = bx[4] <= tx1 && bx[5] >= lx && bx[6] <= ty1 && bx[7] >= ly;
  if (!touch_e && !touch_g) return;  // uniform over the block: no face of either render reaches this tile

  const int x = lx + (tid & (kRastTile - 1)), y = ly + (tid >> 4);
  const bool inside = x < W && y < H;
  long long f0;
  int nf;
  rast_range(face_range, b, Ftot, f0, nf);
  const double pu = (double)x, pv = (double)y;  // the whole frame: rmin = cmin = 0
  const double tu0 = (double)lx, tu1 = (double)tx1, tv0 = (double)ly, tv1 = (double)ty1;

  RastCam cam;
  RastHit hit;
  double z_est = 0.0, z_gt = 0.0;  // a pixel that no face covers has depth 0
  if (touch_e) {
    rast_load_cam(cam, R_est, t_est, K4, b);
    rast_depth_walk(cam, verts, Vtot, faces, f0, nf, tu0, tu1, tv0, tv1, pu, pv, inside, s_setup, s_id, s_wcnt, hit);
    if (hit.f >= 0) z_est = hit.z;
  }
  if (touch_g) {
    rast_load_cam(cam, R_gt, t_gt, K4, b);
    rast_depth_walk(cam, verts, Vtot, faces, f0, nf, tu0, tu1, tv0, tv1, pu, pv, inside, s_setup, s_id, s_wcnt, hit);
    if (hit.f >= 0) z_gt = hit.z;
  }
  const int NC = 2 + T;
  if (tid < NC) s_cnt[tid] = 0;
  __syncthreads();

  bool in_union = false, in_inter = false;
  double cost = 0.0;
  if (inside) {
    const double xn = (pu - cam.cx) / cam.fx, yn = (pv - cam.cy) / cam.fy;  // K4 is the same for both poses
    const double ray = sqrt((xn * xn + yn * yn) + 1.0);
    const int fr = frame[b];
    double d_obs = 0.0;
    if (fr >= 0 && fr < F) d_obs = (double)depth[((size_t)fr * H + y) * W + x] / depth_scale;
    const double obs = d_obs > 0.0 ? d_obs * ray : 0.0;  // also for a negative or NaN sample
    const double dist_est = z_est > 0.0 ? z_est * ray : 0.0;
    const double dist_gt = z_gt > 0.0 ? z_gt * ray : 0.0;
    const bool v_gt = (obs > 0.0 && dist_gt > 0.0 && (dist_gt - obs) <= delta) || (obs == 0.0 && dist_gt > 0.0);
    const bool v_est = (obs > 0.0 && dist_est > 0.0 && (dist_est - obs) <= delta) ||
                       (obs == 0.0 && dist_est > 0.0) || (v_gt && dist_est > 0.0);
    in_inter = v_gt && v_est;
    in_union = v_gt || v_est;
    cost = fabs(dist_gt - dist_est) / diameter[b];
  }
  for (int c = 0; c < NC; ++c) {
    const bool flag = c == 0 ? in_union : c == 1 ? in_inter : (in_inter && cost >= taus[c - 2]);
    const unsigned long long bal = __ballot(flag);
    if (lane == 0 && bal) atomicAdd(&s_cnt[c], __popcll(bal));
  }
  __syncthreads();
  if (tid < NC && s_cnt[tid]) atomicAdd(&counts[(size_t)b * NC + tid], s_cnt[tid]);
}

__global__ void bop_vsd_finish_kernel(const int* __restrict__ counts, int B, int T, double* __restrict__ e_vsd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * T) return;
  const int b = i / T, k = i - b * T;
  const int* c = counts + (size_t)b * (2 + T);
  const int un = c[0], in = c[1], step = c[2 + k];
  e_vsd[i] = un > 0 ? (double)(step + (un - in)) / (double)un : 1.0;
}

__global__ __launch_bounds__(kRastThreads) void bop_mssd_mspd_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ vert_range, const double* __restrict__ R_est,
    const double* __restrict__ t_est, const double* __restrict__ R_gt, const double* __restrict__ t_gt,
    const float* __restrict__ K4, const double* __restrict__ syms, int NStot, const int* __restrict__ sym_range,
    int B, double* __restrict__ ws) {
  __shared__ double s_max[kRastWaves][2];
  const int b = blockIdx.x, g = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  RastCam ce, cg;
  rast_load_cam(ce, R_est, t_est, K4, b);
  rast_load_cam(cg, R_gt, t_gt, K4, b);
  long long v0, s0;
  int nv, ns;
  rast_range(vert_range, b, Vtot, v0, nv);
  rast_range(sym_range, b, NStot, s0, ns);
  double best3 = INFINITY, best2 = INFINITY;  // thread 0's running minima over this block's slice
  int idx3 = -1, idx2 = -1;
  if (nv == 0) ns = 0;
  const int per = krrn_cdiv(ns, kBopSymSplit);
  const int s_hi = min(ns, (g + 1) * per);
  for (int s = g * per; s < s_hi; ++s) {  // uniform over the block
    const double* S = syms + (size_t)(s0 + s) * 12;
    double m3 = 0.0, m2 = 0.0;
    for (int i = tid; i < nv; i += kRastThreads) {
      const float* p = verts + (size_t)(v0 + i) * 3;
      const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
      double e[3], g[3];
      rast_camera(ce, p, e);
      const double sx = ((S[0] * x + S[1] * y) + S[2] * z) + S[9];
      const double sy = ((S[3] * x + S[4] * y) + S[5] * z) + S[10];
      const double sz = ((S[6] * x + S[7] * y) + S[8] * z) + S[11];
      g[0] = ((cg.r[0] * sx + cg.r[1] * sy) + cg.r[2] * sz) + cg.t[0];
      g[1] = ((cg.r[3] * sx + cg.r[4] * sy) + cg.r[5] * sz) + cg.t[1];
      g[2] = ((cg.r[6] * sx + cg.r[7] * sy) + cg.r[8] * sz) + cg.t[2];
      const double dx = e[0] - g[0], dy = e[1] - g[1], dz = e[2] - g[2];
      double d3 = sqrt((dx * dx + dy * dy) + dz * dz);
      const double du = (ce.fx * e[0] / e[2] + ce.cx) - (cg.fx * g[0] / g[2] + cg.cx);
      const double dv = (ce.fy * e[1] / e[2] + ce.cy) - (cg.fy * g[1] / g[2] + cg.cy);
      double d2 = sqrt(du * du + dv * dv);
      if (!(d3 == d3)) d3 = INFINITY;  // a NaN distance counts as +inf, so that max stays order-free
      if (!(d2 == d2)) d2 = INFINITY;
      m3 = fmax(m3, d3), m2 = fmax(m2, d2);
    }
    m3 = bop_wave_max(m3), m2 = bop_wave_max(m2);
    if (lane == 0) s_max[wave][0] = m3, s_max[wave][1] = m2;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kRastWaves; ++w) m3 = fmax(m3, s_max[w][0]), m2 = fmax(m2, s_max[w][1]);
      if (m3 < best3) best3 = m3, idx3 = s;
      if (m2 < best2) best2 = m2, idx2 = s;
    }
    __syncthreads();  // the next symmetry rewrites s_max
  }
  if (tid == 0) {  // ws = f64 [B][split][2] minima, then int32 [B][split][2] their symmetry indices
    const size_t o = ((size_t)b * kBopSymSplit + g) * 2;
    int* wi = reinterpret_cast<int*>(ws + (size_t)B * kBopSymSplit * 2);
    ws[o] = best3, ws[o + 1] = best2;
    wi[o] = idx3, wi[o + 1] = idx2;
  }
}

__global__ void bop_mssd_mspd_finish_kernel(const double* __restrict__ ws, int B, double* __restrict__ mssd,
                                            double* __restrict__ mspd, int* __restrict__ sym_idx) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int* wi = reinterpret_cast<const int*>(ws + (size_t)B * kBopSymSplit * 2);
  double best3 = INFINITY, best2 = INFINITY;
  int idx3 = -1, idx2 = -1;
  for (int g = 0; g < kBopSymSplit; ++g) {  // the slices in symmetry order: the lowest index on ties
    const size_t o = ((size_t)b * kBopSymSplit + g) * 2;
    if (ws[o] < best3) best3 = ws[o], idx3 = wi[o];
    if (ws[o + 1] < best2) best2 = ws[o + 1], idx2 = wi[o + 1];
  }
  mssd[b] = best3, mspd[b] = best2;
  if (sym_idx) sym_idx[2 * b] = idx3, sym_idx[2 * b + 1] = idx2;
}

}  // namespace

KRRN_API int krrn_bop_vsd_ws(int B, long long* n_ints) {
  if (!n_ints) return KRRN_EARG;
  if (B < 1 || B > 65535) return KRRN_ESHAPE;
  *n_ints = 8ll * B;
  return KRRN_OK;
}

KRRN_API int krrn_bop_vsd_f32(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                              const double* R_est, const double* t_est, const double* R_gt, const double* t_gt,
                              const float* K4, const float* depth, int F, int H, int W, const int* frame,
                              double depth_scale, const double* diameter, double delta, const double* taus, int T,
                              int B, int* ws, int* counts, double* e_vsd, void* stream) {
  if (!verts || !faces || !face_range || !R_est || !t_est || !R_gt || !t_gt || !K4 || !depth || !frame || !diameter ||
      !taus || !ws || !counts || !e_vsd)
    return KRRN_EARG;
  if (B < 1 || B > 65535 || Vtot < 1 || Ftot < 0 || F < 1 || H < 1 || W < 1 || H > 65535 * kRastTile ||
      W > 65535 * kRastTile || T < 1 || T > kBopMaxT || !(delta > 0.0) || !(depth_scale > 0.0))
    return KRRN_ESHAPE;
  const size_t b = (size_t)B;
  const Span outs[3] = {{ws, 32 * b}, {counts, 4 * b * (2 + T)}, {e_vsd, 8 * b * T}};
  const Span ins[12] = {{verts, 12 * (size_t)Vtot}, {faces, 12 * (size_t)Ftot}, {face_range, 8 * b}, {R_est, 72 * b},
                        {t_est, 24 * b},            {R_gt, 72 * b},             {t_gt, 24 * b},      {K4, 16 * b},
                        {depth, 4 * (size_t)F * H * W}, {frame, 4 * b},         {diameter, 8 * b},
                        {taus, 8 * (size_t)T}};
  if (rast_overlap(outs, 3, ins, 12)) return KRRN_EARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bop_box_kernel, dim3(B, 2), dim3(kRastThreads), 0, st, verts, Vtot, faces, Ftot, face_range,
                     R_est, t_est, R_gt, t_gt, K4, 2 + T, ws, counts);
  hipLaunchKernelGGL(bop_vsd_kernel, dim3(krrn_cdiv(W, kRastTile), krrn_cdiv(H, kRastTile), B), dim3(kRastThreads), 0,
                     st, verts, Vtot, faces, Ftot, face_range, R_est, t_est, R_gt, t_gt, K4, depth, F, H, W, frame,
                     depth_scale, diameter, delta, taus, T, ws, counts);
  hipLaunchKernelGGL(bop_vsd_finish_kernel, dim3(krrn_cdiv(B * T, 256)), dim3(256), 0, st, counts, B, T, e_vsd);
  return krrn_launch_status();
}

KRRN_API int krrn_bop_mssd_mspd_ws(int B, long long* n_doubles) {
  if (!n_doubles) return KRRN_EARG;
  if (B < 1) return KRRN_ESHAPE;
  *n_doubles = 3ll * B * kBopSymSplit;  // two f64 minima and two int32 indices per (crop, slice)
  return KRRN_OK;
}

KRRN_API int krrn_bop_mssd_mspd_f32(const float* verts, int Vtot, const int* vert_range, const double* R_est,
                                    const double* t_est, const double* R_gt, const double* t_gt, const float* K4,
                                    const double* syms, int NStot, const int* sym_range, int B, double* ws,
                                    double* mssd, double* mspd, int* sym_idx, void* stream) {
  if (!verts || !vert_range || !R_est || !t_est || !R_gt || !t_gt || !K4 || !syms || !sym_range || !ws || !mssd ||
      !mspd)
    return KRRN_EARG;
  if (B < 1 || Vtot < 1 || NStot < 1) return KRRN_ESHAPE;
  const size_t b = (size_t)B;
  const Span outs[4] = {{mssd, 8 * b}, {mspd, 8 * b}, {sym_idx, sym_idx ? 8 * b : 0}, {ws, 24 * b * kBopSymSplit}};
  const Span ins[9] = {{verts, 12 * (size_t)Vtot}, {vert_range, 8 * b}, {R_est, 72 * b}, {t_est, 24 * b},
                       {R_gt, 72 * b},             {t_gt, 24 * b},      {K4, 16 * b},    {syms, 96 * (size_t)NStot},
                       {sym_range, 8 * b}};
  if (rast_overlap(outs, 4, ins, 9)) return KRRN_EARG;
  hipLaunchKernelGGL(bop_mssd_mspd_kernel, dim3(B, kBopSymSplit), dim3(kRastThreads), 0, (hipStream_t)stream, verts,
                     Vtot, vert_range, R_est, t_est, R_gt, t_gt, K4, syms, NStot, sym_range, B, ws);
  hipLaunchKernelGGL(bop_mssd_mspd_finish_kernel, dim3(krrn_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, ws, B,
                     mssd, mspd, sym_idx);
  return krrn_launch_status();
}
