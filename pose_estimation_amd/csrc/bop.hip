// The BOP-19 pose errors (Hodan et al., ECCV-W 2020) of a batch of estimates against their GT poses:
// VSD (krrn_bop_vsd_f32) and MSSD / MSPD (krrn_bop_mssd_mspd_f32). Written from the published definition;
// include/krrn_hip.h states it, tests/bop_ref.py restates it in numpy f64 with the same operation order.
// Everything is f64 without FMA contraction (FLAGS_bop). krrn_bop_visib_u8, at the end of the VSD part, writes
// out the ground-truth visibility of B instances (silhouette, visible mask, pixel counts, boxes) with the same
// walk and the same visibility rule (bop_visible below: stated once for both).
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
#include "krrn_observe.h"

namespace {

constexpr int kBopMaxT = 16;
constexpr int kBopCounts = 2 + kBopMaxT;
constexpr int kBopSymSplit = 16;  // blocks per crop of the MSSD / MSPD kernel

// the "bop19" visibility rule of include/krrn_hip.h for one pixel: obs and model are distances from the camera
// centre, 0 = nothing observed / nothing rendered
__device__ __forceinline__ bool bop_visible(double obs, double model, double delta) {
  return (obs > 0.0 && model > 0.0 && (model - obs) <= delta) || (obs == 0.0 && model > 0.0);
}

// ws int32 [B][2][4] = (u lo, u hi, v lo, v hi) of pose 0 (estimate) and 1 (GT); lo > hi = no vertex
__global__ __launch_bounds__(kRastThreads) void bop_box_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ face_range, const double* __restrict__ R_est, const double* __restrict__ t_est,
    const double* __restrict__ R_gt, const double* __restrict__ t_gt, const float* __restrict__ K4, int NC,
    int* __restrict__ ws, int* __restrict__ counts) {
  __shared__ double s_box[kRastWaves][4];
  const int b = blockIdx.x, pose = blockIdx.y, tid = threadIdx.x;
  if (pose == 0 && tid < NC) counts[(size_t)b * NC + tid] = 0;
  RastCam cam;
  rast_load_cam(cam, pose ? R_gt : R_est, pose ? t_gt : t_est, K4, b);
  bop_project_box(cam, verts, Vtot, faces, Ftot, face_range, b, s_box, ws + ((size_t)b * 2 + pose) * 4);
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
    double ray, obs;  // K4 is the same for both poses
    bop_observe(cam, pu, pv, depth, F, H, W, frame[b], x, y, depth_scale, ray, obs);
    const double dist_est = z_est > 0.0 ? z_est * ray : 0.0;
    const double dist_gt = z_gt > 0.0 ? z_gt * ray : 0.0;
    const bool v_gt = bop_visible(obs, dist_gt, delta);
    const bool v_est = bop_visible(obs, dist_est, delta) || (v_gt && dist_est > 0.0);
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

// ------------------------------------------------------------------------------------------ GT visibility
// krrn_bop_visib_u8: VSD's structure with one pose per instance, and the result written out.
//   0. the entry point zeroes the requested planes with hipMemsetAsync, so the tiles that return early (and the
//      pixels of a walked tile that no face covers, which store their own zeros again) leave every byte defined.
//   1. bop_visib_box_kernel, one block per instance: its projected bounding box (bop_project_box) and the reset
//      of its counters and box bounds.
//   2. bop_visib_kernel, one block per 16 x 16 tile and instance: a tile outside the box returns after reading
//      4 ints; otherwise one depth walk, the observed depth, the two flags per pixel. A wave holds 4 rows of 16
//      pixels (krrn_mask.h's tile layout), so its 64-bit ballot of a flag is 4 rows of 16 bits, which
//      mask_store_row writes to the plane. The same ballots give
//      the counts (popcount) and the wave's box bounds (first / last set column and row), which go through LDS
//      and then one integer atomicAdd / atomicMin / atomicMax per block and quantity: all order-independent.
//   3. bop_visib_finish_kernel: (lo, hi) bounds to (x, y, w, h), and visib_fract.
// ws int32 [B][16] = box (u lo, u hi, v lo, v hi), counts (all, valid, visib), one unused, the bounds of mask
// (x lo, x hi, y lo, y hi), the bounds of mask_visib.
constexpr int kVisWs = 16;
constexpr int kVisLoInit = 0x7fffffff, kVisHiInit = -1;

__global__ __launch_bounds__(kRastThreads) void bop_visib_box_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ face_range, const double* __restrict__ R, const double* __restrict__ t,
    const float* __restrict__ K4, int* __restrict__ ws) {
  __shared__ double s_box[kRastWaves][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  int* o = ws + (size_t)b * kVisWs;
  if (tid >= 4 && tid < 8) o[tid] = 0;
  if (tid >= 8 && tid < kVisWs) o[tid] = (tid & 1) ? kVisHiInit : kVisLoInit;
  RastCam cam;
  rast_load_cam(cam, R, t, K4, b);
  bop_project_box(cam, verts, Vtot, faces, Ftot, face_range, b, s_box, o);
}

// one plane's stores and one box's bounds for one wave: bal = the wave's ballot of the pixel flag
__device__ __forceinline__ void bop_visib_emit(unsigned long long bal, bool inside, bool row_fast,
                                               unsigned char* __restrict__ plane, size_t pix, int lane, int lx,
                                               int wy, int* s_bounds) {
  if (plane) mask_store_row(bal, lane, inside, row_fast, plane, pix);
  if (lane == 0 && bal) {
    const unsigned cols = (unsigned)((bal | (bal >> 16) | (bal >> 32) | (bal >> 48)) & 0xffffull);
    int r0 = 0, r1 = 3;
    while (!((bal >> (16 * r0)) & 0xffffull)) ++r0;
    while (!((bal >> (16 * r1)) & 0xffffull)) --r1;
    atomicMin(&s_bounds[0], lx + (__ffs(cols) - 1));
    atomicMax(&s_bounds[1], lx + (31 - __clz(cols)));
    atomicMin(&s_bounds[2], wy + r0);
    atomicMax(&s_bounds[3], wy + r1);
  }
}

__global__ __launch_bounds__(kRastThreads) void bop_visib_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ face_range, const double* __restrict__ R, const double* __restrict__ t,
    const float* __restrict__ K4, const float* __restrict__ depth, int F, int H, int W, const int* __restrict__ frame,
    double depth_scale, double delta, int* __restrict__ ws, unsigned char* __restrict__ mask,
    unsigned char* __restrict__ mask_visib) {
  __shared__ double s_setup[kRastThreads * kRastSetup];
  __shared__ int s_id[kRastThreads];
  __shared__ int s_wcnt[kRastWaves];
  __shared__ int s_out[11];  // 3 counts, 2 x 4 bounds

  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lx = blockIdx.x * kRastTile, ly = blockIdx.y * kRastTile;
  const int tx1 = min(lx + kRastTile, W) - 1, ty1 = min(ly + kRastTile, H) - 1;
  int* o = ws + (size_t)b * kVisWs;
  if (!(o[0] <= tx1 && o[1] >= lx && o[2] <= ty1 && o[3] >= ly)) return;  // uniform: the planes are zero already

  const int x = lx + (tid & (kRastTile - 1)), y = ly + (tid >> 4);
  const bool inside = x < W && y < H;
  long long f0;
  int nf;
  rast_range(face_range, b, Ftot, f0, nf);
  const double pu = (double)x, pv = (double)y;
  RastCam cam;
  RastHit hit;
  rast_load_cam(cam, R, t, K4, b);
  rast_depth_walk(cam, verts, Vtot, faces, f0, nf, (double)lx, (double)tx1, (double)ly, (double)ty1, pu, pv, inside,
                  s_setup, s_id, s_wcnt, hit);
  if (tid < 11) s_out[tid] = tid < 3 ? 0 : (((tid - 3) & 1) ? kVisHiInit : kVisLoInit);
  __syncthreads();

  bool in_mask = false, in_valid = false, in_visib = false;
  if (inside) {
    double ray, obs;
    bop_observe(cam, pu, pv, depth, F, H, W, frame[b], x, y, depth_scale, ray, obs);
    const double z = hit.f >= 0 ? hit.z : 0.0;
    const double dist = z > 0.0 ? z * ray : 0.0;
    in_mask = z > 0.0;
    in_valid = in_mask && obs > 0.0;
    in_visib = bop_visible(obs, dist, delta);
  }
  const size_t pix = ((size_t)b * H + y) * W + x;  // used only where `inside`
  const size_t row0 = pix - (x - lx);
  const bool fast_m = mask && mask_row_fast(mask + row0, W - lx);
  const bool fast_v = mask_visib && mask_row_fast(mask_visib + row0, W - lx);
  const unsigned long long bal_m = __ballot(in_mask), bal_val = __ballot(in_valid), bal_v = __ballot(in_visib);
  const int wy = ly + kMaskWaveRows * wave;
  bop_visib_emit(bal_m, inside, fast_m, mask, pix, lane, lx, wy, s_out + 3);
  bop_visib_emit(bal_v, inside, fast_v, mask_visib, pix, lane, lx, wy, s_out + 7);
  if (lane == 0) {
    if (bal_m) atomicAdd(&s_out[0], __popcll(bal_m));
    if (bal_val) atomicAdd(&s_out[1], __popcll(bal_val));
    if (bal_v) atomicAdd(&s_out[2], __popcll(bal_v));
  }
  __syncthreads();
  if (tid < 3) {
    if (s_out[tid]) atomicAdd(&o[4 + tid], s_out[tid]);
  } else if (tid < 11) {
    const int v = s_out[tid];
    if ((tid - 3) & 1) {
      if (v != kVisHiInit) atomicMax(&o[8 + (tid - 3)], v);
    } else {
      if (v != kVisLoInit) atomicMin(&o[8 + (tid - 3)], v);
    }
  }
}

__global__ void bop_visib_finish_kernel(const int* __restrict__ ws, int B, int* __restrict__ info,
                                        double* __restrict__ visib_fract) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int* o = ws + (size_t)b * kVisWs;
  int* q = info + (size_t)b * 11;
  q[0] = o[4], q[1] = o[5], q[2] = o[6];
  for (int k = 0; k < 2; ++k) {
    const int* e = o + 8 + 4 * k;
    const bool any = o[k ? 6 : 4] > 0;
    q[3 + 4 * k] = any ? e[0] : -1, q[4 + 4 * k] = any ? e[2] : -1;
    q[5 + 4 * k] = any ? e[1] - e[0] : -1, q[6 + 4 * k] = any ? e[3] - e[2] : -1;
  }
  visib_fract[b] = o[4] > 0 ? (double)o[6] / (double)o[4] : 0.0;
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

KRRN_API int krrn_bop_visib_ws(int B, long long* n_ints) {
  if (!n_ints) return KRRN_EARG;
  if (B < 1 || B > 65535) return KRRN_ESHAPE;
  *n_ints = (long long)kVisWs * B;
  return KRRN_OK;
}

KRRN_API int krrn_bop_visib_u8(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                               const double* R, const double* t, const float* K4, const float* depth, int F, int H,
                               int W, const int* frame, double depth_scale, double delta, int B, int* ws,
                               unsigned char* mask, unsigned char* mask_visib, int* info, double* visib_fract,
                               void* stream) {
  if (!verts || !faces || !face_range || !R || !t || !K4 || !depth || !frame || !ws || !info || !visib_fract)
    return KRRN_EARG;
  if (B < 1 || B > 65535 || Vtot < 1 || Ftot < 0 || F < 1 || H < 1 || W < 1 || H > 65535 * kRastTile ||
      W > 65535 * kRastTile || !(delta > 0.0) || !(depth_scale > 0.0))
    return KRRN_ESHAPE;
  const size_t b = (size_t)B, plane = b * H * W;
  const Span outs[5] = {{ws, 4 * b * kVisWs}, {mask, mask ? plane : 0}, {mask_visib, mask_visib ? plane : 0},
                        {info, 44 * b},       {visib_fract, 8 * b}};
  const Span ins[8] = {{verts, 12 * (size_t)Vtot}, {faces, 12 * (size_t)Ftot}, {face_range, 8 * b}, {R, 72 * b},
                       {t, 24 * b},                {K4, 16 * b},               {depth, 4 * (size_t)F * H * W},
                       {frame, 4 * b}};
  if (rast_overlap(outs, 5, ins, 8)) return KRRN_EARG;
  hipStream_t st = (hipStream_t)stream;
  for (unsigned char* p : {mask, mask_visib}) {
    const hipError_t e = p ? hipMemsetAsync(p, 0, plane, st) : hipSuccess;
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(bop_visib_box_kernel, dim3(B), dim3(kRastThreads), 0, st, verts, Vtot, faces, Ftot, face_range, R,
                     t, K4, ws);
  hipLaunchKernelGGL(bop_visib_kernel, dim3(krrn_cdiv(W, kRastTile), krrn_cdiv(H, kRastTile), B), dim3(kRastThreads), 0,
                     st, verts, Vtot, faces, Ftot, face_range, R, t, K4, depth, F, H, W, frame, depth_scale, delta, ws,
                     mask, mask_visib);
  hipLaunchKernelGGL(bop_visib_finish_kernel, dim3(krrn_cdiv(B, 256)), dim3(256), 0, st, ws, B, info, visib_fract);
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
