// Whole scenes in one z-buffer, and the pictures made from them (include/krrn_hip.h states the definitions;
// tests/scene_ref.py restates them in numpy):
//   krrn_scene_render_f64     all instances of a frame, each under its own pose, drawn into one depth buffer with one
//                             object hiding another: per pixel the winning instance, its depth and a flat shade
//   krrn_scene_overlay_u8     the shaded, tinted estimates blended over the RGB frames, with outlines (integer work)
//   krrn_scene_depth_diff_u8  the signed difference between a rendered and an observed depth plane as colours
// The render is f64 without FMA contraction (FLAGS_scene), on krrn_raster.h's depth walk. Two launches:
//   1. scene_box_kernel, one block per instance: the bounding box of its projected vertices (bop_project_box) into
//      ws, 4 ints per instance.
//   2. scene_tile_kernel, one block per 16 x 16 tile of a frame, frames on gridDim.y. The frame's instances are
//      taken in increasing index; one whose box misses the tile is skipped (block-uniform), the others run one depth
//      walk each on one LDS face list, and every thread keeps its pixel's best (depth, instance, face) in registers
//      under a strict <. The winner's normal is formed once per pixel after the loop; then the three stores. A tile
//      that no instance reaches stores -1 / 0 / 0 without a walk. Every pixel is stored: no memset.
// The cull changes no output: the walk keeps a face only if all three of its vertices are in front of the near
// plane and the face's own bounding box reaches the tile's sample points; the instance's box is the outward-rounded
// hull of every such vertex's projection, computed by the walk's own expressions (the same bits), so a tile that the
// instance's box misses is missed by every face the walk could keep.
// No atomics, no block waits for another, nothing is read back; a frame's planes are written by its own blocks from
// its own instances alone, so they do not depend on the rest of the batch, bit for bit.
#include "krrn_observe.h"

namespace {

constexpr int kSceneThreads = 256;
constexpr int kSceneMaxBlocks = 1 << 20;  // of the per-pixel kernels: more pixels than that share threads

__global__ __launch_bounds__(kRastThreads) void scene_box_kernel(const float* __restrict__ verts, int Vtot,
                                                                 const int* __restrict__ faces, int Ftot,
                                                                 const int* __restrict__ face_range,
                                                                 const double* __restrict__ R,
                                                                 const double* __restrict__ t,
                                                                 const float* __restrict__ K4, int* __restrict__ ws) {
  __shared__ double s_box[kRastWaves][4];
  const int n = blockIdx.x;
  RastCam cam;
  rast_load_cam(cam, R, t, K4, n);
  bop_project_box(cam, verts, Vtot, faces, Ftot, face_range, n, s_box, ws + (size_t)n * 4);
}

__global__ __launch_bounds__(kRastThreads) void scene_tile_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ face_range, const double* __restrict__ R, const double* __restrict__ t,
    const float* __restrict__ K4, const int* __restrict__ inst_range, int N, int F, int H, int W, int tiles_x,
    const int* __restrict__ ws, int* __restrict__ inst, float* __restrict__ depth, unsigned char* __restrict__ shade) {
  __shared__ double s_setup[kRastThreads * kRastSetup];
  __shared__ int s_id[kRastThreads];
  __shared__ int s_wcnt[kRastWaves];

  const int tid = threadIdx.x;
  const int tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
  const int lx = txi * kRastTile, ly = tyi * kRastTile;
  const int tx1 = min(lx + kRastTile, W) - 1, ty1 = min(ly + kRastTile, H) - 1;
  const int x = lx + (tid & (kRastTile - 1)), y = ly + (tid >> 4);
  const bool inside = x < W && y < H;
  const double pu = (double)x, pv = (double)y;  // the whole frame: rmin = cmin = 0
  const double tu0 = (double)lx, tu1 = (double)tx1, tv0 = (double)ly, tv1 = (double)ty1;

  for (int f = blockIdx.y; f < F; f += gridDim.y) {  // uniform over the block
    long long n0;
    int cnt;
    rast_range(inst_range, f, N, n0, cnt);
    double best_z = INFINITY;
    int best_n = -1, best_face = -1;  // the winner's index in the whole list, its face's in `faces`
    for (int i = 0; i < cnt; ++i) {   // uniform; increasing n: equal depths stay with the lowest instance
      const int n = (int)n0 + i;
      const int* bx = ws + (size_t)n * 4;
      if (!(bx[0] <= tx1 && bx[1] >= lx && bx[2] <= ty1 && bx[3] >= ly)) continue;  // uniform: the box misses the tile
      long long f0;
      int nf;
      rast_range(face_range, n, Ftot, f0, nf);
      RastCam cam;
      rast_load_cam(cam, R, t, K4, n);
      RastHit hit;
      rast_depth_walk(cam, verts, Vtot, faces, f0, nf, tu0, tu1, tv0, tv1, pu, pv, inside, s_setup, s_id, s_wcnt, hit);
      if (inside && hit.f >= 0 && hit.z < best_z) best_z = hit.z, best_n = n, best_face = (int)(f0 + hit.f);
    }
    if (!inside) continue;
    unsigned char sh = 0;
    if (best_n >= 0) {
      RastCam cam;
      rast_load_cam(cam, R, t, K4, best_n);
      double nrm[3];
      rast_face_normal(cam, verts, faces + (size_t)best_face * 3, nrm);  // a zero normal: lam = 0
      const double lam = fmin(fmax(-nrm[2], 0.0), 1.0);
      const double s = 64.0 + 191.0 * lam;
      sh = (unsigned char)(int)(s + 0.5);
    }
    const size_t pix = ((size_t)f * H + y) * W + x;
    inst[pix] = best_n;
    depth[pix] = best_n >= 0 ? (float)best_z : 0.0f;
    shade[pix] = sh;
  }
}

// an id plane's value at p, ids outside [0, limit) as -1 (limit < 0: the plane as it stands)
__device__ __forceinline__ int scene_id(const int* __restrict__ L, size_t p, int limit) {
  const int v = L[p];
  return limit >= 0 && (v < 0 || v >= limit) ? -1 : v;
}

// L[p] >= 0 and some q with |dx|, |dy| <= radius inside the frame has L[q] != L[p]; `base` = the frame's first pixel
__device__ __forceinline__ bool scene_edge(const int* __restrict__ L, size_t base, int x, int y, int H, int W,
                                           int radius, int limit) {
  const int c = scene_id(L, base + (size_t)y * W + x, limit);
  if (c < 0) return false;
  const int y0 = max(y - radius, 0), y1 = min(y + radius, H - 1);
  const int x0 = max(x - radius, 0), x1 = min(x + radius, W - 1);
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx)
      if (scene_id(L, base + (size_t)yy * W + xx, limit) != c) return true;
  return false;
}

__global__ __launch_bounds__(kSceneThreads) void scene_overlay_kernel(
    const unsigned char* __restrict__ rgb, const int* __restrict__ est, const unsigned char* __restrict__ shade,
    const unsigned char* __restrict__ tint, int N, int alpha, int radius, const int* __restrict__ gt, int gt_r,
    int gt_g, int gt_b, size_t total, int H, int W, unsigned char* __restrict__ out) {
  const size_t plane = (size_t)H * W;
  for (size_t p = (size_t)blockIdx.x * kSceneThreads + threadIdx.x; p < total; p += (size_t)gridDim.x * kSceneThreads) {
    const size_t base = p / plane * plane;
    const int q = (int)(p - base), y = q / W, x = q - y * W;
    int c[3] = {rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]};
    const int e = scene_id(est, p, N);
    if (e >= 0) {
      const int s = shade[p];
      for (int k = 0; k < 3; ++k) {
        const int lit = (tint[3 * e + k] * s + 127) / 255;
        c[k] = (c[k] * (256 - alpha) + lit * alpha + 128) >> 8;
      }
      if (scene_edge(est, base, x, y, H, W, radius, N))
        for (int k = 0; k < 3; ++k) c[k] = tint[3 * e + k];
    }
    if (gt && scene_edge(gt, base, x, y, H, W, radius, -1)) c[0] = gt_r, c[1] = gt_g, c[2] = gt_b;
    for (int k = 0; k < 3; ++k) out[3 * p + k] = (unsigned char)c[k];
  }
}

__global__ __launch_bounds__(kSceneThreads) void scene_depth_diff_kernel(const float* __restrict__ ren,
                                                                         const float* __restrict__ obs,
                                                                         double depth_scale, double tol, size_t total,
                                                                         unsigned char* __restrict__ out) {
  for (size_t p = (size_t)blockIdx.x * kSceneThreads + threadIdx.x; p < total; p += (size_t)gridDim.x * kSceneThreads) {
    const double r = (double)ren[p], o = (double)obs[p] / depth_scale;
    int c0 = 0, c1 = 0, c2 = 0;  // nothing rendered (a NaN is never > 0)
    if (r > 0.0 && o > 0.0) {
      const double e = r - o;
      const int k = (int)(fmin(fabs(e) / tol, 1.0) * 255.0 + 0.5);
      c0 = c1 = c2 = 255;
      if (e > 0.0) c1 = c2 = 255 - k;       // the model is behind the observed surface
      else if (e < 0.0) c0 = c1 = 255 - k;  // in front of it
    } else if (r > 0.0) {
      c0 = c1 = c2 = 128;                   // rendered, nothing observed
    }
    out[3 * p] = (unsigned char)c0, out[3 * p + 1] = (unsigned char)c1, out[3 * p + 2] = (unsigned char)c2;
  }
}

// `elems` elements of `size` bytes from p as a span, cut off where the address space ends (no wrap in the check)
static Span scene_span(const void* p, size_t elems, size_t size) {
  const size_t room = ~(size_t)0 - (size_t)(uintptr_t)p;
  size_t n;
  if (__builtin_mul_overflow(elems, size, &n) || n > room) n = room;
  return {p, n};
}

// F H W, saturated: every frame count fits after the H W <= INT32_MAX check except on overflow of the product
static size_t scene_pixels(int F, int H, int W) {
  size_t n;
  return __builtin_mul_overflow((size_t)F, (size_t)H * (size_t)W, &n) ? ~(size_t)0 : n;
}

static bool scene_bad_frames(int F, int H, int W) {
  return F < 1 || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffll;
}

static int scene_blocks(size_t total) {
  const size_t b = (total - 1) / kSceneThreads + 1;
  return (int)(b < (size_t)kSceneMaxBlocks ? b : (size_t)kSceneMaxBlocks);
}

}  // namespace

KRRN_API int krrn_scene_render_ws(int N, long long* n_ints) {
  if (!n_ints) return KRRN_EARG;
  if (N < 0) return KRRN_ESHAPE;
  *n_ints = 4ll * N;
  return KRRN_OK;
}

KRRN_API int krrn_scene_render_f64(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                                   const double* R, const double* t, const float* K4, const int* inst_range, int N,
                                   int F, int H, int W, int* ws, int* inst, float* depth, unsigned char* shade,
                                   void* stream) {
  if (!verts || !faces || !face_range || !R || !t || !K4 || !inst_range || !ws || !inst || !depth || !shade)
    return KRRN_EARG;
  if (N < 0 || Vtot < 1 || Ftot < 0 || scene_bad_frames(F, H, W)) return KRRN_ESHAPE;
  const size_t n = (size_t)N, pixels = scene_pixels(F, H, W);
  const Span outs[4] = {scene_span(ws, n, 16), scene_span(inst, pixels, 4), scene_span(depth, pixels, 4),
                        scene_span(shade, pixels, 1)};
  const Span ins[7] = {scene_span(verts, (size_t)Vtot, 12), scene_span(faces, (size_t)Ftot, 12),
                       scene_span(face_range, n, 8),        scene_span(R, n, 72),
                       scene_span(t, n, 24),                scene_span(K4, n, 16),
                       scene_span(inst_range, (size_t)F, 8)};
  if (rast_overlap(outs, 4, ins, 7)) return KRRN_EARG;
  hipStream_t st = (hipStream_t)stream;
  if (N > 0)
    hipLaunchKernelGGL(scene_box_kernel, dim3(N), dim3(kRastThreads), 0, st, verts, Vtot, faces, Ftot, face_range, R, t,
                       K4, ws);
  const int tiles_x = krrn_cdiv(W, kRastTile), tiles_y = krrn_cdiv(H, kRastTile);  // tiles_x * tiles_y <= H * W
  hipLaunchKernelGGL(scene_tile_kernel, dim3(tiles_x * tiles_y, F < kMaskMaxY ? F : kMaskMaxY), dim3(kRastThreads), 0,
                     st, verts, Vtot, faces, Ftot, face_range, R, t, K4, inst_range, N, F, H, W, tiles_x, ws, inst,
                     depth, shade);
  return krrn_launch_status();
}

KRRN_API int krrn_scene_overlay_u8(const unsigned char* rgb, const int* est, const unsigned char* shade,
                                   const unsigned char* tint, int N, int alpha, int radius, const int* gt, int gt_r,
                                   int gt_g, int gt_b, int F, int H, int W, unsigned char* out, void* stream) {
  if (!rgb || !est || !shade || !tint || !out) return KRRN_EARG;
  if (N < 0 || scene_bad_frames(F, H, W) || alpha < 0 || alpha > 256 || radius < 1 || radius > 4 || gt_r < 0 ||
      gt_r > 255 || gt_g < 0 || gt_g > 255 || gt_b < 0 || gt_b > 255)
    return KRRN_ESHAPE;
  const size_t pixels = scene_pixels(F, H, W);
  const Span outs[1] = {scene_span(out, pixels, 3)};
  const Span ins[5] = {scene_span(rgb, pixels, 3), scene_span(est, pixels, 4), scene_span(shade, pixels, 1),
                       scene_span(tint, (size_t)N, 3), scene_span(gt, gt ? pixels : 0, 4)};
  if (rast_overlap(outs, 1, ins, 5)) return KRRN_EARG;
  hipLaunchKernelGGL(scene_overlay_kernel, dim3(scene_blocks(pixels)), dim3(kSceneThreads), 0, (hipStream_t)stream, rgb,
                     est, shade, tint, N, alpha, radius, gt, gt_r, gt_g, gt_b, pixels, H, W, out);
  return krrn_launch_status();
}

KRRN_API int krrn_scene_depth_diff_u8(const float* ren, const float* obs, double depth_scale, double tol, int F, int H,
                                      int W, unsigned char* out, void* stream) {
  if (!ren || !obs || !out) return KRRN_EARG;
  if (scene_bad_frames(F, H, W) || !(tol > 0.0) || !isfinite(tol) || depth_scale == 0.0) return KRRN_ESHAPE;
  const size_t pixels = scene_pixels(F, H, W);
  const Span outs[1] = {scene_span(out, pixels, 3)};
  const Span ins[2] = {scene_span(ren, pixels, 4), scene_span(obs, pixels, 4)};
  if (rast_overlap(outs, 1, ins, 2)) return KRRN_EARG;
  hipLaunchKernelGGL(scene_depth_diff_kernel, dim3(scene_blocks(pixels)), dim3(kSceneThreads), 0, (hipStream_t)stream,
                     ren, obs, depth_scale, tol, pixels, out);
  return krrn_launch_status();
}
