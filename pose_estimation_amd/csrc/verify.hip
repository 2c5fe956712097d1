// Pose verification by render-and-compare (krrn_pose_score_f32): C candidate poses per crop are scored against
// the observed depth frame and the detector's mask, without a ground-truth pose, and the best is selected.
// include/krrn_hip.h states the definition; tests/verify_ref.py restates it in numpy f64 with the same operation
// order. Everything is f64 without FMA contraction (FLAGS_verify); all sums are integer.
//
// The structure is VSD's (bop.hip), with C poses per crop instead of two. Three launches:
//   1. verify_box_kernel, one block per (crop, candidate): the bounding box of the projected vertices of the
//      crop's faces under that candidate (bop_project_box), and the reset of the pair's six counts.
//   2. verify_score_kernel, one block per 16 x 16 tile of the frame and crop: the observed distance and the mask
//      byte are read once per pixel; a tile that touches neither the crop's box nor any candidate's box returns
//      at once. Otherwise, per candidate: one whose box misses the tile adds only the tile's evidence count;
//      the others run one depth walk each (reusing one LDS face list), and their five flags go through wave
//      ballots into LDS ints. One integer atomicAdd per non-zero (candidate, count) of the tile at the end.
//   3. verify_finish_kernel, one thread per crop: union, score, best, and the winner's pose as f32.
// Integer addition is associative: the counts do not depend on the order in which the tiles arrive, so the
// result is deterministic and a (crop, candidate) pair's does not depend on the batch or on the other candidates.
#include "krrn_observe.h"

namespace {

constexpr int kVerMaxC = 8;
constexpr int kVerCounts = 6;  // render, claim, evid, both, inter, union
constexpr int kVerFlags = 5;   // the tile kernel's share: union is the finish kernel's

// ws int32 [B][C][4] = (u lo, u hi, v lo, v hi) of candidate c of crop b; lo > hi = no vertex
__global__ __launch_bounds__(kRastThreads) void verify_box_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ face_range, const double* __restrict__ R, const double* __restrict__ t, int C,
    const float* __restrict__ K4, int* __restrict__ ws, int* __restrict__ counts) {
  __shared__ double s_box[kRastWaves][4];
  const int b = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const size_t bc = (size_t)b * C + c;
  if (tid < kVerCounts) counts[bc * kVerCounts + tid] = 0;
  RastCam cam;
  rast_load_cam(cam, R + bc * 9, t + bc * 3, K4 + (size_t)b * 4, 0);
  bop_project_box(cam, verts, Vtot, faces, Ftot, face_range, b, s_box, ws + bc * 4);
}

__global__ __launch_bounds__(kRastThreads) void verify_score_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ face_range, const double* __restrict__ R, const double* __restrict__ t, int C,
    const float* __restrict__ K4, const float* __restrict__ depth, const unsigned char* __restrict__ mask, int F,
    int H, int W, const int* __restrict__ frame, const int* __restrict__ box, double depth_scale,
    const double* __restrict__ tau, const int* __restrict__ ws, int* __restrict__ counts) {
  __shared__ double s_setup[kRastThreads * kRastSetup];
  __shared__ int s_id[kRastThreads];
  __shared__ int s_wcnt[kRastWaves];
  __shared__ int s_cnt[kVerMaxC * kVerFlags];

  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
  const int lx = blockIdx.x * kRastTile, ly = blockIdx.y * kRastTile;
  const int tx1 = min(lx + kRastTile, W) - 1, ty1 = min(ly + kRastTile, H) - 1;
  // the crop's box: rows [r0, r1), cols [c0, c1), clipped to the frame
  int r0 = 0, r1 = H, c0 = 0, c1 = W;
  if (box) {
    r0 = max(box[4 * b + 0], 0), r1 = min(box[4 * b + 1], H);
    c0 = max(box[4 * b + 2], 0), c1 = min(box[4 * b + 3], W);
  }
  const bool touch_box = mask && c0 <= tx1 && c1 > lx && r0 <= ty1 && r1 > ly;
  const int* bx = ws + (size_t)b * C * 4;
  unsigned touch = 0;  // bit c: candidate c's projected box reaches this tile
  for (int c = 0; c < C; ++c)
    if (bx[4 * c] <= tx1 && bx[4 * c + 1] >= lx && bx[4 * c + 2] <= ty1 && bx[4 * c + 3] >= ly) touch |= 1u << c;
  if (!touch_box && !touch) return;  // uniform over the block: no evidence and no render in this tile

  const int x = lx + (tid & (kRastTile - 1)), y = ly + (tid >> 4);
  const bool inside = x < W && y < H;
  long long f0;
  int nf;
  rast_range(face_range, b, Ftot, f0, nf);
  const double pu = (double)x, pv = (double)y;  // the whole frame: rmin = cmin = 0
  const double tu0 = (double)lx, tu1 = (double)tx1, tv0 = (double)ly, tv1 = (double)ty1;
  const double tol = tau[b];

  if (tid < C * kVerFlags) s_cnt[tid] = 0;
  __syncthreads();

  RastCam cam;
  rast_load_cam(cam, R + (size_t)b * C * 9, t + (size_t)b * C * 3, K4 + (size_t)b * 4, 0);  // K4: every candidate's
  double ray = 1.0, obs = 0.0;
  bool evid = false;
  if (inside) {
    const int fr = frame[b];
    bop_observe(cam, pu, pv, depth, F, H, W, fr, x, y, depth_scale, ray, obs);
    if (touch_box && obs > 0.0 && y >= r0 && y < r1 && x >= c0 && x < c1)  // obs > 0: fr is inside [0, F)
      evid = mask[((size_t)fr * H + y) * W + x] != 0;
  }
  const unsigned long long bal_e = __ballot(evid);

  for (int c = 0; c < C; ++c) {  // uniform over the block
    int* sc = s_cnt + c * kVerFlags;
    if (!((touch >> c) & 1u)) {
      if (lane == 0 && bal_e) atomicAdd(&sc[2], __popcll(bal_e));
      continue;
    }
    const size_t bc = (size_t)b * C + c;
    RastHit hit;
    rast_load_cam(cam, R + bc * 9, t + bc * 3, K4 + (size_t)b * 4, 0);
    rast_depth_walk(cam, verts, Vtot, faces, f0, nf, tu0, tu1, tv0, tv1, pu, pv, inside, s_setup, s_id, s_wcnt, hit);
    bool render = false, claim = false, both = false, inter = false;
    if (inside) {
      const double z = hit.f >= 0 ? hit.z : 0.0;  // a pixel that no face covers has depth 0
      const double m = z > 0.0 ? z * ray : 0.0;
      render = m > 0.0;
      if (render && obs > 0.0) {
        const double diff = m - obs;
        claim = !(diff > tol);
        both = claim && evid;
        inter = both && fabs(diff) <= tol;
      }
    }
    const unsigned long long bal_r = __ballot(render), bal_c = __ballot(claim), bal_b = __ballot(both),
                             bal_i = __ballot(inter);
    if (lane == 0) {
      if (bal_r) atomicAdd(&sc[0], __popcll(bal_r));
      if (bal_c) atomicAdd(&sc[1], __popcll(bal_c));
      if (bal_e) atomicAdd(&sc[2], __popcll(bal_e));
      if (bal_b) atomicAdd(&sc[3], __popcll(bal_b));
      if (bal_i) atomicAdd(&sc[4], __popcll(bal_i));
    }
  }
  __syncthreads();
  if (tid < C * kVerFlags && s_cnt[tid]) {
    const int c = tid / kVerFlags, k = tid - c * kVerFlags;
    atomicAdd(&counts[((size_t)b * C + c) * kVerCounts + k], s_cnt[tid]);
  }
}

__global__ void verify_finish_kernel(const double* __restrict__ R, const double* __restrict__ t, int C, int B,
                                     int* __restrict__ counts, double* __restrict__ score, int* __restrict__ best,
                                     float* __restrict__ R_sel, float* __restrict__ t_sel) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int win = 0;
  double top = 0.0;
  for (int c = 0; c < C; ++c) {
    int* q = counts + ((size_t)b * C + c) * kVerCounts;
    const int un = q[1] + q[2] - q[3];
    q[5] = un;
    const double s = un > 0 ? (double)q[4] / (double)un : 0.0;
    score[(size_t)b * C + c] = s;
    if (s > top) top = s, win = c;  // strict >: the lowest index among equals, 0 when every score is 0
  }
  best[b] = win;
  const size_t bc = (size_t)b * C + win;
  if (R_sel)
    for (int i = 0; i < 9; ++i) R_sel[(size_t)b * 9 + i] = (float)R[bc * 9 + i];
  if (t_sel)
    for (int i = 0; i < 3; ++i) t_sel[(size_t)b * 3 + i] = (float)t[bc * 3 + i];
}

}  // namespace

KRRN_API int krrn_pose_score_ws(int B, int C, long long* n_ints) {
  if (!n_ints) return KRRN_EARG;
  if (B < 1 || B > 65535 || C < 1 || C > kVerMaxC) return KRRN_ESHAPE;
  *n_ints = 4ll * B * C;
  return KRRN_OK;
}

KRRN_API int krrn_pose_score_f32(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                                 const double* R, const double* t, int C, const float* K4, const float* depth,
                                 const unsigned char* mask, int F, int H, int W, const int* frame, const int* box,
                                 double depth_scale, const double* tau, int B, int* ws, int* counts, double* score,
                                 int* best, float* R_sel, float* t_sel, void* stream) {
  if (!verts || !faces || !face_range || !R || !t || !K4 || !depth || !frame || !tau || !ws || !counts || !score ||
      !best)
    return KRRN_EARG;
  if (B < 1 || B > 65535 || C < 1 || C > kVerMaxC || Vtot < 1 || Ftot < 0 || F < 1 || H < 1 || W < 1 ||
      H > 65535 * kRastTile || W > 65535 * kRastTile || !(depth_scale > 0.0))
    return KRRN_ESHAPE;
  const size_t b = (size_t)B, bc = b * C, plane = (size_t)F * H * W;
  const Span outs[6] = {{ws, 16 * bc}, {counts, 4 * kVerCounts * bc}, {score, 8 * bc},
                        {best, 4 * b}, {R_sel, R_sel ? 36 * b : 0},   {t_sel, t_sel ? 12 * b : 0}};
  const Span ins[11] = {{verts, 12 * (size_t)Vtot}, {faces, 12 * (size_t)Ftot}, {face_range, 8 * b}, {R, 72 * bc},
                        {t, 24 * bc},               {K4, 16 * b},               {depth, 4 * plane},
                        {mask, mask ? plane : 0},   {frame, 4 * b},             {box, box ? 16 * b : 0},
                        {tau, 8 * b}};
  if (rast_overlap(outs, 6, ins, 11)) return KRRN_EARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(verify_box_kernel, dim3(B, C), dim3(kRastThreads), 0, st, verts, Vtot, faces, Ftot, face_range, R,
                     t, C, K4, ws, counts);
  hipLaunchKernelGGL(verify_score_kernel, dim3(krrn_cdiv(W, kRastTile), krrn_cdiv(H, kRastTile), B),
                     dim3(kRastThreads), 0, st, verts, Vtot, faces, Ftot, face_range, R, t, C, K4, depth, mask, F, H, W,
                     frame, box, depth_scale, tau, ws, counts);
  hipLaunchKernelGGL(verify_finish_kernel, dim3(krrn_cdiv(B, 256)), dim3(256), 0, st, R, t, C, B, counts, score, best,
                     R_sel, t_sel);
  return krrn_launch_status();
}
