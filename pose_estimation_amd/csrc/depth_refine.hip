// Render-based point-to-plane pose refinement on the depth frame (krrn_pose_refine_depth_f32). The definition is
// this project's own (the reference has no such step); include/krrn_hip.h states it too and
// tests/depth_refine_ref.py restates it in numpy f64. Everything is f64 without FMA contraction
// (FLAGS_depth_refine).
//
// Per crop, R, t = R0, t0 (f32 inputs, f64 from there on), rho = radius. Pass k = 0, 1, ...:
//   1. render   the crop's faces under (R, t) and K4 over the whole frame with rast_depth_walk: depth z, winning
//               face f (strict <, lowest face on ties). n = the camera-frame normal of f as raster.hip defines it:
//               (c1 - c0) x (c2 - c0), normalised, negated if n . c0 > 0. A zero or non-finite normal contributes
//               nothing.
//   2. observe  d = depth[frame][y][x] / depth_scale. A pixel is kept iff it is covered, d > 0,
//               |d - z| < max_dist, and mask[frame][y][x] != 0 when the mask is given.
//   3. points   xn = (x - cx) / fx, yn = (y - cy) / fy; p = z (xn, yn, 1), o = d (xn, yn, 1), r = n . (o - p).
//   4. counts   K kept pixels, err_k = sum r^2 / K.
//   5. stop, tested in this order (R, t as they stand are the result, rmse = sqrt(err_k), +inf for K = 0):
//               K < min_pairs -> STARVED; k >= 1 and |err_{k-1} - err_k| <= tol err_{k-1} -> CONVERGED;
//               k == max_iter -> MAX_ITER.
//   6. update   one damped Gauss-Newton step in a twist about the object's own centre t, the rotation part scaled
//               by rho: J = [((p - t) / rho) x n, n]; A = sum J J^T, b = sum J r; A += damp trace(A) / 6 I; 6 x 6
//               Cholesky. A non-positive or non-finite pivot, or a non-finite solution, keeps the pose from before
//               the update and stops with DEGENERATE. Otherwise xi = (w, v): R <- exp(w / rho) R (Rodrigues),
//               t <- t + v.
//   7. outputs  R, t as f32 (the input's own bits for a stop in pass 0), passes = the k at the stop, pairs = the
//               last K, rmse f32, status = icp.hip's codes.
//
// Three launches per pass, in the style of verify.hip, and max_iter + 1 passes enqueued whatever the data:
//   refine_box_kernel    one block per crop: bop_project_box under the crop's current pose (pass 0 also moves R0, t0
//                        into the crop's f64 state).
//   refine_tile_kernel   one block per 16 x 16 tile of the frame and crop. A tile outside the box, or of a crop
//                        whose state is final, returns at once. Otherwise one depth walk; every thread forms its
//                        pixel's J and r; the 21 upper-triangle entries of A, the 6 of b and sum r^2 are reduced one
//                        after the other (per-thread value, wave butterfly, then the four waves in order), the
//                        count by ballot; the tile's partials go to its own slot of ws with plain vector stores,
//                        zeros included.
//   refine_solve_kernel  one block per crop: 28 threads add one entry each over the box's slots in row-major tile
//                        order, one thread the counts; thread 0 tests, solves, updates the crop's pose and state
//                        and stores the outputs once the state is final.
// No atomics, no block waits for another, every loop is bounded by nf, max_iter and the tile counts. A tile's sums
// depend on the crop alone and are added in a fixed order: results are bit-identical from run to run and whatever
// else is in the batch.
#include "krrn_observe.h"

namespace {

constexpr int kRefA = 21, kRefB = 6;
constexpr int kRefSums = kRefA + kRefB + 1;  // A's upper triangle row by row, b, sum r^2
constexpr int kRefState = 16;                // f64 per crop: R [9], t [3], err of the pass before, 3 spare
constexpr int kRefInts = 8;                  // int per crop: final flag, then the box (u lo, u hi, v lo, v hi), 3 spare
constexpr int kRefSolveThreads = 64;
constexpr int kRefMaxIter = 32;
enum { kRefConverged = 0, kRefMaxIterHit = 1, kRefStarved = 2, kRefDegenerate = 3 };

// ws: f64 state [B][16] | f64 slots [B][tiles][28] | int32 ints [B][8] | int32 counts [B][tiles]
struct RefWs {
  double* state;
  double* slots;
  int* ints;
  int* counts;
};

__host__ __device__ inline RefWs ref_ws(void* ws, int B, int tiles) {
  RefWs w;
  w.state = (double*)ws;
  w.slots = w.state + (size_t)B * kRefState;
  w.ints = (int*)(w.slots + (size_t)B * tiles * kRefSums);
  w.counts = w.ints + (size_t)B * kRefInts;
  return w;
}

// the tiles [tx0, tx1] x [ty0, ty1] the projected box reaches inside the frame; false = none
__device__ __forceinline__ bool ref_tile_range(const int* bx, int H, int W, int& tx0, int& tx1, int& ty0, int& ty1) {
  if (bx[0] > bx[1] || bx[2] > bx[3]) return false;
  const int u0 = max(bx[0], 0), u1 = min(bx[1], W - 1), v0 = max(bx[2], 0), v1 = min(bx[3], H - 1);
  if (u0 > u1 || v0 > v1) return false;
  tx0 = u0 / kRastTile, tx1 = u1 / kRastTile, ty0 = v0 / kRastTile, ty1 = v1 / kRastTile;
  return true;
}

__device__ __forceinline__ double ref_wave_sum(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__global__ __launch_bounds__(kRastThreads) void refine_box_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ face_range, const float* __restrict__ R0, const float* __restrict__ t0,
    const float* __restrict__ K4, int pass, int B, int tiles, void* ws_) {
  __shared__ double s_box[kRastWaves][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const RefWs ws = ref_ws(ws_, B, tiles);
  double* st = ws.state + (size_t)b * kRefState;
  int* in = ws.ints + (size_t)b * kRefInts;
  if (pass > 0 && in[0]) return;  // uniform over the block: the crop is final
  RastCam cam;
  if (pass == 0) {
    for (int i = 0; i < 9; ++i) cam.r[i] = (double)R0[(size_t)b * 9 + i];
    for (int i = 0; i < 3; ++i) cam.t[i] = (double)t0[(size_t)b * 3 + i];
    if (tid < 9) st[tid] = (double)R0[(size_t)b * 9 + tid];
    else if (tid < 12) st[tid] = (double)t0[(size_t)b * 3 + tid - 9];
    else if (tid < kRefState) st[tid] = 0.0;
    if (tid == kRefState) in[0] = 0;
    cam.fx = (double)K4[4 * b + 0], cam.fy = (double)K4[4 * b + 1];
    cam.cx = (double)K4[4 * b + 2], cam.cy = (double)K4[4 * b + 3];
  } else {
    rast_load_cam(cam, st, st + 9, K4 + (size_t)b * 4, 0);
  }
  bop_project_box(cam, verts, Vtot, faces, Ftot, face_range, b, s_box, in + 1);
}

__global__ __launch_bounds__(kRastThreads) void refine_tile_kernel(
    const float* __restrict__ verts, int Vtot, const int* __restrict__ faces, int Ftot,
    const int* __restrict__ face_range, const float* __restrict__ K4, const float* __restrict__ depth,
    const unsigned char* __restrict__ mask, int F, int H, int W, const int* __restrict__ frame, double depth_scale,
    const double* __restrict__ max_dist, const double* __restrict__ radius, int B, int tiles, void* ws_) {
  __shared__ double s_setup[kRastThreads * kRastSetup];
  __shared__ int s_id[kRastThreads];
  __shared__ int s_wcnt[kRastWaves];
  __shared__ double s_red[kRastWaves][kRefSums];

  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const RefWs ws = ref_ws(ws_, B, tiles);
  const int* in = ws.ints + (size_t)b * kRefInts;
  if (in[0]) return;  // uniform over the block: the crop is final
  int tx0, tx1, ty0, ty1;
  if (!ref_tile_range(in + 1, H, W, tx0, tx1, ty0, ty1)) return;
  const int bxi = blockIdx.x, byi = blockIdx.y;
  if (bxi < tx0 || bxi > tx1 || byi < ty0 || byi > ty1) return;  // uniform: the render does not reach this tile

  const int lx = bxi * kRastTile, ly = byi * kRastTile;
  const int px1 = min(lx + kRastTile, W) - 1, py1 = min(ly + kRastTile, H) - 1;
  const int x = lx + (tid & (kRastTile - 1)), y = ly + (tid >> 4);
  const bool inside = x < W && y < H;
  long long f0;
  int nf;
  rast_range(face_range, b, Ftot, f0, nf);
  const double pu = (double)x, pv = (double)y;  // the whole frame: rmin = cmin = 0

  const double* st = ws.state + (size_t)b * kRefState;
  RastCam cam;
  rast_load_cam(cam, st, st + 9, K4 + (size_t)b * 4, 0);
  RastHit hit;
  rast_depth_walk(cam, verts, Vtot, faces, f0, nf, (double)lx, (double)px1, (double)ly, (double)py1, pu, pv, inside,
                  s_setup, s_id, s_wcnt, hit);

  bool kept = false;
  double J[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r = 0.0;
  if (inside && hit.f >= 0) {
    const double z = hit.z;
    const int fr = frame[b];
    double d = 0.0;
    bool on = false;
    if (fr >= 0 && fr < F) {
      const size_t pix = ((size_t)fr * H + y) * W + x;
      d = (double)depth[pix] / depth_scale;
      on = mask ? mask[pix] != 0 : true;
    }
    if (on && d > 0.0 && fabs(d - z) < max_dist[b]) {  // false for a NaN sample, depth or max_dist
      double n[3];
      if (rast_face_normal(cam, verts, faces + (size_t)(f0 + hit.f) * 3, n)) {  // in range: it passed the walk's test
        const double xn = (pu - cam.cx) / cam.fx, yn = (pv - cam.cy) / cam.fy;
        const double p[3] = {z * xn, z * yn, z};
        const double o[3] = {d * xn, d * yn, d};
        r = (n[0] * (o[0] - p[0]) + n[1] * (o[1] - p[1])) + n[2] * (o[2] - p[2]);
        const double rho = radius[b];
        const double q[3] = {(p[0] - cam.t[0]) / rho, (p[1] - cam.t[1]) / rho, (p[2] - cam.t[2]) / rho};
        J[0] = q[1] * n[2] - q[2] * n[1];
        J[1] = q[2] * n[0] - q[0] * n[2];
        J[2] = q[0] * n[1] - q[1] * n[0];
        J[3] = n[0], J[4] = n[1], J[5] = n[2];
        kept = true;
      }
    }
  }
  // one sum at a time keeps seven f64 per thread live across the butterflies instead of 28
  int e = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j, ++e) {
      const double v = ref_wave_sum(J[i] * J[j]);
      if (lane == 0) s_red[wave][e] = v;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double v = ref_wave_sum(J[i] * r);
    if (lane == 0) s_red[wave][kRefA + i] = v;
  }
  {
    const double v = ref_wave_sum(r * r);
    if (lane == 0) s_red[wave][kRefA + kRefB] = v;
  }
  const unsigned long long bal = __ballot(kept);
  if (lane == 0) s_wcnt[wave] = __popcll(bal);  // the walk ended with a barrier
  __syncthreads();
  const size_t slot = (size_t)b * tiles + (size_t)byi * gridDim.x + bxi;
  if (tid < kRefSums) {
    double v = s_red[0][tid];
    for (int w = 1; w < kRastWaves; ++w) v += s_red[w][tid];
    ws.slots[slot * kRefSums + tid] = v;
  } else if (tid == kRefSums) {
    int c = 0;
    for (int w = 0; w < kRastWaves; ++w) c += s_wcnt[w];
    ws.counts[slot] = c;
  }
}

__global__ __launch_bounds__(kRefSolveThreads) void refine_solve_kernel(
    const float* __restrict__ R0, const float* __restrict__ t0, const double* __restrict__ radius, int H, int W,
    int pass, int max_iter, double tol, int min_pairs, double damp, int B, int tiles, int tiles_x, void* ws_,
    float* __restrict__ R_out, float* __restrict__ t_out, int* __restrict__ passes, int* __restrict__ pairs,
    float* __restrict__ rmse, int* __restrict__ status) {
  __shared__ double s_sum[kRefSums];
  __shared__ int s_count;
  const int b = blockIdx.x, tid = threadIdx.x;
  const RefWs ws = ref_ws(ws_, B, tiles);
  double* st = ws.state + (size_t)b * kRefState;
  int* in = ws.ints + (size_t)b * kRefInts;
  if (in[0]) return;  // uniform over the block: final in an earlier pass
  int tx0 = 0, tx1 = -1, ty0 = 0, ty1 = -1;
  ref_tile_range(in + 1, H, W, tx0, tx1, ty0, ty1);  // false leaves an empty range
  if (tid <= kRefSums) {
    double v = 0.0;
    int c = 0;
    for (int ty = ty0; ty <= ty1; ++ty)
      for (int tx = tx0; tx <= tx1; ++tx) {
        const size_t slot = (size_t)b * tiles + (size_t)ty * tiles_x + tx;
        if (tid < kRefSums) v += ws.slots[slot * kRefSums + tid];
        else c += ws.counts[slot];
      }
    if (tid < kRefSums) s_sum[tid] = v;
    else s_count = c;
  }
  __syncthreads();
  if (tid != 0) return;

  const int K = s_count;
  const double err = K > 0 ? s_sum[kRefA + kRefB] / (double)K : INFINITY;
  const double err_prev = st[12];
  int stop = -1;
  if (K < min_pairs) stop = kRefStarved;
  else if (pass >= 1 && fabs(err_prev - err) <= tol * err_prev) stop = kRefConverged;
  else if (pass == max_iter) stop = kRefMaxIterHit;

  if (stop < 0) {
    double A[6][6], L[6][6], g[6], xi[6];
    int e = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j, ++e) A[i][j] = A[j][i] = s_sum[e];
    for (int i = 0; i < 6; ++i) g[i] = s_sum[kRefA + i];
    const double tr = ((((A[0][0] + A[1][1]) + A[2][2]) + A[3][3]) + A[4][4]) + A[5][5];
    const double lam = damp * tr / 6.0;
    for (int i = 0; i < 6; ++i) A[i][i] += lam;
    bool ok = true;
    for (int j = 0; j < 6 && ok; ++j) {
      double s = A[j][j];
      for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
      if (!(s > 0.0) || !isfinite(s)) {
        ok = false;
        break;
      }
      L[j][j] = sqrt(s);
      for (int i = j + 1; i < 6; ++i) {
        double a = A[i][j];
        for (int k = 0; k < j; ++k) a -= L[i][k] * L[j][k];
        L[i][j] = a / L[j][j];
      }
    }
    if (ok) {
      double yv[6];
      for (int i = 0; i < 6; ++i) {  // L y = b
        double a = g[i];
        for (int k = 0; k < i; ++k) a -= L[i][k] * yv[k];
        yv[i] = a / L[i][i];
      }
      for (int i = 5; i >= 0; --i) {  // L^T xi = y
        double a = yv[i];
        for (int k = i + 1; k < 6; ++k) a -= L[k][i] * xi[k];
        xi[i] = a / L[i][i];
      }
      for (int i = 0; i < 6; ++i) ok = ok && isfinite(xi[i]);
    }
    double Rn[9], tn[3];
    if (ok) {
      const double rho = radius[b];
      const double w[3] = {xi[0] / rho, xi[1] / rho, xi[2] / rho};
      const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
      double E[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
      if (th > 0.0) {
        const double k0 = w[0] / th, k1 = w[1] / th, k2 = w[2] / th;
        const double s = sin(th), c1 = 1.0 - cos(th);
        const double Kx[9] = {0.0, -k2, k1, k2, 0.0, -k0, -k1, k0, 0.0};
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) {
            const double kk = (Kx[3 * i] * Kx[j] + Kx[3 * i + 1] * Kx[3 + j]) + Kx[3 * i + 2] * Kx[6 + j];
            E[3 * i + j] = (E[3 * i + j] + s * Kx[3 * i + j]) + c1 * kk;
          }
      }
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          Rn[3 * i + j] = (E[3 * i] * st[j] + E[3 * i + 1] * st[3 + j]) + E[3 * i + 2] * st[6 + j];
          ok = ok && isfinite(Rn[3 * i + j]);
        }
      for (int i = 0; i < 3; ++i) {
        tn[i] = st[9 + i] + xi[3 + i];
        ok = ok && isfinite(tn[i]);
      }
    }
    if (ok) {
      for (int i = 0; i < 9; ++i) st[i] = Rn[i];
      for (int i = 0; i < 3; ++i) st[9 + i] = tn[i];
      st[12] = err;
      return;  // the next pass renders the new pose
    }
    stop = kRefDegenerate;
  }

  in[0] = 1;
  if (pass == 0) {  // no update was applied: the start pose's own bits
    for (int i = 0; i < 9; ++i) R_out[(size_t)b * 9 + i] = R0[(size_t)b * 9 + i];
    for (int i = 0; i < 3; ++i) t_out[(size_t)b * 3 + i] = t0[(size_t)b * 3 + i];
  } else {
    for (int i = 0; i < 9; ++i) R_out[(size_t)b * 9 + i] = (float)st[i];
    for (int i = 0; i < 3; ++i) t_out[(size_t)b * 3 + i] = (float)st[9 + i];
  }
  passes[b] = pass;
  pairs[b] = K;
  rmse[b] = (float)sqrt(err);
  status[b] = stop;
}

bool ref_dims_ok(int B, int H, int W) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= 65535 * kRastTile && W <= 65535 * kRastTile;
}

long long ref_ws_bytes(int B, int tiles) {
  return (long long)B * (8ll * kRefState + 4ll * kRefInts + (long long)tiles * (8ll * kRefSums + 4ll));
}

}  // namespace

KRRN_API int krrn_pose_refine_depth_ws(int B, int H, int W, long long* n_bytes) {
  if (!n_bytes) return KRRN_EARG;
  if (!ref_dims_ok(B, H, W)) return KRRN_ESHAPE;
  *n_bytes = ref_ws_bytes(B, krrn_cdiv(W, kRastTile) * krrn_cdiv(H, kRastTile));
  return KRRN_OK;
}

KRRN_API int krrn_pose_refine_depth_f32(const float* verts, int Vtot, const int* faces, int Ftot,
                                        const int* face_range, const float* R0, const float* t0, const float* K4,
                                        const float* depth, const unsigned char* mask, int F, int H, int W,
                                        const int* frame, double depth_scale, const double* max_dist,
                                        const double* radius, int max_iter, double tol, int min_pairs, double damp,
                                        int B, void* ws, float* R, float* t, int* passes, int* pairs, float* rmse,
                                        int* status, void* stream) {
  if (!verts || !faces || !face_range || !R0 || !t0 || !K4 || !depth || !frame || !max_dist || !radius || !ws || !R ||
      !t || !passes || !pairs || !rmse || !status)
    return KRRN_EARG;
  if (!ref_dims_ok(B, H, W) || Vtot < 1 || Ftot < 0 || F < 1 || max_iter < 0 || max_iter > kRefMaxIter ||
      min_pairs < 6 || !(tol >= 0.0) || !isfinite(tol) || !(damp >= 0.0) || !isfinite(damp) || !(depth_scale > 0.0))
    return KRRN_ESHAPE;
  const int tiles_x = krrn_cdiv(W, kRastTile), tiles_y = krrn_cdiv(H, kRastTile);
  if ((long long)tiles_x * tiles_y > INT32_MAX) return KRRN_ESHAPE;
  const int tiles = tiles_x * tiles_y;
  const size_t b = (size_t)B, plane = (size_t)F * H * W;
  const Span outs[7] = {{ws, (size_t)ref_ws_bytes(B, tiles)}, {R, 36 * b}, {t, 12 * b}, {passes, 4 * b},
                        {pairs, 4 * b}, {rmse, 4 * b}, {status, 4 * b}};
  const Span ins[11] = {{verts, 12 * (size_t)Vtot}, {faces, 12 * (size_t)Ftot}, {face_range, 8 * b}, {R0, 36 * b},
                        {t0, 12 * b},               {K4, 16 * b},               {depth, 4 * plane},
                        {mask, mask ? plane : 0},   {frame, 4 * b},             {max_dist, 8 * b},
                        {radius, 8 * b}};
  if (rast_overlap(outs, 7, ins, 11)) return KRRN_EARG;
  hipStream_t st = (hipStream_t)stream;
  for (int pass = 0; pass <= max_iter; ++pass) {  // no decision on the host: a final crop costs an early exit
    hipLaunchKernelGGL(refine_box_kernel, dim3(B), dim3(kRastThreads), 0, st, verts, Vtot, faces, Ftot, face_range,
                       R0, t0, K4, pass, B, tiles, ws);
    hipLaunchKernelGGL(refine_tile_kernel, dim3(tiles_x, tiles_y, B), dim3(kRastThreads), 0, st, verts, Vtot, faces,
                       Ftot, face_range, K4, depth, mask, F, H, W, frame, depth_scale, max_dist, radius, B, tiles, ws);
    hipLaunchKernelGGL(refine_solve_kernel, dim3(B), dim3(kRefSolveThreads), 0, st, R0, t0, radius, H, W, pass,
                       max_iter, tol, min_pairs, damp, B, tiles, tiles_x, ws, R, t, passes, pairs, rmse, status);
  }
  return krrn_launch_status();
}
