// On-GPU input construction of the KRRN eval path, replacing the numpy
// per-sample work of PoseDataset._load_data (dataset/linemod/batchdataset.py:603-771) and, by this project's own
// definition, of its Data.RESIZE path (_load_resize_data, :339-601). Crop b is the S_b x S_b window
// of frame frame[b] at rows rc[2b] .., cols rc[2b+1] .., resampled to T x T (the host snaps the boxes,
// get_square_bbox :890-961):
//
//   crop     img = Normalize(bilinear(window) / 255.) (:722, 744; ImageNet mean / std, :70; cv2.resize's half-pixel
//            centres, INTER_LINEAR, the window's own edge as the border) as NCHW f32, and the point mask =
//            mask_label * mask_depth (* mask_obj when given) (:662-666) at the nearest source pixel of each output
//            pixel's centre
//   choose   the mask pixels in row-major order (:667), a uniformly random order-preserving subset of N when there
//            are more (:668-673), wrap-padded to N when fewer (:675-679); then x/y_map_choosed = the chosen pixel's
//            centre in full-frame coordinates (:712-715; fractional when resampled) and the cloud = the
//            back-projection of its nearest source pixel (:714-721)
//
// krrn_crop_inputs_resize_u8 / krrn_choose_points_resize read S_b = side[b] on the device, so one launch mixes
// sides; krrn_crop_inputs_u8 / krrn_choose_points are the same with every side == S == T.
//
// All index arithmetic is integer: output pixel j sits at window coordinate ((2j+1) S - T) / (2T), so
// nx = (2j+1) S - T, D = 2T, x0 = floor(nx / D), weight (nx - x0 D) / D in f64, nearest pixel ((2j+1) S) / D.
// With S == T the weights are 0, the nearest pixel is j and the centre is j: the native crop. Compiled without FMA
// contraction: every f64 product and sum of the interpolation is rounded on its own. That changes no bit of the
// native outputs, whose other arithmetic has no multiply-add to fuse: (x - mean) / std, (xm - cx) * pt2 / fx.
//
// One workgroup per crop for choose; the selection itself (krrn_choose.h) is the N smallest of per-rank 32-bit hash
// keys. The reference draws the subset with numpy's global RNG (np.random.shuffle); this one is a counter hash of
// (seed, crop, rank): the same distribution, not the same draw.
#include "krrn_choose.h"

namespace {

constexpr int kResizeMaxT = 4096;

// a window the frame does not hold (a bad side[b] or rc row, which the host cannot see): the crop is empty
__device__ __forceinline__ bool window_inside(int r0, int c0, int S, int H, int W) {
  return S >= 1 && r0 >= 0 && c0 >= 0 && S <= H - r0 && S <= W - c0;
}

// output index j of T -> left tap, right tap (clamped to the window) and the right tap's weight
__device__ __forceinline__ void resize_taps(int j, int S, int T, int& a, int& b, double& w) {
  const long long D = 2ll * T, nx = (2ll * j + 1) * S - T;
  long long x0 = nx / D;
  if (nx - x0 * D < 0) --x0;  // floor division
  w = (double)(nx - x0 * D) / (double)D;
  a = (int)min(max(x0, 0ll), (long long)S - 1);
  b = (int)min(max(x0 + 1, 0ll), (long long)S - 1);
}

// the centre of output index j in window coordinates, and its nearest source pixel
__device__ __forceinline__ double resize_centre(int j, int S, int T) {
  return (double)((2ll * j + 1) * S - T) / (double)(2ll * T);
}
__device__ __forceinline__ int resize_nearest(int j, int S, int T) { return (int)(((2ll * j + 1) * S) / (2ll * T)); }

// side == nullptr: every crop's side is T
__global__ __launch_bounds__(256) void crop_inputs_kernel(
    const unsigned char* __restrict__ rgb, const float* __restrict__ depth, const unsigned char* __restrict__ mlabel,
    const unsigned char* __restrict__ mobj, int H, int W, const int* __restrict__ frame, const int* __restrict__ rc,
    const int* __restrict__ side, int T, float* __restrict__ img, unsigned char* __restrict__ mask) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= T * T) return;
  const int i = p / T, j = p - (p / T) * T;
  const int S = side ? side[b] : T;
  const int r0 = rc[2 * b], c0 = rc[2 * b + 1];
  const size_t TT = (size_t)T * T;
  if (!window_inside(r0, c0, S, H, W)) {
    for (int ch = 0; ch < 3; ++ch) img[((size_t)b * 3 + ch) * TT + p] = 0.f;
    mask[(size_t)b * TT + p] = 0;
    return;
  }
  const size_t f = (size_t)frame[b];
  // S == T (uniform over the block: b is blockIdx.y): what the formula gives with less work, the weights being 0
  // and the nearest pixel (i, j); measured, profiles/inputs_one_path.txt
  const bool same = S == T;
  int xa = j, xb = j, ya = i, yb = i;
  double wx = 0.0, wy = 0.0;
  if (!same) {
    resize_taps(j, S, T, xa, xb, wx);
    resize_taps(i, S, T, ya, yb, wy);
  }
  const size_t rowa = (f * H + r0 + ya) * W + c0, rowb = (f * H + r0 + yb) * W + c0;
  const float mean[3] = {0.485f, 0.456f, 0.406f};
  const float stdv[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    double v = (double)rgb[(rowa + xa) * 3 + ch];
    if (!same) {
      const double top = (1.0 - wx) * v + wx * (double)rgb[(rowa + xb) * 3 + ch];
      const double bot = (1.0 - wx) * (double)rgb[(rowb + xa) * 3 + ch] + wx * (double)rgb[(rowb + xb) * 3 + ch];
      v = (1.0 - wy) * top + wy * bot;
    }
    // torchvision Normalize on float32(v / 255.) (the division in f64, as numpy does it)
    const float x = (float)(v / 255.0);
    img[((size_t)b * 3 + ch) * TT + p] = (x - mean[ch]) / stdv[ch];
  }
  const size_t fp = same ? rowa + xa : (f * H + r0 + resize_nearest(i, S, T)) * W + c0 + resize_nearest(j, S, T);
  const bool m = mlabel[fp] != 0 && depth[fp] != 0.f && (!mobj || mobj[fp] != 0);
  mask[(size_t)b * TT + p] = m ? 1 : 0;
}

__global__ __launch_bounds__(kChooseThreads) void choose_points_kernel(
    const unsigned char* __restrict__ mask, int T, int N, const float* __restrict__ depth, int H, int W,
    const int* __restrict__ frame, const int* __restrict__ rc, const int* __restrict__ side,
    const float* __restrict__ K4, float depth_scale, const long long* __restrict__ seed, int stream_id,
    long long* __restrict__ choose, float* __restrict__ cloud, float* __restrict__ xmap, float* __restrict__ ymap,
    int* __restrict__ count_out) {
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int S = side ? side[b] : T;
  const int r0 = rc[2 * b], c0 = rc[2 * b + 1];
  long long* cb = choose + (size_t)b * N;
  const int count = !window_inside(r0, c0, S, H, W) ? 0 :
                    choose_select(mask + (size_t)b * T * T, T * T, N, choose_key_base(seed, stream_id, b), cb);
  if (tid == 0) count_out[b] = count;
  if (count == 0) {
    choose_zero_outputs(b, N, choose, cloud, xmap, ymap);
    return;
  }

  // chosen pixels -> the pixel's centre in the full frame (what PnP reads) and the back-projection of its nearest
  // source pixel with the frame's own K4, float32 arithmetic in the reference's order: pt2 = depth / scale;
  // pt0 = (x - cx) * pt2 / fx; pt1 = (y - cy) * pt2 / fy
  const float fx = K4[4 * b + 0], fy = K4[4 * b + 1], cx = K4[4 * b + 2], cy = K4[4 * b + 3];
  const size_t f = (size_t)frame[b];
  for (int k = tid; k < N; k += kChooseThreads) {
    const int p = (int)cb[k];
    const int i = p / T, j = p % T;
    const int row = r0 + resize_nearest(i, S, T), col = c0 + resize_nearest(j, S, T);
    const float pt2 = depth[(f * H + row) * W + col] / depth_scale;
    xmap[(size_t)b * N + k] = (float)((double)c0 + resize_centre(j, S, T));
    ymap[(size_t)b * N + k] = (float)((double)r0 + resize_centre(i, S, T));
    float* o = cloud + ((size_t)b * N + k) * 3;
    o[0] = ((float)col - cx) * pt2 / fx;
    o[1] = ((float)row - cy) * pt2 / fy;
    o[2] = pt2;
  }
}

}  // namespace

KRRN_API int krrn_crop_inputs_u8(const unsigned char* rgb, const float* depth, const unsigned char* mask_label,
                                 const unsigned char* obj_mask, int F, int H, int W, const int* frame, const int* rc,
                                 int B, int S, float* img, unsigned char* mask, void* stream) {
  if (!rgb || !depth || !mask_label || !frame || !rc || !img || !mask) return KRRN_EARG;
  if (F < 1 || H < 1 || W < 1 || B < 1 || S < 1 || S > H || S > W || B > 65535) return KRRN_ESHAPE;
  hipLaunchKernelGGL(crop_inputs_kernel, dim3(krrn_cdiv(S * S, 256), B), dim3(256), 0, (hipStream_t)stream, rgb,
                     depth, mask_label, obj_mask, H, W, frame, rc, nullptr, S, img, mask);
  return krrn_launch_status();
}

KRRN_API int krrn_choose_points(const unsigned char* mask, int B, int S, int N, const float* depth, int H, int W,
                                const int* frame, const int* rc, const float* K4, float depth_scale,
                                const long long* seed, int stream_id, long long* choose, float* cloud, float* xmap,
                                float* ymap, int* count, void* stream) {
  if (!mask || !depth || !frame || !rc || !K4 || !seed || !choose || !cloud || !xmap || !ymap || !count)
    return KRRN_EARG;
  if (B < 1 || S < 1 || N < 1 || H < 1 || W < 1 || S > H || S > W || depth_scale == 0.f) return KRRN_ESHAPE;
  // (stream_id + 1) << 48 keeps 16 bits of the id: 65535 would give the keys of no stream term at all and
  // 65536 those of 0, so ids outside 0 .. 65534 are refused instead of aliasing
  if (stream_id < 0 || stream_id > kChooseStreamMax) return KRRN_ESHAPE;
  hipLaunchKernelGGL(choose_points_kernel, dim3(B), dim3(kChooseThreads), 0, (hipStream_t)stream, mask, S, N, depth,
                     H, W, frame, rc, nullptr, K4, depth_scale, seed, stream_id, choose, cloud, xmap, ymap, count);
  return krrn_launch_status();
}

KRRN_API int krrn_crop_inputs_resize_u8(const unsigned char* rgb, const float* depth, const unsigned char* mask_label,
                                        const unsigned char* obj_mask, int F, int H, int W, const int* frame,
                                        const int* rc, const int* side, int B, int T, float* img, unsigned char* mask,
                                        void* stream) {
  if (!rgb || !depth || !mask_label || !frame || !rc || !side || !img || !mask) return KRRN_EARG;
  if (F < 1 || H < 1 || W < 1 || B < 1 || B > 65535 || T < 1 || T > kResizeMaxT) return KRRN_ESHAPE;
  hipLaunchKernelGGL(crop_inputs_kernel, dim3(krrn_cdiv(T * T, 256), B), dim3(256), 0, (hipStream_t)stream, rgb,
                     depth, mask_label, obj_mask, H, W, frame, rc, side, T, img, mask);
  return krrn_launch_status();
}

KRRN_API int krrn_choose_points_resize(const unsigned char* mask, int B, int T, int N, const float* depth, int H,
                                       int W, const int* frame, const int* rc, const int* side, const float* K4,
                                       float depth_scale, const long long* seed, int stream_id, long long* choose,
                                       float* cloud, float* xmap, float* ymap, int* count, void* stream) {
  if (!mask || !depth || !frame || !rc || !side || !K4 || !seed || !choose || !cloud || !xmap || !ymap || !count)
    return KRRN_EARG;
  if (B < 1 || B > 65535 || T < 1 || T > kResizeMaxT || N < 1 || H < 1 || W < 1 || depth_scale == 0.f)
    return KRRN_ESHAPE;
  // the same 16 bits of the key as krrn_choose_points: ids outside 0 .. 65534 would alias
  if (stream_id < 0 || stream_id > kChooseStreamMax) return KRRN_ESHAPE;
  hipLaunchKernelGGL(choose_points_kernel, dim3(B), dim3(kChooseThreads), 0, (hipStream_t)stream, mask, T, N, depth,
                     H, W, frame, rc, side, K4, depth_scale, seed, stream_id, choose, cloud, xmap, ymap, count);
  return krrn_launch_status();
}
