/*
 * krrn_hip.h — C ABI of libkrrn_hip.so, the MI355X (gfx950) kernels of the KRRN dense-fusion
 * inference path of yaomy533/pose_estimation (lib/network/krrn.py + tools/trainer.py:383-438).
 *
 * The reference has no FFI (pure Python/PyTorch); each entry point below names
 * the reference function(s) whose arithmetic it replaces. The Python host side
 * (pose_estimation_amd/) keeps the reference's model/loader/get_pose API and binds these
 * symbols with ctypes (INTEGRATION.md shows the binding).
 *
 * Contract shared by every entry point
 *   - Ownership: the caller allocates every input, output and workspace buffer (device
 *     memory); the library never allocates, keeps no global state and is reentrant.
 *   - Streams: all work is enqueued on `stream` (a hipStream_t); no host synchronisation, so
 *     every call can be captured into a hipGraph.
 *   - Errors: 0 = launched; KRRN_EARG (-1) null pointer / bad enum, KRRN_ESHAPE (-2) size out
 *     of range, KRRN_EALIGN (-3) 16-byte / channel-multiple-of-4 violation — all detected on
 *     the host before any launch; a positive value is the hipError_t of the launch.
 *   - Layouts: activations are NHWC f32 with a channel stride `*_cs` and channel offset
 *     `*_co` (so a buffer can be a slice of a concat); point sets are [B][n][stride] f32 with a
 *     batch stride `*_bs` (floats); indices produced by the library are int32.
 */
#ifndef KRRN_HIP_H
#define KRRN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KRRN_OK 0
#define KRRN_EARG (-1)
#define KRRN_ESHAPE (-2)
#define KRRN_EALIGN (-3)
#define KRRN_EUNSUPPORTED (-4) /* valid arguments, but a form the kernel does not offer */

/* Implicit-GEMM convolution / GEMM on the f32 matrix cores, BN folded into scale/bias.
 * Replaces nn.Conv2d + BatchNorm2d (+ residual add) (+ ReLU) of BasicBlock / Bottleneck /
 * transitions / fuse layers / last_layer (lib/network/hrnet/myhrnet.py:34-103, 177-221,
 * 328-381), the XYZNet / NMLNet convs and 1x1 heads (lib/network/krrn.py:46-84),
 * ConvTranspose2d (myhrnet.py:314-326, krrn.py:47) as 4 parity-class launches, the GCN
 * `feature_map @ weights + bias` (lib/network/point/gcn3d.py:151, 203) and the TBase Conv1d
 * chain (lib/network/pose/posenet.py:58-77).
 *   out[m, n] = act(scale[n] * sum_k A[m,k] W[n,k] + bias[n] + bias2[m / b2_div, n] + res[m, n])
 *   m = (b, gy, gx) on a B x Hg x Wg grid; k = (tap, c), A = in[b, gy*in_s + tap_dy, gx*in_s + tap_dx, c]
 *   output pixel (gy*osy + ooy, gx*osx + oox) of a Ho x Wo map; wt is [N][ntaps*cin] row-major.
 *   N = computed channels (multiple of 4), n_store <= N stored; out_nchw = 1 writes
 *   out[b][out_co + n][oy][ox] with out_cs = total channels. tile (BMxBNxBK): 0 auto,
 *   1 = 128x128x16, 2 = 128x64x16, 3 = 64x64x16, 4 = 128x128x32, 5 = 256x32x16,
 *   6 = 128x32x32, 7 = 128x64x32, 8 = 64x64x32; out_nchw supports tiles 0-3 only.
 *   splits > 1 (NHWC only; N, n_store multiples of 4): split-K for small-M / deep-K layers
 *   (the 4x4 and 8x8 HRNet branches): each of `splits` slices of the k-tiles writes raw
 *   partial sums to workspace [splits][M][N] f32, then a second kernel sums them in slice
 *   order and applies the epilogue (deterministic). The slice count actually used is
 *   cdiv(nkt, cdiv(nkt, splits)) <= splits. splits = 1: workspace unused (may be NULL). */
int krrn_conv2d_f32(const float* in, int in_cs, int in_co, int B, int Hi, int Wi, int cin, int Hg, int Wg,
                    int in_s, int ntaps, const int* tap_dy, const int* tap_dx, const float* wt, int N,
                    int n_store, const float* scale, const float* bias, const float* bias2, int b2_div,
                    const float* res, int res_cs, int res_co, float* out, int out_cs, int out_co, int Ho,
                    int Wo, int osy, int osx, int ooy, int oox, int relu, int out_nchw, int tile, int splits,
                    float* workspace, void* stream);

/* One problem of a grouped convolution launch: the arguments of krrn_conv2d_f32 as a struct
 * (NHWC output only; tap_dy/tap_dx hold the first ntaps entries). */
typedef struct krrn_conv_desc {
  const float* in;
  int in_cs, in_co, B, Hi, Wi, cin, Hg, Wg, in_s, ntaps;
  int tap_dy[9];
  int tap_dx[9];
  const float* wt;
  int N, n_store;
  const float* scale;
  const float* bias;
  const float* bias2;
  int b2_div;
  const float* res;
  int res_cs, res_co;
  float* out;
  int out_cs, out_co, Ho, Wo, osy, osx, ooy, oox, relu, out_nchw, splits;
  float* workspace;
  /* k order of wt: 0 = tap-major (k = tap*cin + c); Q > 0 (Q % 4 == 0, Q | cin) = channel-chunk
   * major, k = ((c / Q)*ntaps + tap)*Q + c % Q: a block walks every tap of a Q-channel slice of
   * its input pixels back to back, so the taps' overlapping reads hit L1 / L2 instead of re-fetching
   * a whole tap's slab (the transposed convs' parity classes). Grouped launches only. */
  int k_chunk;
} krrn_conv_desc;

/* Up to 4 independent convolutions in ONE launch with a shared tile shape (tile 1 = 128x128x16,
 * 6 = 128x32x32 or 8 = 64x64x32), each with its own split-K factor: the j-th conv of every HRNet branch of a
 * HighResolutionModule (myhrnet.py:177-225: branch i is a chain of BasicBlocks on its own
 * resolution, so the branches are independent until the fuse layer). Each problem computes
 * exactly what krrn_conv2d_f32 would with the same descriptor. */
int krrn_conv2d_group_f32(const krrn_conv_desc* descs, int n, int tile, void* stream);

/* krrn_conv2d_f32 / krrn_conv2d_group_f32 on the bf16 matrix cores at f32 accuracy (NHWC output,
 * every tile of the menu / tiles 1, 6, 8): the activations are split while staged, the weights beforehand, into
 * three bf16 terms each (x = x_h + x_m + x_l, round-to-nearest, exact); every product is summed
 * over the six term pairs hh, hm, mh, hl, lh, mm (the dropped ones are below 2^-23 |a b|) and
 * accumulated in f32. wt3 (or each desc's wt) holds the split weights, bf16 [N][K / 4][16]: per 4 k
 * the terms m0..m3 h0..h3 l0..l3 then 4 zeros (ops.conv_weights_x3); 16-byte aligned. */
int krrn_conv2d_x3_f32(const float* in, int in_cs, int in_co, int B, int Hi, int Wi, int cin, int Hg, int Wg,
                       int in_s, int ntaps, const int* tap_dy, const int* tap_dx, const void* wt3, int N, int n_store,
                       const float* scale, const float* bias, const float* bias2, int b2_div, const float* res,
                       int res_cs, int res_co, float* out, int out_cs, int out_co, int Ho, int Wo, int osy, int osx,
                       int ooy, int oox, int relu, int tile, int splits, float* workspace, void* stream);
int krrn_conv2d_group_x3_f32(const krrn_conv_desc* descs, int n, int tile, void* stream);
/* Stride-2 ConvTranspose2d (kernel <= 4, padding 1; myhrnet.py:314-326's deconv, krrn.py:47-49's
 * XYZNet layer) as its four output parity classes in ONE block per 4 x 32 region of the input grid, on
 * split-bf16 operands at f32 accuracy (convt.hip): out[2a + py][2b + px][n] (NHWC, channels out_co ..
 * out_co + N - 1 of pixel rows of out_cs floats, Ho x Wo <= 2 Hi x 2 Wi) = act(scale[n] *
 * sum over the class's taps t and channels k of in[a + dy_t][b + dx_t][k] W[k][n] + bias[n]).
 * cls_taps (host memory, read at the call): for class c = 2 py + px, cls_taps[5c] = its tap count
 * (1..4) and cls_taps[5c + 1 + t] = (dy_t + 1) * 3 + (dx_t + 1). U3 = ops.convT_weights_x3: plane
 * U_mh [cin/8][16][N][2][8] bf16 (element class * 4 + tap; m0..m3 h0..h3 of channels 4 half ..
 * 4 half + 3) then plane U_l [cin/8][16][N][2][4]; 16-byte aligned. N = 128; cin a multiple of 8;
 * in 16-byte aligned with in_cs, in_co multiples of 4. relu != 0 applies ReLU. Replaces the grouped
 * krrn_conv2d_group_x3_f32 launch of the four classes (lib/network/krrn.py:47-49). */
int krrn_convT_s2_x3_f32(const float* in, int in_cs, int in_co, int B, int Hi, int Wi, int cin, const int* cls_taps,
                         const void* U3, int N, const float* scale, const float* bias, int relu, float* out,
                         int out_cs, int out_co, int Ho, int Wo, void* stream);

/* Plain GEMM on the bf16 matrix cores at f32 accuracy (gemm_x3.hip: split-bf16 operands,
 * six term products per f32 product): the GCN `feature_map @ weights` of G6/G7
 * (lib/network/point/gcn3d.py:125-127, 184-186) and TBase's Conv1d chain (posenet.py:51-96).
 *   out[m*ldo + n] = act(sum_k A[m*lda + k] W[n][k] + bias[n] + res[m*ldr + n]),  0 <= n < N
 * in `batch` strided groups of M rows (A / out / res advance a_grp / o_grp / r_grp floats per
 * group, W [N][K] shared); ldr = 0 adds one
 * res row per group (res[g*r_grp + n], a per-crop bias). w3f holds W split
 * into per-wave MFMA fragments (ops.gemm_weights_x3: [N/32][K/8][2][64 lanes][4] u32).
 * K % 32 == 0, N % 128 == 0, lda / ldo / ldr % 4 == 0, 16-byte aligned A / W / out / res. */
int krrn_gemm_x3_f32(const float* a, int lda, int M, int K, int N, const void* w3f, const float* bias,
                     const float* res, int ldr, float* out, int ldo, int relu, int batch, long long a_grp,
                     long long o_grp, long long r_grp, void* stream);

/* TBase conv2 on a gathered operand (gemm_x3.hip, GA form): conv1 runs by linearity on the fusion's
 * level rows (posenet.py:51-96 with the concat of lib/network/point/fusion.py:234-238 and the
 * one-hot channels of lib/network/krrn.py:132-138 folded into two per-crop row tables), and conv2
 * reads h1 = ReLU(A[b, ia[b, i]] + A2[b, ib[b, i]]) row by row while staging its operand, so h1 is
 * never materialised (it replaces krrn_gather2_add_f32 + krrn_gemm_x3_f32 on h1):
 *   out[(b*npts + i)*ldo + n] = act(sum_k h1[b, i, k] W[n][k] + bias[n])
 * A [B][a_bs floats], rows a_st apart; A2 likewise; ia / ib int32 [B][npts] row indices into the
 * crop's table. w3f as for krrn_gemm_x3_f32. K % 32 == 0, N % 128 == 0, strides % 4 == 0,
 * 16-byte aligned tables / W / out, B * a_bs and B * a2_bs < 2^29 floats. */
int krrn_gemm_x3_gather_f32(const int* ia, const float* A, long long a_bs, int a_st, const int* ib, const float* A2,
                            long long a2_bs, int a2_st, int npts, int B, int K, int N, const void* w3f,
                            const float* bias, float* out, int ldo, int relu, void* stream);

/* Live-row forms of the two GEMMs above, for TBase on a crop's distinct rows (posenet.py:51-96 with
 * pred_t of krrn.py:150-153: a point's h1 row depends only on its (nearest_pool_1, nearest_pool_2)
 * pair, krrn_pair_compact_i32): live int32 [batch] / [B] = rows in use per group. Row tiles (128
 * rows) are per group (the gathered form tiles each crop's npts rows, out[(b*npts + j)*ldo + n]); a
 * tile that starts at or past live[g] is skipped and writes nothing, a partly live tile is computed
 * whole (its reads and stores stay inside the group's rows). Live rows equal the rows of the forms
 * above bit for bit. live must not be NULL (KRRN_EARG); other arguments and limits as above. */
int krrn_gemm_x3_live_f32(const float* a, int lda, int M, int K, int N, const void* w3f, const float* bias,
                          const float* res, int ldr, float* out, int ldo, int relu, int batch, long long a_grp,
                          long long o_grp, long long r_grp, const int* live, void* stream);
int krrn_gemm_x3_gather_live_f32(const int* ia, const float* A, long long a_bs, int a_st, const int* ib,
                                 const float* A2, long long a2_bs, int a2_st, int npts, int B, int K, int N,
                                 const void* w3f, const float* bias, float* out, int ldo, int relu, const int* live,
                                 void* stream);

/* Short-K GEMM streaming its output (gemm_panel.hip): the fusion's level-0 / level-1 GCN
 * `feature_map @ weights + bias` of Conv_layer (lib/network/point/gcn3d.py:136-164, K = 128,
 * N = 8 * 128) and layer1's 64 -> 256 1x1 convs (myhrnet.py:65-103, K = 64):
 *   out[m*ldo + n] = act(sum_k A[m*lda + k] W[n][k] + bias[n] + res[m*ldr + n]),  0 <= n < N
 * Split-bf16 operands at f32 accuracy; each wave keeps its 32 activation rows in registers, the
 * 4 waves of a block walk 32-column tiles whose weights are copied once per block into LDS. wpf
 * holds W split into bf16 terms (ops.gemm_weights_panel: [N/32][K/8][384] u32, per 8-k group 64 lanes
 * x [m0..m3 h0..h3] then 64 lanes x [l0..l3]).
 * K = 64 or 128, N % 32 == 0, N <= 2048, lda % 4 == 0, A / wpf 16-byte
 * aligned; `csplit` column ranges per row panel (grid = ceil(M / 128) x csplit). K = 128 with a
 * residual: KRRN_EUNSUPPORTED. */
int krrn_gemm_panel_x3_f32(const float* a, int lda, int M, int K, int N, const void* wpf, const float* bias,
                           const float* res, int ldr, float* out, int ldo, int relu, int csplit, void* stream);

/* 1x1 conv with NCHW output (the heads' final xyz / normal convs, lib/network/krrn.py:97-98,
 * 80-84): out[b][out_co + n][p] = scale[n] * sum_c in[(b * HW + p) * in_cs + in_co + c] wt[n][c]
 * + bias[n] for n < n_store, p < HW; out has out_cs channels per image. cin <= 256 (multiple of 4),
 * N <= 80 weight rows (wt [N][cin]); in / wt 16-byte aligned. */
int krrn_conv1x1_nchw_f32(const float* in, int in_cs, int in_co, int B, int HW, int cin, const float* wt, int N,
                          int n_store, const float* scale, const float* bias, float* out, int out_cs, int out_co,
                          void* stream);

/* krrn_conv1x1_nchw_f32 on split-bf16 operands (f32 accuracy; the same output): cin = 128 and w3
 * the split weight planes of ops.quad_weights_x3(wt, N, 128) (16-byte aligned); 32 < N <= 80. */
int krrn_conv1x1_nchw_x3_f32(const float* in, int in_cs, int in_co, int B, int HW, int cin, const void* w3, int N,
                             int n_store, const float* scale, const float* bias, float* out, int out_cs, int out_co,
                             void* stream);

/* 3x3 stride-1 pad-1 convolution by fused Winograd F(2x2, 3x3) (the head / last_layer /
 * deconv-BasicBlock convs: krrn.py:46-84, myhrnet.py:324-346; cuDNN / MIOpen use the same
 * algorithm for these f32 convs), on the bf16 matrix cores at f32 accuracy: every operand split
 * into three bf16 terms (x = x_h + x_m + x_l, round-to-nearest, exact), each product summed over
 * the six term pairs hh, hm, mh, hl, lh, mm (the dropped ones are below 2^-23 |a b|), accumulated
 * in f32. U = G g G^T are the transformed weights, f32 in chunk-major order
 * [ceil(cin/8)][16][N][8] (element xi = 4u + v of the 4x4 transform; input channels padded to a
 * multiple of 8 with zeros), computed once per plan (wino_weights); U3 is U split on the host
 * (wino_weights_x3): plane U_mh [ceil(cin/8)][16][N][2][8] bf16 (m0..m3 h0..h3 of channels
 * 4 half .. 4 half + 3) followed by plane U_l [ceil(cin/8)][16][N][2][4] bf16. Epilogue as
 * krrn_conv2d_f32: out = act(scale[n] * conv + bias[n] (+ res)). NHWC in/out with channel
 * stride / offset; cin multiple of 4, U3 16-byte aligned. */
int krrn_conv3x3_wino_x3_f32(const float* in, int in_cs, int in_co, int B, int H, int W, int cin, const void* U3,
                             int N, int n_store, const float* scale, const float* bias, const float* res, int res_cs,
                             int res_co, float* out, int out_cs, int out_co, int relu, void* stream);
/* The same conv by Winograd F(4x4, 3x3) (points 0, +-1, +-2; 2.25 products per output instead of
 * 4) on split-bf16 operands, for the heads' wide 128 -> 128 convs (krrn.py:52-63, 74-81). U3 is
 * wino4_weights' U = G g G^T ([cin/8][36][N][8] f32, element xi = 6u + v) split on the host
 * (wino_weights_x3): plane U_mh [cin/8][36][N][2][8] bf16 then plane U_l [cin/8][36][N][2][4]
 * bf16. cin a multiple of 8; in 16-byte aligned with in_cs, in_co multiples of 4; other arguments
 * as krrn_conv3x3_wino_x3_f32 (any out / res channel alignment).
 * `relu` holds flags: bit 0 = ReLU; bit 1 = `in` is the half-resolution source of
 * UpsamplingBilinear2d(2) (align_corners = True, krrn.py:56, 78): [B][H / 2][W / 2][in_cs], and the conv
 * reads its x2 bilinear upsample, which is never formed (the interpolation is folded into the input
 * transform: V = (B^T Ly) X (B^T Lx)^T over the 4 x 4 source pixels X a 6 x 6 patch touches). H, W stay
 * the conv's own size and must be even with bit 1 set; any other bit, or an odd size: KRRN_ESHAPE.
 * Callers passing 0 or 1 get the plain conv. */
int krrn_conv3x3_wino4_x3_f32(const float* in, int in_cs, int in_co, int B, int H, int W, int cin, const void* U3,
                              int N, int n_store, const float* scale, const float* bias, const float* res, int res_cs,
                              int res_co, float* out, int out_cs, int out_co, int relu, void* stream);
/* krrn_conv3x3_wino_x3_head_f32 on the F(4x4, 3x3) kernel (U3 as krrn_conv3x3_wino4_x3_f32; cin a
 * multiple of 8, in 16-byte aligned with in_cs, in_co multiples of 4; `relu` holds the same flags). */
int krrn_conv3x3_wino4_x3_head_f32(const float* in, int in_cs, int in_co, int B, int H, int W, int cin,
                                   const void* U3, int N, const float* scale, const float* bias, const float* res,
                                   int res_cs, int res_co, int relu, const float* w1, const float* b1, int p1,
                                   float* part, float* out, int out_c, void* stream);
/* A head's last 3x3 conv fused with its final 1x1 conv (nml_final, krrn.py:80-84 / 98, when it has
 * at most 4 output channels): h = act(scale[n] * conv3x3 + bias[n] (+ res)) as
 * krrn_conv3x3_wino_x3_f32 with n_store = N, then out[b][o][y][x] = sum_n w1[o][n] h[n] + b1[o]
 * for o < p1 (NCHW, out_c channels per image). The N-channel map h is never written: each
 * 64-channel block of the Winograd grid writes its 4 partial dot products per pixel to part
 * (ceil(N / 64) * B * H * W * 4 floats, 16-byte aligned), and a second launch adds them in block
 * order plus b1 (deterministic). w1 [4][N] f32 (rows >= p1 zero), 16-byte aligned; N % 4 == 0,
 * 1 <= p1 <= 4; b1 may be NULL. */
int krrn_conv3x3_wino_x3_head_f32(const float* in, int in_cs, int in_co, int B, int H, int W, int cin,
                                  const void* U3, int N, const float* scale, const float* bias, const float* res,
                                  int res_cs, int res_co, int relu, const float* w1, const float* b1, int p1,
                                  float* part, float* out, int out_c, void* stream);

/* Direct conv for narrow layers: 3x3 / pad 1 / stride 1 or 2, or 1x1 / stride 1 (the HRNet
 * branches' BasicBlock convs, lib/network/hrnet/myhrnet.py:34-63, and the fuse layers' stride-2
 * downsamples / 1x1 projections, :177-225). NHWC in (in_cs / in_co, H x W input, cin physical
 * channels, multiple of 4), weights wt [N][ksize^2 * cin] (k = tap * cin + c, tap = ky * ksize + kx),
 * out (Ho x Wo = the conv's output size) = act(scale[n] * conv + bias[n] (+ res)) for n < n_store.
 * A block stages the input rows of its 64 / ks output pixels (all channels) in LDS once;
 * 16x16x4 f32 MFMAs; nw = 16-channel output tiles per wave (1..3), ks = waves splitting the
 * reduction of one tile (1, 2, 4; partials summed in LDS in order). A last tile of one channel
 * quad (N % 16 in 1..4) runs on the 4x4x1 f32 MFMA where a wave's share of the reduction is at least
 * 8 16-wide K steps (ceil(ceil(ksize^2 * cin / 16) / ks) >= 8); its channels are then four
 * per-k-quad fma chains added as (g0 + g1) + (g2 + g3), still f32, deterministic and independent of
 * the batch. Shorter reductions and remainders of 2 or 3 quads run as a padded 16-channel tile. */
int krrn_conv_small_f32(const float* in, int in_cs, int in_co, int B, int H, int W, int cin, const float* wt, int N,
                        int n_store, const float* scale, const float* bias, const float* res, int res_cs, int res_co,
                        float* out, int out_cs, int out_co, int relu, int ksize, int stride, int nw, int ks,
                        void* stream);

/* Test-only: one v_mfma_f32_4x4x1_16b_f32 on one wave, to pin the lane layout krrn_conv_small_f32's
 * ragged channel tail relies on. a, b: 64 floats (lane l's first / second operand), c: 64 x 4 floats
 * (lane l's accumulator registers 0..3), d: 64 x 4 floats out, the same layout. c, d 16-byte aligned. */
int krrn_mfma4x4_probe_f32(const float* a, const float* b, const float* c, float* d, void* stream);


/* k nearest neighbours without the [n, n] distance matrix.
 * Replaces gcn3d.get_neighbor_index (gcn3d.py:15-26; mode 0, drop_first = 1: topk(k+1)[1:])
 * and gcn3d.get_nearest_index (gcn3d.py:29-38; mode 1, k = 1, drop_first = 0).
 * Queries: q + b*q_bs + qi*q_st (qi = qidx[t] if qidx else t, t < nq; qidx shared by the
 * batch: the Pool_layer randperm rows, gcn3d.py:239); candidates c + b*c_bs + j*c_st, j < nc;
 * d = 3 or 9. Exact f32 expression order (no FMA):
 *   mode 0: ((-2 <q,c>) + |c|^2) + |q|^2      mode 1: (|c|^2 + |q|^2) - 2 <q,c>
 * with <.,.> and |.|^2 summed sequentially over d; ties -> lower index.
 * out: int32 [B][nq][k]. k + drop_first <= 16. */
int krrn_knn_f32(const float* q, long long q_bs, int q_st, int nq, const int* qidx, const float* c,
                 long long c_bs, int c_st, int nc, int d, int k, int drop_first, int mode, int B, int* out,
                 void* stream);

/* 3D-GCN neighbourhood reduction, fused with the BN1d + ReLU FusionNetLite applies.
 * Y == NULL: Conv_surface (gcn3d.py:88-112):  out[i,c] = sum_s max_j relu(dir_ij . dn[:, sC+c])
 * Y != NULL: Conv_layer / Conv_fuse_layer (gcn3d.py:136-216):
 *   out[i,c] = Y[i,c] + sum_s max_j relu(dir_ij . dn[:, sC+c]) * Y[idx[i,j], C + sC + c]
 * then out = out*bn_scale + bn_bias (if given), relu (if set) (fusion.py:183-213).
 * dir_ij = F.normalize(v[idx[i,j]] - v[i]) over d = 3 or 9 coords (v stride v_st);
 * dn = F.normalize(directions, dim=0) [d][S*C]; Y [B][n][(S+1)*C]; idx int32 [B][n][k], k <= 16;
 * out + b*o_bs + i*o_st + c. */
int krrn_gcn_conv_f32(const int* idx, int n, int k, const float* v, long long v_bs, int v_st, int d,
                      const float* dn, int S, int C, const float* Y, const float* bn_scale, const float* bn_bias,
                      int relu, float* out, long long o_bs, int o_st, int B, void* stream);

/* Pool_layer max (gcn3d.py:233-236) at the sampled rows only: out[b,t,:] = max_j F[b, nbr[b,t,j], :].
 * C, strides multiple of 4 (float4). */
int krrn_pool_max_f32(const int* nbr, int nq, int kk, const float* F, long long f_bs, int f_st, int C, float* out,
                      long long o_bs, int o_st, int B, void* stream);

/* Bilinear resize NHWC (F.interpolate(mode='bilinear'), myhrnet.py:242-245 / 511-516 with
 * align_corners = 0; nn.UpsamplingBilinear2d, krrn.py:56/78, with align_corners = 1), optionally
 * out = add + resize(in) and ReLU: the HRNet fuse-layer "y = y + interpolate(...)" step. */
int krrn_resize_bilinear_f32(const float* in, int B, int Hi, int Wi, int in_cs, int in_co, int C, float* out,
                             int Ho, int Wo, int out_cs, int out_co, const float* add, int add_cs, int add_co,
                             int align_corners, int relu, void* stream);

/* out = relu?(a + b) on NHWC channel slices (HRNet fuse identity term, myhrnet.py:237-238;
 * b == NULL copies a, the concat of myhrnet.py:516). C, strides and offsets multiples of 4, a / b /
 * out 16-byte aligned (float4; KRRN_EALIGN otherwise). out may be a itself (same stride and offset). */
int krrn_add_relu_f32(const float* a, int a_cs, int a_co, const float* b, int b_cs, int b_co, float* out,
                      int o_cs, int o_co, long long npix, int C, int relu, void* stream);

/* NCHW [B][C][H][W] -> NHWC channel slice (the API boundary of KRRN.forward's x). */
int krrn_nchw_to_nhwc_f32(const float* in, int B, int C, int H, int W, float* out, int o_cs, int o_co,
                          void* stream);

/* Per-crop class selection of the xyz / normal maps + F.normalize(p=2, dim=1, eps=1e-12)
 * (krrn.py:105-108). fx: xyz_final output NCHW [B][Cx][H][W] (xyz block at channel xyz_off),
 * fn: nml_final output [B][Cn][H][W]; cls int64 [B]. */
int krrn_heads_select_f32(const float* fx, int Cx, int xyz_off, const float* fn, int Cn, const long long* cls,
                          float* xyz_out, float* nml_out, int B, int H, int W, void* stream);

/* The `choose` gather (krrn.py:121-122) packed as P9 [B][N][9] = [cloud | xyz_emb | nml_emb]
 * (the feat_feature layout of fusion.py:194). choose int64 [B][N]. */
int krrn_points_gather_f32(const float* cloud, const float* xyz, const float* nml, const long long* choose, int B,
                           int N, int H, int W, float* p9, void* stream);

/* Row gather dst[b, r, 0:width] = src[b, idx[b*idx_bs + r], 0:width] (int32 or int64 idx;
 * idx_bs = 0 shares one index list across the batch): Pool_layer sampling (gcn3d.py:240-241),
 * indexing_neighbor by the nearest indices into the 1280-wide concat (fusion.py:234-238),
 * the one-hot column of TBase conv1 (krrn.py:132-138). */
int krrn_gather_rows_f32(const void* idx, int idx64, long long idx_bs, int nrows, const float* src, long long src_bs,
                         int src_st, float* dst, long long dst_bs, int dst_st, int width, int B, void* stream);

/* TBase conv1 over the fusion concat by linearity (krrn.py:132-141 with fusion.py:234-238):
 * out[b][i] = act(scale * (A[b][ia[b][i]] + B[b][ib[b][i]]) + bias + bias2[b]) over C channels,
 * with A = fm_5 W1[:, 0:512]^T (level-2 rows, ia = nearest_pool_2) and B = feat_1 W1[:, 512:896]^T +
 * feat_2 W1[:, 896:1280]^T (level-1 rows, ib = nearest_pool_1); ia / ib int32 [B][n]; bias2
 * [B][C] optional (the one-hot class column, pre-scaled). C, strides multiple of 4, 16-B aligned. */
int krrn_gather2_add_f32(const int* ia, const float* A, long long a_bs, int a_st, const int* ib, const float* B_,
                         long long b_bs, int b_st, int n, int C, const float* scale, const float* bias,
                         const float* bias2, int relu, float* out, long long o_bs, int o_st, int B, void* stream);

/* TBase conv4 (first 3 outputs, posenet.py:76-80) + pred_t = mean_N(cloud + t_res) (krrn.py:153).
 * h [B][n][C]; w4 [3][C]; b4 [3]; cloud [B][n][3]; pred_t [B][3]; t_res optional [B][n][3].
 * C multiple of 4, h and w4 16-byte aligned (KRRN_EALIGN otherwise). */
int krrn_tbase_tail_f32(const float* h, int B, int n, int C, const float* w4, const float* b4, const float* cloud,
                        float* pred_t, float* t_res, void* stream);

/* The same tail reading point i's row at h[b][slot[b][i]] (slot int32 [B][n], values < n): TBase on
 * the crop's distinct rows (posenet.py:51-96, krrn.py:150-153). Same loop, lane mapping and reduction
 * tree, so pred_t / t_res equal krrn_tbase_tail_f32's on the expanded h bit for bit. */
int krrn_tbase_tail_slot_f32(const float* h, const int* slot, int B, int n, int C, const float* w4, const float* b4,
                             const float* cloud, float* pred_t, float* t_res, void* stream);

/* Distinct (ia, ib) pairs per crop (posenet.py:51-96, krrn.py:150-153: TBase's row of a point depends
 * only on its two nearest indices). ia / ib int32 [B][npts] with values < n1 / < n2; keys ia*n2 + ib.
 * cnt[b] = number of distinct keys; (pa, pb)[b][j], j < cnt[b], = the distinct pairs in ascending key
 * order, entries j >= cnt[b] repeat entry 0; slot[b][i] = the rank of point i's key. One block per
 * crop, deterministic. n1 * n2 <= 2^18 and npts <= 65535 (KRRN_ESHAPE otherwise). */
int krrn_pair_compact_i32(const int* ia, const int* ib, int B, int npts, int n1, int n2, int* cnt, int* pa, int* pb,
                          int* slot, void* stream);

/* Batched PnP-RANSAC: Trainer.get_pose (tools/trainer.py:383-438), cv2.solvePnPRansac(EPNP,
 * reprojectionError = thr, confidence = conf (0.9999 there), iterationsCount = H) restated.
 * xyz [B][3][HW] (normalised model coords), choose int64 [B][N], sel int32 [B][P] (the
 * randperm(N)[:P] subset), x/ymap [B][N] full-frame pixels, K4 [B][4] = fx fy cx cy,
 * extent / lfborder f64 [B][3], subsets int32 [B][H][5] (hypothesis h's sample); workspace:
 * B*H*13 floats (per-hypothesis pose + inlier count). Hypotheses are scored in parallel; the
 * selection is ptsetreg.cpp's loop over them in order with its adaptive iteration count
 * (niters <- RANSACUpdateNumIters(conf, outlier ratio, 5, niters) on every new best). Outputs R
 * [B][9] row-major, t [B][3], inlier count [B] (0 = RANSAC failed -> R = I, t = 0), inlier_mask
 * [B][P] (optional). Two launches: one 16-lane group per hypothesis, then one wave per crop for
 * the selection + EPnP on all inliers. */
int krrn_pnp_ransac_f32(const float* xyz, int HW, const long long* choose, int N, const int* sel, int P,
                        const float* xmap, const float* ymap, const float* K4, const double* extent,
                        const double* lfborder, const int* subsets, int H, float thr, double conf, float* workspace,
                        float* R, float* t, int* inliers, unsigned char* inlier_mask, int B, void* stream);

/* Model points of the chosen pixels (tools/script/eval.py:128's coordinate_choosed_all, de-normalised
 * as trainer.py:415-421 does): out[b][i] = float(xyz[b][:, choose[b][i]] * extent[b] + lfborder[b]),
 * f64 math then f32 -- the same expression krrn_pnp_ransac_f32 uses for its object points.
 * xyz [B][3][HW], choose int64 [B][N] (a pixel outside [0, HW) gives NaN), out [B][N][3]. */
int krrn_model_points_f32(const float* xyz, int HW, const long long* choose, int N, const double* extent,
                          const double* lfborder, float* out, int B, void* stream);

/* estimateSimilarityTransform (lib/transform/umeyama.py:8-98), batched: RANSAC over 5-point Umeyama
 * fits of dst ~ s R src + t, then a refit on the inliers of the best one. src / dst f32 [B][N][3]
 * (5 <= N <= 4096); subsets int32 [B][H][5] (indices in [0, N), duplicates allowed; H <= 8192);
 * hyp_counts int32 [B][H] (workspace and diagnostic: every hypothesis's inlier count); outputs
 * scale [B], R [B][9] row-major, t [B][3], inliers [B] (0 = failed -> scale 1, R = I, t = 0),
 * best_hyp [B] (optional, -1 on failure), inlier_mask uint8 [B][N] (optional).
 * All arithmetic in f64. Threshold s_h * inlier_frac * 2 * max_i |src_i - mean(src)| (:16-20, the
 * reference's inlier_frac is 0.1), strict <; a hypothesis whose scale is not finite and positive
 * counts 0. Selection: the reference's loop over the hypotheses in order on the counts scored in
 * parallel (:31-49): a strictly larger count becomes the best, and the loop stops after iteration i
 * (zero-based) once 1 - (1 - best_ratio^5)^i > conf (0.99 there); best_ratio < min_ratio (0.1) is
 * the reference's None (:50-52). Two launches: scoring (16 hypotheses per wave, one lane each),
 * then one block per crop for the selection and the refit (fixed-order sums, no atomics). */
int krrn_umeyama_ransac_f32(const float* src, const float* dst, int N, const int* subsets, int H,
                            double inlier_frac, double conf, double min_ratio, int* hyp_counts,
                            float* scale, float* R, float* t, int* inliers, int* best_hyp,
                            unsigned char* inlier_mask, int B, void* stream);

/* Point-to-point ICP refinement of a pose against the depth cloud, batched (this project's own
 * definition: the reference has none). R0 [B][9] row-major, t0 [B][3]: the starting pose, model to
 * camera (p = R m + t); cloud f32 [B][N][3] (3 <= N <= 4096), model f32 [B][M][3] (1 <= M <= 4096),
 * max_dist [B] in metres. Pass k = 0 .. max_iter (<= 64): q_i = R^T (p_i - t); the nearest model point
 * j(i) by d^2 = (dx dx + dy dy) + dz dz (the lowest j among equal distances; a distance that is
 * NaN never wins, so a non-finite model point pairs with nothing and a non-finite cloud point has no
 * pair, nn_idx -1); pair i kept iff d_i^2 < max_dist^2 (max_dist 0 keeps nothing, +inf every finite
 * d^2); K pairs, err_k = mean kept d^2. Stop, tested in this order: K < min_pairs
 * (>= 3) -> status 2 STARVED; k >= 1 and |err_{k-1} - err_k| <= tol err_{k-1} -> 0 CONVERGED;
 * k == max_iter -> 1 MAX_ITER. Otherwise Kabsch on the kept pairs (two-pass covariance, the Jacobi SVD
 * of krrn_umeyama_ransac_f32) gives the next R, t; if that is not finite the pose from before the
 * update is returned with 3 DEGENERATE. Outputs (must not alias the inputs): R [B][9], t [B][3],
 * passes [B] = k + 1, pairs [B] = K and rmse [B] = sqrt(err_k) (+inf for K = 0) of the returned pose,
 * status [B], nn_idx int32 [B][N] (optional: j(i) of the returned pose, -1 = rejected). A stop in pass
 * 0 (max_iter 0, no pairs, a non-finite start) returns R0, t0 bit for bit. All arithmetic in f64; one
 * block per crop and one launch for the whole loop, fixed-order sums, no atomics: a crop's outputs do
 * not depend on the rest of the batch. */
int krrn_icp_refine_f32(const float* R0, const float* t0, const float* cloud, int N, const float* model, int M,
                        const float* max_dist, int max_iter, double tol, int min_pairs, float* R, float* t,
                        int* passes, int* pairs, float* rmse, int* status, int* nn_idx, int B, void* stream);

/* torch.randperm(n)[:k] per row (gcn3d.py:239, trainer.py:407) from a counter-based generator
 * seeded by *seed_ptr (device memory) and `stream_id`; n <= 4096. out int32 [rows][k]. */
int krrn_randperm_i32(const unsigned long long* seed_ptr, unsigned int stream_id, int n, int k, int rows, int* out,
                      void* stream);

/* Up to 8 independent single-row draws of krrn_randperm_i32 in ONE launch (the five Pool_layer
 * permutations of a forward, gcn3d.py:239): draw q is torch.randperm(n[q])[:k[q]] for stream id
 * stream_id[q] into out[q], bit-identical to krrn_randperm_i32(seed_ptr, stream_id[q], n[q], k[q],
 * 1, out[q]); the draws run side by side (one block each) instead of back to back. */
int krrn_randperm_multi_i32(const unsigned long long* seed_ptr, int count, const unsigned int* stream_id, const int* n,
                            const int* k, int* const* out, void* stream);

/* RANSAC subsets: 5 distinct indices in [0, P) per (crop, hypothesis); out int32 [B][H][5]. */
int krrn_ransac_subsets(const unsigned long long* seed_ptr, unsigned int stream_id, int B, int H, int P, int* out,
                        void* stream);

/* *seed_ptr += 1 (last node of a replayed step). */
int krrn_rng_advance(unsigned long long* seed_ptr, void* stream);

/* Eval-time KRRNLoss map terms (lib/network/loss.py:57-65 over loss_utils.py:8-70), SURVEY §8f f1.
 * NCHW maps of B crops with HW pixels: xyz / xyz_gt [B][3][HW] (l1), nml / nml_gt [B][3][HW]
 * (1 - cosine, CosineSimilarity eps 1e-6), region [B][R][HW] + region_gt int64 [B][HW] and mask
 * [B][M][HW] + mask_gt int64 [B][HW] (-log(softmax + 1e-6) at the label). Pixels whose target is
 * all zero (label 0) are excluded; each term = sum / valid count. Any term may be skipped by
 * passing NULL maps. out f64 [8]: losses xyz, normal, region, mask, then the four valid counts.
 * ws: f64 workspace of krrn_map_losses_ws(B, HW) doubles. Deterministic (fixed-order sums). */
int krrn_map_losses_ws(int B, int HW, long long* n_doubles);
int krrn_map_losses_f32(const float* xyz, const float* xyz_gt, const float* nml, const float* nml_gt,
                        const float* region, int R, const long long* region_gt, const float* mask, int M,
                        const long long* mask_gt, int B, int HW, double* ws, double* out, void* stream);
/* Per-crop form, read from the ws a preceding krrn_map_losses_f32(B, HW) filled (same stream):
 * out_crop f64 [B][8] = crop b's four losses then its four valid counts. The reference's test
 * loop runs batch size 1 and adds each crop's own losses to its object (tools/trainer.py:180-182). */
int krrn_map_losses_crop_f32(const double* ws, int B, int HW, double* out_crop, void* stream);

/* PoseLoss (lib/network/loss.py:19-42) with the GT rotation and the predicted translation as
 * KRRNLoss calls it (:66-67): pred = model_points [B][P][3] @ target_r[b]^T + pred_t[b]; for
 * crops whose cls_id is in sym[0..nsym) each predicted point takes its nearest target point
 * (squared distance, ties -> lower index; the KeOps argkmin of train.py:126); out f64 [1] =
 * mean over crops of mean_P |pred - target|. ws: krrn_pose_loss_ws(B, P) doubles. */
int krrn_pose_loss_ws(int B, int P, long long* n_doubles);
int krrn_pose_loss_f32(const float* target_r, const float* pred_t, const float* target, const float* model_points,
                       const long long* cls_id, const int* sym, int nsym, int B, int P, double* ws, double* out,
                       void* stream);

/* ADD(-S) per crop (Metric.cal_adds_cuda, lib/utils/metric.py:17-35, called by Trainer.cal_dis,
 * tools/trainer.py:370-381): pred = model_points [B][P][3] @ pred_r[b]^T + pred_t[b]; out f64 [B]
 * = mean_i |pred_i - target_i| (ADD), or for cls_id[b] in sym[0..nsym) mean over targets i of
 * min over preds j |pred_j - target_i| (ADD-S, exact direct-difference norms). ws: the same
 * size as krrn_pose_loss_ws(B, P). Deterministic. */
int krrn_add_metric_f32(const float* pred_r, const float* pred_t, const float* model_points, const float* target,
                        const long long* cls_id, const int* sym, int nsym, int B, int P, double* ws, double* out,
                        void* stream);

/* On-GPU input construction, replacing PoseDataset._load_data's per-sample numpy work
 * (dataset/linemod/batchdataset.py:603-771) and, by this project's own definition, its Data.RESIZE
 * path (_load_resize_data, :339-601), for B crops resampled to one size T.
 * Frames: rgb u8 [F][H][W][3], depth f32 [F][H][W], mask_label u8 [F][H][W], optional obj_mask u8
 * [F][H][W] (the reference's mask_obj from the GT coordinate map, :662; NULL = all ones).
 * Crop b is the S_b x S_b window of frame[b] at rows rc[2b] .., cols rc[2b+1] .., S_b = side[b] (int32 [B], read
 * on the device: one launch mixes sides). All index arithmetic is integer. Output pixel j of T sits at window
 * coordinate ((2j+1) S_b - T) / (2T) (cv2.resize's half-pixel centres; rows alike): nx = (2j+1) S_b - T, D = 2T,
 * x0 = floor(nx / D), wx = (double)(nx - x0 D) / (double)D, taps xa = clamp(x0, 0, S_b - 1), xb = clamp(x0 + 1, 0,
 * S_b - 1): the border is the window's own edge (the reference resizes the cut window).
 * krrn_crop_inputs_resize_u8: img f32 [B][3][T][T]: per channel on the raw u8 values, in f64 with every product and
 * sum rounded on its own, top = (1 - wx) a[ya][xa] + wx a[ya][xb], bot likewise on row yb, p = (1 - wy) top + wy bot;
 * then (float(p / 255.) - mean) / std (ImageNet, :70, 722, 744). Plain bilinear also when S_b > T (INTER_LINEAR; no
 * area averaging). mask u8 [B][T*T] = mask_label != 0 && depth != 0 (&& obj_mask != 0) (:662-666) at the nearest
 * source pixel of the centre, (r0 + ((2i+1) S_b) / D, c0 + ((2j+1) S_b) / D) by integer division, always inside the
 * window. The reference's 'resize' branch resizes the whole frame, not the window, for mask, coordinate and region:
 * not copied. 1 <= T <= 4096, 1 <= B <= 65535 (KRRN_ESHAPE otherwise, before any launch). The host cannot see
 * side[b] or rc: the caller keeps every window inside the frame (dataset.build_inputs checks its boxes); a window
 * that is not gives a crop of zeros with an empty mask. */
int krrn_crop_inputs_resize_u8(const unsigned char* rgb, const float* depth, const unsigned char* mask_label,
                               const unsigned char* obj_mask, int F, int H, int W, const int* frame, const int* rc,
                               const int* side, int B, int T, float* img, unsigned char* mask, void* stream);

/* choose (:667-679) over the T*T mask: its pixels in row-major order; more than N -> a uniformly random
 * order-preserving N-subset (the N smallest of counter-hash keys of (seed, stream_id, crop, rank),
 * radix-selected; the reference draws it with np.random.shuffle), fewer -> wrap-padded to N. choose int64 [B][N] =
 * i*T + j; count [B] = mask pixels (0 -> zeros everywhere: the reference drops such a sample). For a chosen pixel
 * (i, j): x_map = (float)((double)c0 + (double)nx / (double)D), y_map likewise: the resized pixel's centre in
 * full-frame coordinates (:712-715), generally fractional, which is what krrn_pnp_ransac_f32 reads; cloud [B][N][3] =
 * the back-projection of the nearest source pixel (sr, sc) above with the frame's own K4 [B][4] = fx, fy, cx, cy,
 * f32 arithmetic in the reference's order (:718-721): z = depth[sr][sc] / depth_scale, ((float)sc - cx) z / fx,
 * ((float)sr - cy) z / fy. The reference (:551-553) truncates bilinear x / y maps to int16 to index the depth and
 * (:526) moves the principal point to OUT_SIZE / 2: not copied. Limits as above, N >= 1, depth_scale != 0; a window
 * outside the frame gives count 0 and zeros.
 * 0 <= stream_id <= 65534 (KRRN_ESHAPE otherwise, before any launch): the id enters the key's top 16 bits
 * as stream_id + 1, so ids further apart would draw the same subsets. A caller that needs more draws per
 * seed than that advances the seed (PoseDataset.batch does). */
int krrn_choose_points_resize(const unsigned char* mask, int B, int T, int N, const float* depth, int H, int W,
                              const int* frame, const int* rc, const int* side, const float* K4, float depth_scale,
                              const long long* seed, int stream_id, long long* choose, float* cloud, float* xmap,
                              float* ymap, int* count, void* stream);

/* Crops at their own snapped square size S: the same with every side == S and T = S, by the same kernels. The
 * weights are then 0, the nearest pixel is (i, j) and x_map / y_map are the full-frame column / row: img f32
 * [B][3][S][S], mask u8 [B][S*S], choose = crop-local r*S + c. 1 <= S <= min(H, W), 1 <= B <= 65535 for the crop,
 * B, N >= 1 (KRRN_ESHAPE otherwise); a window the frame does not hold (a bad rc row) is an empty crop here too: an
 * image of zeros, an empty mask, count 0 and zero outputs. */
int krrn_crop_inputs_u8(const unsigned char* rgb, const float* depth, const unsigned char* mask_label,
                        const unsigned char* obj_mask, int F, int H, int W, const int* frame, const int* rc, int B,
                        int S, float* img, unsigned char* mask, void* stream);
int krrn_choose_points(const unsigned char* mask, int B, int S, int N, const float* depth, int H, int W,
                       const int* frame, const int* rc, const float* K4, float depth_scale, const long long* seed,
                       int stream_id, long long* choose, float* cloud, float* xmap, float* ymap, int* count,
                       void* stream);

/* The zoom-in pass's windows (this project's own rule): per crop b the square window of its H x W frame
 * that holds the projection of its model points pts f32 [B][P][3] (metres) under the pose R f64 [B][9] row-major,
 * t f64 [B][3] and the pinhole K4 f32 [B][4], as rc int32 [B][2] = (r0, c0) and side int32 [B] = S in the form
 * the two entry points above read from device memory, so that a pose computed on the GPU re-crops without a
 * read-back. All f64, every product and sum rounded on its own (no FMA contraction):
 * per point X = ((R00 x + R01 y) + R02 z) + t0, Y and Z alike, u = (fx X) / Z + cx, v = (fy Y) / Z + cy. A point is
 * bad unless Z > 0 (NaN is not) and u and v are finite; this is tested per point, not on the extremes.
 * status int32 [B]: 1 = some point is bad; else 2 = the projection misses the frame (umax < 0, umin > W - 1,
 * vmax < 0 or vmin > H - 1, the extremes over the points); else 0 and
 *   e = max(umax - umin, vmax - vmin) * pad, S = clamp(ceil(e), min_side, min(H, W)),
 *   c0 = clamp(floor((umin + umax) * 0.5 - S * 0.5 + 1.0), 0, W - S), r0 alike from v and H,
 * clamped in f64 before the conversion to int: the window is shifted into the frame and never shrunk. With
 * status != 0 the window is the previous one, (rc_in [B][2], side_in [B]) copied. In every case
 * bbox f32 [B][4] = (r0, r0 + S, c0, c0 + S), scale f32 [B] = (float)(S / T) and intr f32 [B][4] =
 * (fx / s, fy / s, (cx - c0 + 0.5) / s - 0.5, (cy - r0 + 0.5) / s - 0.5) with s = S / T in f64 from the f32 K4, cast
 * once: dataset.resize_intrinsic's values bit for bit. One block per crop, no atomics, no workspace; graph-capturable.
 * 1 <= B <= 65535, P >= 1, T >= 1, H, W >= 1, 1 <= min_side <= min(H, W), pad finite and > 0 (KRRN_ESHAPE
 * otherwise, before any launch). */
int krrn_pose_windows_f64(const float* pts, int P, const double* R, const double* t, const float* K4, int H, int W,
                          int T, double pad, int min_side, const int* rc_in, const int* side_in, int B, int* rc,
                          int* side, float* bbox, float* scale, float* intr, int* status, void* stream);

/* Farthest point sampling (tools/script/sample_model.py:35-48): per set b of
 * pts [B][n][3], out_idx int32 [B][n_samples] = start at 0, then repeatedly the argmax (lowest
 * index on ties) of the running min distance to the selected set; distances as numpy computes
 * them (f32, sqrt(((dx*dx + dy*dy) + dz*dz)), no FMA). n <= 16384. */
int krrn_fps_f32(const float* pts, int B, int n, int n_samples, int* out_idx, void* stream);

/* Ground-truth map rendering, batched (this project's own definition: the reference unpickles xyz /
 * normal / region maps made by an offline renderer that is not in its tree, batchdataset.py:200-210). A
 * z-buffered triangle rasteriser over B crops of one size S. verts f32 [Vtot][3] (model frame, metres),
 * faces int32 [Ftot][3] (indices into verts), face_range int32 [B][2] = first face, face count of crop b
 * (a batch may mix objects; count 0 = all background), R f64 [B][9] row-major and t f64 [B][3] (model to
 * camera), K4 f32 [B][4] = fx fy cx cy, rc int32 [B][2] = rmin, cmin, region_pts f32 [B][NR][3] (model
 * frame, metres; NR 1..256). All arithmetic in f64, no FMA contraction:
 *   c_k = ((r0 x + r1 y) + r2 z) + t per vertex; a face with a vertex index outside [0, Vtot) or any
 *   c_k.z not > 1e-3 is skipped whole (no clipping); u = fx c.x / c.z + cx, v = fy c.y / c.z + cy;
 *   E(a, b, p) = (b.u - a.u)(p.v - a.v) - (b.v - a.v)(p.u - a.u); A = E(v0, v1, v2), a face with A == 0 or
 *   not finite is skipped; both windings are drawn. Pixel (x, y) of the crop is sampled at its integer
 *   coordinates p = (cmin + x, rmin + y) (the loader's xmap / ymap convention, :712-721; not + 0.5) and
 *   tested against a face iff p lies in the face's bounding box (inclusive): w0 = E(v1, v2, p) / A,
 *   w1 = E(v2, v0, p) / A, w2 = E(v0, v1, p) / A, covered iff all three >= 0. q_k = w_k / z_k, depth
 *   z = 1 / ((q0 + q1) + q2) (perspective-correct); the winner is the covering face with the smallest z,
 *   the lowest face index among equal z. Model coordinate m = z ((q0 vert_0 + q1 vert_1) + q2 vert_2);
 *   normal = normalize((c1 - c0) x (c2 - c0)), the face's flat unit normal in the camera frame, negated
 *   if n . c0 > 0 so that it faces the camera (the offline renderer's normals are unknown: a stated
 *   departure); region = 1 + argmin_j ((dx dx + dy dy) + dz dz) between m and region_pts[b][j], the lowest
 *   j on ties.
 * Outputs (must not alias anything): face int32 [B][S*S] (index local to the crop's range, background
 * -1), depth f32 [B][S*S] (0), coord f32 [B][3][S*S] (metres, 0), normal f32 [B][3][S*S] (0), region int32
 * [B][S*S] (0); cover_frame u8 [B][H][W] (optional; H, W unused without it): 1 = covered / 0 written at
 * (rmin + y, cmin + x) only, the obj_mask krrn_crop_inputs_u8 reads with frame[b] = b; the rest of the
 * frame is not touched. Host checks: null pointer or overlapping buffers KRRN_EARG; S outside 1..480, NR
 * outside 1..256, B, Vtot < 1, Ftot < 0, or cover_frame with H < S or W < S KRRN_ESHAPE. face_range and rc
 * are device memory, so the kernel guards them: a negative first face or count is an empty range, a range
 * is cut at Ftot, and a cover_frame pixel off the frame is not written. One launch, one block per 16x16
 * tile, no atomics, no workspace: a crop's maps do not depend on the rest of the batch, bit for bit. */
int krrn_raster_maps_f32(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                         const double* R, const double* t, const float* K4, const int* rc, int S,
                         const float* region_pts, int NR, int B, int* face, float* depth, float* coord,
                         float* normal, int* region, unsigned char* cover_frame, int H, int W, void* stream);

/* The pointwise masking of batchdataset.py:663-671, 689-694, 755-759 on the maps above. point_mask u8
 * [B][HW]: the crop's mask of krrn_crop_inputs_u8 with obj_mask = cover_frame (label * depth * cover);
 * cls int64 [B]; extent, lfborder f64 [B][3]. xyz f32 [B][3][HW] = float((coord - lfborder) / extent)
 * where the mask is set, else 0; normal is masked in place; region int64 [B][HW] = region_raw masked;
 * mask f32 [B][HW]; multi_cls_mask int64 [B][HW] = mask * (cls + 1); mask_obj f32 [B][HW] (optional,
 * needs face) = face >= 0. Departure from the reference: it zeroes xyz element-wise where a coordinate
 * component is exactly 0 (xyz_map * (coordinate != [0, 0, 0]), :694); here the mask is coverage, so a
 * surface point on a model-frame axis plane keeps its normalised coordinate. */
int krrn_gt_maps_finish_f32(const float* coord, const int* region_raw, const int* face,
                            const unsigned char* point_mask, const long long* cls, const double* extent,
                            const double* lfborder, int B, int HW, float* xyz, float* normal, long long* region,
                            float* mask, long long* multi_cls_mask, float* mask_obj, void* stream);

/* BOP-19 pose errors (Hodan et al., "BOP Challenge 2020 on 6D Object Localization", ECCV-W 2020), written
 * from the published definition; not compared against the BOP toolkit's output. One stated departure:
 * pixels are sampled at their integer coordinates (this project's rasteriser convention, above).
 *
 * VSD, the visible surface discrepancy, of B estimates. verts / faces / face_range / K4 as
 * krrn_raster_maps_f32; R_est, R_gt f64 [B][9], t_est, t_gt f64 [B][3]; depth f32 [F][H][W] the observed
 * frames in raw units, frame int32 [B] the frame of crop b, depth_scale raw units per metre; diameter f64
 * [B] metres; delta metres (BOP-19: 0.015); taus f64 [T], 1 <= T <= 16, fractions of the diameter (BOP-19:
 * 0.05, 0.10 .. 0.50). Per crop over the whole H x W frame, in f64 without FMA contraction:
 *   D_est(p), D_gt(p) = krrn_raster_maps_f32's depth z at the integer pixel p = (col, row) with rmin = cmin
 *   = 0 under the estimated / the GT pose (the same face test, skip rules, strict < and lowest-face-index
 *   tie rule: one device function, csrc/krrn_raster.h); 0 where no face covers p.
 *   D_obs(p) = (double)depth[frame[b]][row][col] / depth_scale; all zero for a frame index outside [0, F).
 *   xn = (col - cx) / fx, yn = (row - cy) / fy, ray = sqrt((xn xn + yn yn) + 1.0); a depth d > 0 becomes the
 *   distance from the camera centre d ray, anything else (0, negative, NaN) the distance 0.
 *   visib(model) = (obs > 0 && model > 0 && (model - obs) <= delta) || (obs == 0 && model > 0)   ("bop19")
 *   V_gt = visib(dist_gt); V_est = visib(dist_est) || (V_gt && dist_est > 0)
 *   inter = V_gt && V_est; union = V_gt || V_est; cost = |dist_gt - dist_est| / diameter[b] on inter
 *   step_k = #{p in inter: cost >= taus[k]};  e_vsd[b][k] = (step_k + (union - inter)) / union, 1.0 if union = 0
 * Outputs: counts int32 [B][2 + T] = (union, inter, step_0 .. step_{T-1}); e_vsd f64 [B][T] (one f64 division
 * of the integers). ws: krrn_bop_vsd_ws(B) ints (the two projected bounding boxes per crop; tiles of the
 * frame outside both do no work). The per-crop counts are summed over the tiles with integer atomicAdd (no
 * per-tile workspace, no second pass): integer sums do not depend on order, so the result is deterministic
 * and a crop's does not depend on the rest of the batch, bit for bit. Neither depth image is written to
 * memory. Host checks: null or overlapping buffers KRRN_EARG; B, Vtot, F, H, W < 1, Ftot < 0, T outside
 * 1..16, delta or depth_scale not > 0 KRRN_ESHAPE. frame and face_range are device memory and guarded by the
 * kernel (a bad face range is an empty range). */
int krrn_bop_vsd_ws(int B, long long* n_ints);
int krrn_bop_vsd_f32(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                     const double* R_est, const double* t_est, const double* R_gt, const double* t_gt,
                     const float* K4, const float* depth, int F, int H, int W, const int* frame, double depth_scale,
                     const double* diameter, double delta, const double* taus, int T, int B, int* ws, int* counts,
                     double* e_vsd, void* stream);

/* Ground-truth visibility of B object instances: what BOP's calc_gt_masks / calc_gt_info scripts compute on the
 * CPU, with VSD's render and VSD's visibility rule. verts / faces / face_range / K4 / depth / frame / depth_scale
 * as krrn_bop_vsd_f32; R f64 [B][9], t f64 [B][3]: one pose per instance. Per instance b over the whole H x W
 * frame, with D(p), D_obs(p), ray and the depth-to-distance conversion exactly as above (one depth walk under
 * (R, t); dist = D ray where D > 0, else 0; obs likewise from D_obs):
 *   mask[b][row][col]       = D(p) > 0
 *   mask_visib[b][row][col] = visib(dist), the "bop19" rule above (obs == 0 && dist > 0 included)
 * Both planes u8 [B][H][W] of 0 / 1; either may be NULL (not written). Every byte of a requested plane is defined
 * after the call: the entry point zeroes the planes (hipMemsetAsync) before the tiles that a face can reach
 * store theirs. info int32 [B][11] = px_count_all = #mask, px_count_valid = #(mask && obs > 0), px_count_visib =
 * #mask_visib, bbox_obj (x, y, w, h) of mask, bbox_visib (x, y, w, h) of mask_visib, with BOP's calc_2d_bbox
 * convention w = x_max - x_min, h = y_max - y_min over the set pixels (a single pixel has w = h = 0); a box with
 * no pixel is (-1, -1, -1, -1). visib_fract f64 [B] = px_count_visib / px_count_all (one f64 division), 0.0 when
 * px_count_all == 0. Stated departures from BOP's scripts: bbox_obj is clipped to the frame (BOP renders the
 * silhouette into a 3 x larger window), and pixels are sampled at their integer coordinates. ws:
 * krrn_bop_visib_ws(B) ints (per instance the projected bounding box, the three counts and the two boxes' lo /
 * hi bounds). Counts are integer atomicAdd, bounds integer atomicMin / atomicMax over the tiles: order-free, so
 * the result is deterministic and an instance's does not depend on the rest of the batch, bit for bit. Host
 * checks, before any HIP call: null pointer (mask and mask_visib exempt) or overlapping buffers KRRN_EARG; B,
 * Vtot, F, H, W < 1, Ftot < 0, delta or depth_scale not > 0 KRRN_ESHAPE. frame and face_range are guarded by the
 * kernel as in VSD: a bad face range is an empty range, a frame index outside [0, F) observes nothing. */
int krrn_bop_visib_ws(int B, long long* n_ints);
int krrn_bop_visib_u8(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                      const double* R, const double* t, const float* K4, const float* depth, int F, int H, int W,
                      const int* frame, double depth_scale, double delta, int B, int* ws,
                      unsigned char* mask, unsigned char* mask_visib, int* info, double* visib_fract,
                      void* stream);

/* Decode n run-length encoded masks (COCO RLE, the `segmentation` of BOP's detection files) into u8 planes.
 * counts int32: the run lengths of the n masks, concatenated; offs int32 [n + 1] (device memory): mask i owns
 * runs offs[i] .. offs[i + 1] - 1. COCO's semantics: pixels are numbered column-major, p = x H + y; the first run
 * is zeros and the runs alternate; a run may have length 0. With ends = the inclusive prefix sums of mask i's runs,
 *   mask[i][y][x] = 1 iff #{k : ends[k] <= p} is odd, else 0
 * which needs no special case for a zero-length run, and gives a pixel at or past the runs' total the parity of
 * the run count. mask u8 [n][H][W] row-major at any byte address: every byte of it is written by the call (no
 * memset by the caller or the entry point). info int32 [n][5] = (pixel count, x, y, w, h): the number of set
 * pixels and their tight box in BOP's convention w = x_max - x_min, h = y_max - y_min; a mask without a set pixel
 * gives 0, 0, 0, 0, 0. The entry point writes every info row itself. ends: int32 workspace of offs[n] elements
 * (the prefix sums, saturated at H W so that they never wrap). Integer work without atomics: the result is
 * deterministic and a mask's does not depend on the rest of the batch. For any counts (a negative one counts as 0)
 * the kernels read counts / ends only inside [offs[i], offs[i + 1]) and write only mask i's plane and info row;
 * a range that is negative, reversed or past offs[n] is an empty one (an all-zero mask). Host checks, before any
 * HIP call: null counts / offs / ends / mask / info KRRN_EARG; n < 0, H <= 0, W <= 0 or H W > INT32_MAX
 * KRRN_ESHAPE; n == 0 returns 0 and launches nothing. */
int krrn_rle_decode_u8(const int* counts, const int* offs, int n, int H, int W, int* ends, unsigned char* mask,
                       int* info, void* stream);

/* Encode n u8 planes as run-length encoded masks (COCO RLE): the inverse of krrn_rle_decode_u8, and what the host's
 * rle.encode returns. mask u8 [n][H][W] row-major at any byte address; any non-zero byte is a set pixel. Pixels are
 * numbered column-major, p = x H + y; v(p) = 1 for a set pixel and v(-1) = 0. The transitions are the p in [0, H W)
 * with v(p) != v(p - 1), in increasing order t_0 .. t_{T-1}, and the runs are
 *   t_0, t_1 - t_0, .., t_{T-1} - t_{T-2}, H W - t_{T-1}        (T + 1 of them; the one run H W when T = 0)
 * so a set pixel (0, 0) gives a leading 0, and set pixels at the bottom of column x and the top of column x + 1 are
 * one run. Outputs: n_runs int32 [n] = T + 1, always the true count (INT32_MAX where T + 1 would pass it); counts
 * int32 [n][max_runs]: mask i's runs k < min(n_runs[i], max_runs) in counts[i][k], and 0 in the elements from
 * n_runs[i] to max_runs, so every element of
 * counts is written by the call and nothing is written past a mask's slot (a mask with n_runs[i] > max_runs holds the
 * first max_runs runs: encode again with a larger slot); info int32 [n][5] = (pixel count, x, y, w, h) exactly as
 * krrn_rle_decode_u8 defines it (w = x_max - x_min, h = y_max - y_min; five zeros for an empty mask). ws: int32
 * workspace of krrn_rle_encode_ws(n, W) elements (per mask and column: the transitions, set pixels, lowest / highest
 * set row and last transition of the column, then the index of its first run and the last transition before it).
 * Integer work without atomics, and no block waits for another: the result is deterministic and a mask's does not
 * depend on the rest of the batch, bit for bit. Nothing is read back (the call can be captured in a graph). Host
 * checks, before any HIP call: null mask / ws / counts / n_runs / info (n_ints for _ws) KRRN_EARG; n < 0, H <= 0,
 * W <= 0, H W > INT32_MAX or max_runs < 1 KRRN_ESHAPE; n == 0 returns 0 and launches nothing. */
int krrn_rle_encode_ws(int n, int W, long long* n_ints);
int krrn_rle_encode_u8(const unsigned char* mask, int n, int H, int W, int max_runs, int* ws, int* counts,
                       int* n_runs, int* info, void* stream);

/* Paste the mask head's logits into full-frame planes: B crops, each the S x S window of its H x W frame whose top
 * left pixel is (rmin, cmin), to u8 masks that krrn_rle_encode_u8 takes. logits f32: crop b, channel c, pixel (i, j)
 * at logits[b ld_b + (c S + i) S + j], ld_b >= C1 S S (a channel slice of a wider tensor is passed as it lies);
 * chan int32 [B], rc int32 [B][2] = (rmin, cmin), device memory. The label convention is multi_cls_mask = mask (cls +
 * 1): channel 0 is background and channel cls + 1 the object. Per crop pixel, with ordinary IEEE comparisons,
 *   best = 0; for c = 1 .. C1 - 1: if (l[c] > l[best]) best = c
 * so ties go to the lowest channel, -0.0 ties with +0.0, a NaN logit never wins and a NaN in channel 0 leaves best =
 * 0. The pixel is set iff (1 <= chan[b] < C1 and best == chan[b]) or (chan[b] == 0 and best != 0: any foreground);
 * any other chan[b] sets nothing. Crop pixel (i, j) is frame pixel (rmin + i, cmin + j); pixels outside [0, H) x
 * [0, W) are dropped. The differences are taken in 64-bit: any rc, INT32_MIN / INT32_MAX included, reads and writes
 * nothing out of bounds. Outputs: mask u8 [B][H][W] row-major at any byte address, every byte written by the call, 1
 * where set and 0 elsewhere (no memset by the caller or the entry point); info int32 [B][5] = (pixel count, x, y, w,
 * h) exactly as krrn_rle_decode_u8 defines it (w = x_max - x_min, h = y_max - y_min; five zeros for an empty mask),
 * every row written by the entry point. Two launches: 16 x 16 frame tiles, a block per span of 8 side by side and
 * crop (a tile the window cannot touch stores zeros without reading a logit), then for info one block per crop that
 * reduces the plane's bytes inside the clipped window in a fixed order: no atomics. Comparisons and integer work
 * only: the result is deterministic and a crop's does not depend on the rest of the batch, bit for bit. Nothing is
 * read back (the call can be captured in a graph). Host checks, before any HIP call: null logits / chan / rc /
 * mask / info or overlapping buffers KRRN_EARG; B < 0, C1 < 1, S < 1, H <= 0, W <= 0, H W > INT32_MAX, C1 S S >
 * INT32_MAX or ld_b < C1 S S KRRN_ESHAPE (shapes are tested before overlap, whose extents they give); B == 0
 * returns 0 and launches nothing. */
int krrn_mask_paste_f32(const float* logits, long long ld_b, int C1, int S, const int* chan, const int* rc, int B,
                        int H, int W, unsigned char* mask, int* info, void* stream);

/* MSSD / MSPD, the maximum symmetry-aware surface / projection distance. verts f32 [Vtot][3] (all mesh
 * vertices), vert_range int32 [B][2] = first vertex, count of crop b; syms f64 [NStot][12] = row-major R
 * then t (metres, model frame), sym_range int32 [B][2] (each object's set begins with the identity). Per
 * vertex p = (x, y, z) and symmetry S, in f64 without FMA contraction:
 *   e = ((Re0 x + Re1 y) + Re2 z) + te;  s = ((S0 x + S1 y) + S2 z) + St;  g = ((Rg0 s.x + Rg1 s.y) + Rg2 s.z) + tg
 *   d3 = sqrt(((e-g).x^2 + (e-g).y^2) + (e-g).z^2)
 *   du = (fx e.x / e.z + cx) - (fx g.x / g.z + cx), dv likewise; d2 = sqrt(du du + dv dv); a NaN d counts as +inf
 *   mssd[b] = min_S max_p d3 (metres), mspd[b] = min_S max_p d2 (pixels)
 * max and min do not depend on order: any decomposition gives the same bits (here: 16 blocks per crop, each
 * over a contiguous slice of the symmetries, then the minimum over the slices in order; ws holds the slices'
 * minima, krrn_bop_mssd_mspd_ws(B) doubles). sym_idx int32 [B][2] (optional) = the lowest index, local to the
 * crop's range, of a symmetry attaining mssd / mspd (-1 if none is finite). An empty (or bad: guarded like
 * face_range) vertex or symmetry range gives +inf. Host checks: null or overlapping buffers KRRN_EARG; B,
 * Vtot, NStot < 1 KRRN_ESHAPE. */
int krrn_bop_mssd_mspd_ws(int B, long long* n_doubles);
int krrn_bop_mssd_mspd_f32(const float* verts, int Vtot, const int* vert_range, const double* R_est,
                           const double* t_est, const double* R_gt, const double* t_gt, const float* K4,
                           const double* syms, int NStot, const int* sym_range, int B, double* ws, double* mssd,
                           double* mspd, int* sym_idx, void* stream);

/* Matching estimates to ground-truth instances, the BOP toolkit's match_poses (greedy, not an optimal
 * assignment), for G groups at once; a group is one (scene, image, object) target. score f64 [Etot] the
 * estimates' confidences; est_range int32 [G][2] = (first estimate, n_est) into score; gt_range int32 [G][2] =
 * (first instance, n_gt) into the instance axis of `match`; pair_off int32 [G] = the group's first row in err f64
 * [Ptot][C]: a group owns n_est n_gt rows, estimate-major, row(e, j) = pair_off + e n_gt + j. The C columns are the
 * error functions (T VSD taus, then MSSD, then MSPD: 3 <= C <= 18); thr f64 [G][C][NT] the thresholds of
 * correctness, 1 <= NT <= 16, per group because MSSD's scale with the object's diameter; n_top int32 [G]: only the
 * n_top best-scored estimates of the group take part, a value <= 0 means all of them. Each cell (g, c, k) is matched
 * on its own:
 *   order the group's estimates by score descending, ties to the lower index, a NaN score as -inf; keep the first
 *   n_top; for each estimate e in that order, among the group's still unmatched instances j with
 *   err[row(e, j)][c] < thr[g][c][k] (strict; a NaN error never matches) take the one with the lowest error, ties
 *   to the lowest j, and mark it matched.
 * Outputs, every element written by the call, for empty groups as well: match int32 [GTtot][C][NT] = the global
 * index (into score) of the estimate matched to that instance, or -1; tp int32 [G][C][NT] = the number of matched
 * instances. The groups' instance ranges must not overlap; an instance that no group owns keeps what the buffer
 * held. Limits: n_est <= max_est <= 128 and n_gt <= max_gt <= 128, which the caller states because the ranges are
 * device memory. The kernel honours them: a group with n_est > max_est, n_gt > max_gt, a negative range, estimates
 * past Etot or pair rows past Ptot is matched as a group without estimates (tp 0, its instances -1), and an
 * instance range that leaves [0, GTtot) owns no instance; nothing outside the buffers is read or written.
 * Comparisons only (no arithmetic on errors or scores), no atomics, one block per group: the result is
 * bit-reproducible and a group's outputs do not depend on the rest of the batch. Host checks, before any HIP call:
 * null est_range / gt_range / pair_off / thr / n_top / tp, null score with Etot > 0, err with Ptot > 0 or match with
 * GTtot > 0 KRRN_EARG; G, Etot, GTtot or Ptot < 0, Ptot > INT32_MAX, C outside 3..18, NT outside 1..16, max_est or
 * max_gt outside 0..128 KRRN_ESHAPE; G == 0 returns 0 and launches nothing. */
int krrn_bop_match_f64(const double* score, int Etot, const double* err, long long Ptot, int C,
                       const int* est_range, const int* gt_range, const int* pair_off, const double* thr, int NT,
                       const int* n_top, int G, int GTtot, int max_est, int max_gt, int* match, int* tp,
                       void* stream);

/* What BOP's calc_model_info script computes for O object models at once: the diameter (squared) and the axis-aligned
 * box. verts f32 [Vtot][3] in any unit; vert_range int32 [O][2] = (first vertex, count), device memory; max_v: the
 * caller's bound on the counts, from which the grid is sized (as max_est / max_gt above). Per object o, in f64 without
 * FMA contraction:
 *   d2[o]     = max over the object's vertex pairs (i, j) of ((dx dx + dy dy) + dz dz), dx = (double)x_i - (double)x_j;
 *               the walk takes a term with > starting from 0.0, so a NaN term never wins and 0 or 1 vertices give 0.0
 *   box[o][6] = per axis the minimum (x, y, z), then the maximum (x, y, z), over the object's vertices, taken with < / >
 *               from +inf / -inf: a NaN coordinate is ignored and an empty range leaves +inf / -inf
 * The root is not taken: the diameter is sqrt(d2[o]) on the host. The kernels guard the ranges: a negative first or
 * count, a count above max_v or a range reaching past Vtot is an empty range (not cut). max and min do not depend on
 * order, so any decomposition gives the same bits. Here: one block per object for the box; for d2 up to 512 blocks
 * per object stride over row tiles of 256 vertices held in registers while the column vertices pass through LDS 1024
 * at a time, the column tiles below the diagonal skipped, and each block's maximum is folded with an integer
 * atomicMax on the bit pattern of the non-negative double (order-free; no floating-point atomics, no workspace). An
 * object's outputs do not depend on what else is in the batch, bit for bit. Host checks, before any HIP call: null or
 * overlapping buffers KRRN_EARG; O outside 1..65535, Vtot or max_v < 1 KRRN_ESHAPE. */
int krrn_model_extent_f64(const float* verts, int Vtot, const int* vert_range, int O, int max_v, double* d2,
                          double* box, void* stream);

/* How well each declared symmetry maps an object's mesh onto itself. verts / faces / face_range as
 * krrn_raster_maps_f32 (faces index into verts; a face with an index outside [0, Vtot) is skipped); vert_range int32
 * [O][2]; syms f64 [NStot][12] = row-major S then St (bop.symmetry_set rows, in the vertices' unit), sym_range int32
 * [O][2]; max_v / max_f: the caller's bounds on the vertex / face counts. The ranges are device memory and guarded as
 * in krrn_model_extent_f64 (a bad range is an empty one). Per symmetry s of object o, in f64 without FMA contraction:
 *   res2[s] = max over the object's vertices p of  min over the object's faces of dist2(S p, triangle)
 *   S p = ((S0 x + S1 y) + S2 z) + St; every dot product u.v = (ux vx + uy vy) + uz vz; the corners a, b, c are the
 *   f32 vertices widened to f64. The closest point q, the first test that holds deciding:
 *     ab = b - a, ac = c - a, ap = p - a; d1 = ab.ap, d2 = ac.ap;      d1 <= 0 && d2 <= 0           -> q = a
 *     bp = p - b; d3 = ab.bp, d4 = ac.bp;                              d3 >= 0 && d4 <= d3          -> q = b
 *     vc = d1 d4 - d3 d2;                                              vc <= 0 && d1 >= 0 && d3 <= 0 -> q = a + (d1 / (d1 - d3)) ab
 *     cp = p - c; d5 = ab.cp, d6 = ac.cp;                              d6 >= 0 && d5 <= d6          -> q = c
 *     vb = d5 d2 - d1 d6;                                              vb <= 0 && d2 >= 0 && d6 <= 0 -> q = a + (d2 / (d2 - d6)) ac
 *     va = d3 d6 - d5 d4;  va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0  -> q = b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) (c - b)
 *     otherwise den = 1.0 / ((va + vb) + vc);                          q = (a + ab (vb den)) + ac (vc den)
 *   dist2 = (p - q).(p - q). A triangle collapsed to a point, or to a line with three distinct corners, gives a finite
 *   point; with a == b the third case can divide 0 by 0, and the NaN distance never wins the face walk.
 * The face walk takes a distance with < from +inf (a NaN never wins), the vertex walk with > from 0.0; a vertex none of
 * whose distances is finite (a NaN vertex) contributes +inf, so broken input shows as an infinite residual. No vertices
 * give 0.0; vertices with an empty (or bad) face range give +inf. Every res2[s] that an object owns is written by the
 * call; the objects' symmetry ranges must not overlap (the lowest object wins), and a symmetry that no object's
 * sym_range owns keeps what the buffer held. One block per (symmetry, tile of 256 vertices) with the transformed
 * vertices in registers, the faces' nine f64 coordinates staged through LDS 256 at a time, and the same integer
 * atomicMax fold: order-free, so a symmetry's residual does not depend on what else is in the batch, bit for bit.
 * Host checks, before any HIP call: null (faces only with Ftot > 0) or overlapping buffers KRRN_EARG; O, Vtot, NStot,
 * max_v, max_f < 1, Ftot < 0, or NStot x min(ceil(max_v / 256), 256) > 2^23 KRRN_ESHAPE. */
int krrn_symmetry_residual_f64(const float* verts, int Vtot, const int* faces, int Ftot, const int* vert_range,
                               const int* face_range, const double* syms, int NStot, const int* sym_range, int O,
                               int max_v, int max_f, double* res2, void* stream);

/* n points drawn uniformly on the surface of each of O triangle meshes (area-weighted face choice, then the
 * square-root barycentric map: the reference's tools/script/sample_model.py random_point), with the face's flat normal.
 * verts f32 [Vtot][3] / faces int32 [Ftot][3] as krrn_symmetry_residual_f64; face_range int32 [O][2], device memory,
 * guarded as in krrn_model_extent_f64 (a bad range is an empty one) with max_f the caller's bound on the face counts;
 * row_id int32 [O], each >= 0: the generator row of each object (an object's samples depend on its row, the seed and
 * stream_id only, not on its place in the call). cum f64 [O][max_f]: caller-owned workspace and output; pts, nrm f32
 * [O][n][3]; face int32 [O][n]; status int32 [O]. Per object of F faces, in f64 without FMA contraction, every product
 * and sum rounded on its own:
 *   weight   face k (numbered within the range) with corners a, b, c widened to f64: e1 = b - a, e2 = c - a,
 *            N = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), A2 = (Nx Nx + Ny Ny) + Nz Nz,
 *            w_k = sqrt(A2) if A2 > 0 && A2 < inf, else 0 (a NaN corner falls out through the comparison); a face with
 *            an index outside [0, Vtot) has w_k = 0
 *   cum      in tiles of 256 faces: within tile j, run starts at 0 and takes run = run + w_k in face order;
 *            cum[k] = base_j + run with base_0 = 0 and base_{j+1} = base_j + (tile j's last run). Non-decreasing by
 *            construction; total = cum[F - 1], and the surface area is total / 2
 *   draws    sample i: r_q = the generator's value 4 i + q of (seed, stream_id, row_id[o]), q = 0..3 (the generator
 *            of krrn_randperm_i32)
 *   face     m = ((r0 << 32) | r1) >> 11 (53 bits), target = ((double)m * 2^-53) * total; the sample's face is the
 *            first k with cum[k] > target, or F - 1 if none (only a total that is not finite gets there): a face of
 *            weight 0 is never chosen
 *   point    u1 = (double)r2 * 2^-32, u2 = (double)r3 * 2^-32, s = sqrt(u1); wa = 1 - s, wb = s * (1 - u2), wc = s * u2;
 *            per axis p = (wa a + wb b) + wc c, cast once to f32
 *   normal   N / w_k per component, cast once to f32 (the flat normal in the faces' winding)
 * total == 0 (an empty or bad range, or only faces of weight 0) gives status 1, pts = nrm = 0 and face = -1; otherwise
 * status 0. (A face reached through `none` whose index leaves [0, Vtot) keeps pts = nrm = 0.) Three launches: a thread
 * per face stores w_k into cum; one block per object forms the tile runs (a thread per tile) and walks the tile bases
 * in order; a thread per sample draws, searches its object's cum row by bisection and stores. No atomics, no
 * floating-point value combined across lanes, no workspace beyond cum, no read-back: bit-reproducible, and an
 * object's outputs do not depend on what else is in the batch. Host checks, before any HIP call: a null buffer (faces
 * only with Ftot > 0) KRRN_EARG; O outside 1..65535, Vtot < 1, Ftot < 0, max_f < 1 or n outside 1..2^28 (4 i + 3 stays
 * inside 32 bits) KRRN_ESHAPE. */
int krrn_surface_sample_f64(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                            const int* row_id, int O, int max_f, int n, long long seed, unsigned int stream_id,
                            double* cum, float* pts, float* nrm, int* face, int* status, void* stream);

/* IoU of P pairs of run-length encoded masks, from the run lists alone: no plane is decoded and no H or W is
 * needed (a mask is its runs). counts int32 [n_counts]: the run lengths of the n masks, concatenated; offs int32
 * [n + 1] (device memory): mask i owns counts[offs[i] .. offs[i + 1]), as krrn_rle_decode_u8 takes them; pair int32
 * [P][2] = (detection mask, ground-truth mask); crowd u8 [P] (optional, NULL = no crowd). For mask m with runs c_0 ..
 * c_{n-1} (a negative count counts as 0):
 *   e_k   = the inclusive prefix sum of the runs, saturated at INT32_MAX (as the decoder saturates at H W); e_{-1} = 0
 *   the set runs are the odd k, covering the pixels [e_{k-1}, e_k); area(m) = the sum of the odd runs' e_k - e_{k-1}
 *   s_k   = the sum of the odd runs with index <= k, s_{-1} = 0
 *   F_m(p) = the number of set pixels of m with index < p: with j = #{k : e_k <= p}, F_m(p) = s_{n-1} for j >= n,
 *            else s_{j-1} + (j odd ? p - e_{j-1} : 0)
 *   inter(a, b) = sum over a's odd k of F_b(e^a_k) - F_b(e^a_{k-1});   union = area(a) + area(b) - inter
 *   iou = inter / union in f64: one correctly rounded division of two integers; where crowd[p] is set, iou = inter /
 *   area(a) (a = the detection); iou = 0.0 where the denominator is 0.
 * Unlike the decoder, a pixel at or past the runs' total is never set. Outputs, every element written by the call:
 * inter int32 [P], iou f64 [P], area int32 [n]. ws: int32 workspace of krrn_rle_iou_ws(n_counts) elements (e, then
 * s). A pair naming a mask outside [0, n) gives inter = 0, iou = 0.0; a range that is negative, reversed or past
 * min(offs[n], n_counts) is an empty mask (area 0, so inter = 0 and iou = 0.0). Nothing outside the buffers is read
 * or written. Two launches: one block per mask scans its runs into ws; then one wave per pair, whose lanes stride
 * over the set runs of the list with fewer runs and search the other list's e twice each (intersection is symmetric,
 * so the choice changes only the work), with a wave-wide integer add; a pair whose set spans [e_0, last odd end) do
 * not overlap stores 0 without a search. Integers only, no atomics, no read-back (the call can be captured in a
 * graph): a pair's result does not depend on the batch, bit for bit. Host checks, before any HIP call: null counts /
 * offs / pair / ws / inter / iou / area (n_ints for _ws) KRRN_EARG; n < 0, P < 0 or n_counts < 0 KRRN_ESHAPE; P == 0
 * and n == 0 returns 0 and launches nothing. */
int krrn_rle_iou_ws(int n_counts, long long* n_ints);
int krrn_rle_iou_f64(const int* counts, int n_counts, const int* offs, int n, const int* pair,
                     const unsigned char* crowd, int P, int* ws, int* inter, double* iou, int* area, void* stream);

/* IoU of P pairs of [x, y, w, h] boxes as plain rectangles. box f64 [n][4]; pair int32 [P][2] = (detection,
 * ground truth) and crowd u8 [P] (optional) as above. In f64 with every operation rounded on its own (no FMA
 * contraction), where max(u, v) = (v > u ? v : u) and min(u, v) = (v < u ? v : u):
 *   iw = max(0, min(ax + aw, bx + bw) - max(ax, bx));  ih likewise in y;  inter = iw ih
 *   area(m) = max(w, 0) max(h, 0);  den = area(a) + area(b) - inter, or area(a) where crowd[p] is set
 *   iou = den > 0 ? inter / den : 0.0
 * Outputs, every element written by the call: iou f64 [P], area f64 [n]. A pair naming a box outside [0, n) gives
 * 0.0. One thread per pair; no atomics, no read-back. Host checks, before any HIP call: null box / pair / iou / area
 * KRRN_EARG; n < 0 or P < 0 KRRN_ESHAPE; P == 0 and n == 0 returns 0 and launches nothing. */
int krrn_box_iou_f64(const double* box, int n, const int* pair, const unsigned char* crowd, int P, double* iou,
                     double* area, void* stream);

/* COCO's per-image matching (pycocotools' published COCOeval.evaluateImg) for G groups at once; a group is one
 * (scene, image, category). score f64 [Dtot] the detections' scores; det_range int32 [G][2] = (first detection,
 * n_det) into score / det_area; gt_range int32 [G][2] = (first ground truth, n_gt) into gt_area / gt_flags; pair_off
 * int32 [G] = the group's first element in iou f64 [Ptot]: a group owns n_det n_gt elements, detection-major, iou(d,
 * j) = iou[pair_off + d n_gt + j]. det_area f64 [Dtot], gt_area f64 [GTtot]; gt_flags int32 [GTtot]: bit 0 =
 * iscrowd, bit 1 = ignore; area_rng f64 [A][2] = (lo, hi), 1 <= A <= 8; iou_thr f64 [T], 1 <= T <= 16; max_det <=
 * 128 = COCO's maxDets. Each cell (g, a, t) is matched on its own:
 *   ig[j] = (gt_flags[j] != 0) or gt_area[j] < lo_a or gt_area[j] > hi_a (the bounds are inclusive)
 *   the ground truths are walked in the order: the j with ig[j] == 0 in index order, then the others in index order
 *   the detections are ordered by score descending, ties to the lower index, a NaN score as -inf; only the first
 *   max_det take part. For each detection d in that order: best = min(iou_thr[t], 1 - 1e-10), m = -1; for each j in
 *   the walk: skip j if it is already matched and not crowd; stop if m >= 0, ig[m] == 0 and ig[j] == 1; skip j if
 *   iou(d, j) < best or iou(d, j) is NaN; otherwise best = iou(d, j), m = j (an equal IoU moves to the later ground
 *   truth). If m >= 0: dt_match = m, dt_ig = ig[m], and m is marked matched. An unmatched detection has dt_ig =
 *   (det_area[d] < lo_a or det_area[d] > hi_a).
 * Outputs, every element of an owned detection or ground truth written by the call: dt_match int32 [Dtot][A][T] =
 * the global ground-truth index (into gt_area), or -1; dt_ig u8 [Dtot][A][T]; gt_ig u8 [GTtot][A] = ig; rank int32
 * [Dtot] = the detection's position in its group's order, or -1 at or past max_det (such a detection has dt_match =
 * -1, dt_ig = 1 in every cell). The groups' ranges must not overlap; an element that no group owns keeps what the
 * buffer held. Limits: n_det <= lim_det <= 128 and n_gt <= lim_gt <= 128, which the caller states because the ranges
 * are device memory. The kernel honours them: a group with n_det > lim_det, n_gt > lim_gt, a negative range, a range
 * past Dtot / GTtot or pair elements past Ptot is matched as an empty group: the detections its range owns inside
 * [0, Dtot) get rank -1, dt_match -1 and dt_ig 1, the ground truths it owns inside [0, GTtot) their gt_ig; nothing
 * outside the buffers is read or written. Comparisons only, no atomics, one block per group: the result is
 * bit-reproducible and a group's outputs do not depend on the rest of the batch. Written from the published
 * definition; not checked against pycocotools' own output. Host checks, before any HIP call: null det_range /
 * gt_range / pair_off / area_rng / iou_thr, null score / det_area / dt_match / dt_ig / rank with Dtot > 0, iou with
 * Ptot > 0, gt_area / gt_flags / gt_ig with GTtot > 0 KRRN_EARG; G, Dtot, GTtot or Ptot < 0, Ptot > INT32_MAX, A
 * outside 1..8, T outside 1..16, max_det, lim_det or lim_gt outside 0..128 KRRN_ESHAPE; G == 0 returns 0 and launches
 * nothing. */
int krrn_coco_match_f64(const double* score, int Dtot, const int* det_range, const int* gt_range, const int* pair_off,
                        const double* iou, long long Ptot, const double* det_area, const double* gt_area,
                        const int* gt_flags, int GTtot, const double* area_rng, int A, const double* iou_thr, int T,
                        int max_det, int lim_det, int lim_gt, int G, int* dt_match, unsigned char* dt_ig,
                        unsigned char* gt_ig, int* rank, void* stream);

/* Pose verification by render-and-compare: C candidate poses per crop scored against the observed depth frame
 * and the detector's mask, without a ground-truth pose, and the best one selected. verts / faces / face_range /
 * K4 / depth / frame / depth_scale as krrn_bop_vsd_f32; R f64 [B][C][9], t f64 [B][C][3], 1 <= C <= 8; mask u8
 * [F][H][W] (optional) the detector's mask frames (any non-zero byte is set); box int32 [B][4] (optional) =
 * (rmin, rmax, cmin, cmax) of the crop: rows [rmin, rmax), cols [cmin, cmax), clipped to the frame, NULL = the
 * whole frame; tau f64 [B] metres. For crop b and candidate c over the integer pixels p = (col, row) of the H x W
 * frame, in f64 without FMA contraction:
 *   m(p)    = D(p) ray where D(p) > 0, else 0: D the depth of the mesh rendered under (R[b][c], t[b][c]) exactly
 *             as VSD renders (the same device function, near plane, strict < and lowest-face tie), ray as above
 *   o(p)    = the observed distance exactly as VSD's obs: 0 for a hole, a non-positive or NaN sample, or a frame
 *             index outside [0, F)
 *   evid(p) = mask[frame[b]][row][col] != 0 && o > 0 && p inside the crop's box; a NULL mask gives no evidence
 *             anywhere. It does not depend on the candidate.
 *   diff    = m - o, where m > 0 and o > 0
 *   claim   = m > 0 && o > 0 && !(diff > tau[b])   (the render says the object's surface is seen here; a pixel
 *             with something more than tau in front of it is occluded and neutral)
 *   both    = claim && evid;   inter = claim && evid && fabs(diff) <= tau[b]
 * counts int32 [B][C][6] = #(m > 0) "render", #claim, #evid, #both, #inter, union = claim + evid - both.
 *   score[b][c] = union > 0 ? (double)inter / (double)union : 0.0   (f64 [B][C]: a depth-aware IoU between what
 *                 the pose claims is visible and where the detector's mask has depth)
 *   best[b]     = the lowest c with the largest score (strict > walking c upward); 0 when every score is 0
 * A NaN or behind-the-camera pose renders nothing and scores 0, so a failed solver never wins against a sane
 * candidate. R_sel f32 [B][9] / t_sel f32 [B][3] (each optional) = candidate best[b]'s pose rounded to f32. All
 * sums are integer atomicAdd over the tiles, so the result is deterministic and a (crop, candidate) pair's does
 * not depend on the batch or on the other candidates, bit for bit. ws: krrn_pose_score_ws(B, C) ints (the
 * candidates' projected bounding boxes; a tile outside the crop's box and all of them does no work). Host checks,
 * before any HIP call: null pointer (mask, box, R_sel, t_sel exempt) or overlapping buffers KRRN_EARG; C outside
 * 1..8, B, Vtot, F, H, W < 1, Ftot < 0, depth_scale not > 0 KRRN_ESHAPE. frame, face_range and box are device
 * memory and guarded by the kernel as in VSD. */
int krrn_pose_score_ws(int B, int C, long long* n_ints);
int krrn_pose_score_f32(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                        const double* R, const double* t, int C, const float* K4, const float* depth,
                        const unsigned char* mask, int F, int H, int W, const int* frame, const int* box,
                        double depth_scale, const double* tau, int B, int* ws, int* counts, double* score,
                        int* best, float* R_sel, float* t_sel, void* stream);

/* Render-based point-to-plane pose refinement on the depth frame, batched (this project's own definition: the
 * reference has none; tests/depth_refine_ref.py restates it in numpy f64). verts / faces / face_range / K4 / depth /
 * mask / frame / depth_scale as krrn_pose_score_f32; R0 f32 [B][9] row-major, t0 f32 [B][3]: the starting pose,
 * model to camera; max_dist f64 [B] metres; radius f64 [B] = rho, metres. Per crop, R, t = R0, t0 (f64 from there
 * on, without FMA contraction); pass k = 0, 1, ...:
 *   render   the crop's faces under (R, t) and K4 over the whole frame exactly as VSD renders (the same device
 *            function): depth z and winning face per pixel; n = the face's camera-frame normal as
 *            krrn_raster_maps_f32 defines it ((c1 - c0) x (c2 - c0) normalised, negated if n . c0 > 0; a zero or
 *            non-finite normal contributes nothing)
 *   observe  d = depth[frame][y][x] / depth_scale (no sample for a frame index outside [0, F)); a pixel is kept iff
 *            it is covered, d > 0, |d - z| < max_dist, and mask[frame][y][x] != 0 when mask is given
 *   points   xn = (x - cx) / fx, yn = (y - cy) / fy; p = z (xn, yn, 1), o = d (xn, yn, 1), r = n . (o - p)
 *   counts   K = kept pixels, err_k = sum r^2 / K
 *   stop, tested in this order (R, t as they stand are the result; rmse = sqrt(err_k), +inf for K = 0):
 *            K < min_pairs -> status 2 STARVED; k >= 1 and |err_{k-1} - err_k| <= tol err_{k-1} -> 0 CONVERGED;
 *            k == max_iter -> 1 MAX_ITER
 *   update   one damped Gauss-Newton step in a twist about the object's own centre t, rotation scaled by rho:
 *            J = [((p - t) / rho) x n, n], A = sum J J^T, b = sum J r, A += damp trace(A) / 6 I, 6 x 6 Cholesky;
 *            a non-positive or non-finite pivot or a non-finite solution keeps the pose from before the update
 *            and stops with 3 DEGENERATE; otherwise xi = (w, v): R <- exp(w / rho) R (Rodrigues), t <- t + v
 * Outputs: R f32 [B][9], t f32 [B][3] (a stop in pass 0 returns R0, t0 bit for bit), passes [B] = the k at the
 * stop, pairs [B] = the last K, rmse f32 [B], status [B] (the codes of krrn_icp_refine_f32). Per pass three
 * launches: the projected box of the crop's vertices; one block per 16 x 16 tile of the frame and crop, which
 * returns at once outside the box or for a finished crop, and otherwise writes its partial sums (21 + 6 + 1 f64 and
 * the count, reduced in a fixed order) to its own slot of ws; one block per crop that adds the box's slots in
 * row-major tile order, tests, solves and updates. max_iter + 1 rounds are enqueued whatever the data: nothing is
 * read back, no atomics, no block waits for another, and a crop's outputs do not depend on the rest of the batch,
 * bit for bit. NaN or inf in a pose, in K4 or in a depth sample ends in STARVED or DEGENERATE. ws:
 * krrn_pose_refine_depth_ws(B, H, W) bytes, 8-byte aligned. Host checks, before any HIP call: null pointer (mask
 * exempt) or overlapping buffers KRRN_EARG; B outside 1..65535, H, W, Vtot, F < 1, Ftot < 0, max_iter outside
 * 0..32, min_pairs < 6, tol or damp negative or not finite, depth_scale not > 0 KRRN_ESHAPE. frame and face_range
 * are device memory and guarded by the kernel as in VSD. */
int krrn_pose_refine_depth_ws(int B, int H, int W, long long* n_bytes);
int krrn_pose_refine_depth_f32(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                               const float* R0, const float* t0, const float* K4, const float* depth,
                               const unsigned char* mask, int F, int H, int W, const int* frame, double depth_scale,
                               const double* max_dist, const double* radius, int max_iter, double tol, int min_pairs,
                               double damp, int B, void* ws, float* R, float* t, int* passes, int* pairs, float* rmse,
                               int* status, void* stream);

/* Whole scenes in one z-buffer: every instance of a frame drawn under its own pose, one object hiding another (this
 * project's own definition; tests/scene_ref.py restates it in numpy f64). verts f32 [Vtot][3], faces int32 [Ftot][3]
 * (global vertex indices) and face_range int32 [N][2] as krrn_bop_vsd_f32 takes them, one range per instance; R f64
 * [N][9] row-major, t f64 [N][3] metres, K4 f32 [N][4] = (fx, fy, cx, cy): one pose and one camera per instance;
 * inst_range int32 [F][2] = (first instance, count) of frame f. For frame f and the integer pixel p = (col, row) of
 * the H x W frame, in f64 without FMA contraction:
 *   D_n(p), face_n(p)  the depth and the winning face of instance n's faces rendered under (R[n], t[n], K4[n])
 *                      exactly as VSD renders (the same device function: near plane 1e-3, both windings, the
 *                      inclusive bounding-box test, strict < on depth so equal depths go to the lowest face index)
 *   winner(p)          walking the frame's instances in increasing n, the one with the smallest D_n(p) under a
 *                      strict <: equal depths go to the lowest instance index
 *   inst  int32 [F][H][W]  the winner's index n in the whole list, -1 where no instance covers p
 *   depth f32 [F][H][W]    (float)D_winner(p), 0 where none
 *   shade u8 [F][H][W]     nrm = the winning face's camera-frame normal as krrn_raster_maps_f32 defines it (flat;
 *                          zero for a degenerate face); lam = fmin(fmax(-nrm[2], 0.0), 1.0); s = 64.0 + 191.0 lam;
 *                          shade = (unsigned char)(int)(s + 0.5); 0 where none
 * Every element of the three planes is written: the caller does no memset. Two launches: one block per instance
 * writes its projected vertices' bounding box to ws (krrn_scene_render_ws(N) ints); one block per 16 x 16 tile of a
 * frame skips the instances whose box misses the tile (which changes no output: the box is the outward-rounded hull,
 * in the walk's own bits, of every vertex a kept face can have), walks the others, keeps each pixel's best hit in
 * registers, and stores. No atomics, no block waits for another, nothing is read back, and a frame's planes do not
 * depend on the rest of the batch, bit for bit. Host checks, before any HIP call: null pointer or overlapping buffers
 * KRRN_EARG; N < 0, F < 1, Vtot < 1, Ftot < 0, H or W <= 0, H W > INT32_MAX KRRN_ESHAPE; N == 0 still writes the
 * empty planes. inst_range and face_range are device memory and guarded by the kernel as in VSD, against N and Ftot: a
 * negative first or count, or a first beyond the array, is an empty range; a range is cut at the array's end. */
int krrn_scene_render_ws(int N, long long* n_ints);
int krrn_scene_render_f64(const float* verts, int Vtot, const int* faces, int Ftot, const int* face_range,
                          const double* R, const double* t, const float* K4, const int* inst_range, int N, int F,
                          int H, int W, int* ws, int* inst, float* depth, unsigned char* shade, void* stream);

/* The picture of a rendered scene on its frame, integer work only. rgb u8 [F][H][W][3]; est int32 [F][H][W] and shade
 * u8 [F][H][W]: krrn_scene_render_f64's inst and shade planes; tint u8 [N][3]: a colour per instance; gt int32
 * [F][H][W] (optional): a second id plane, drawn as outlines only; out u8 [F][H][W][3]. An id of est outside [0, N)
 * counts as -1 everywhere. Per pixel p:
 *   c = rgb[p]
 *   if e = est[p] >= 0:  lit_k = (tint[e][k] shade[p] + 127) / 255;  c_k = (c_k (256 - alpha) + lit_k alpha + 128) >> 8
 *   edge_L(p) = L[p] >= 0 and some q with |dx|, |dy| <= radius inside the frame has L[q] != L[p]
 *   if edge_est(p):  c = tint[est[p]]
 *   if gt and edge_gt(p):  c = (gt_r, gt_g, gt_b)
 *   out[p] = c
 * Host checks, before any HIP call: null pointer (gt exempt) or out overlapping an input KRRN_EARG; N < 0, F < 1, H or
 * W <= 0, H W > INT32_MAX, alpha outside 0..256, radius outside 1..4, a colour outside 0..255 KRRN_ESHAPE. */
int krrn_scene_overlay_u8(const unsigned char* rgb, const int* est, const unsigned char* shade,
                          const unsigned char* tint, int N, int alpha, int radius, const int* gt, int gt_r, int gt_g,
                          int gt_b, int F, int H, int W, unsigned char* out, void* stream);

/* The signed difference between a rendered and an observed depth plane as colours. ren / obs f32 [F][H][W]; out u8
 * [F][H][W][3]. Per pixel, in f64 without FMA contraction: r = ren, o = obs / depth_scale;
 *   r > 0 and o > 0:  e = r - o;  k = (int)(fmin(fabs(e) / tol, 1.0) 255.0 + 0.5);
 *                     e > 0 (255, 255 - k, 255 - k): the model is behind the observed surface (hidden, or too far);
 *                     e < 0 (255 - k, 255 - k, 255);  e == 0 white
 *   else r > 0:       (128, 128, 128): rendered where nothing is observed
 *   else:             black
 * A NaN is never > 0. Host checks, before any HIP call: null pointer or out overlapping an input KRRN_EARG; F < 1, H
 * or W <= 0, H W > INT32_MAX, tol not finite or not > 0, depth_scale == 0 KRRN_ESHAPE. */
int krrn_scene_depth_diff_u8(const float* ren, const float* obs, double depth_scale, double tol, int F, int H, int W,
                             unsigned char* out, void* stream);

/* BPnP forward (lib/network/dnn/BPnP.py:43-44, cv2.solvePnP(SOLVEPNP_ITERATIVE,
 * useExtrinsicGuess=True)): Levenberg-Marquardt on sum_i ||pi(z_i; y) - x_i||^2 per crop, f64,
 * from y_init. pts2d [B][n][2] pixels; pts3d [n][3] shared (z_per_crop = 0) or [B][n][3];
 * K [3][3] row-major; y_init / y_out [B][6] = angle-axis (kornia convention) then t; R_init
 * [B][9] (optional): a rotation matrix replacing y_init's angle-axis (log map), e.g. the
 * krrn_pnp_ransac_f32 result as cv2.solvePnPRansac's rvec0 (BPnP.py:36-38); cost_out [B] final
 * squared error (optional). At most `iters` accepted steps (stops earlier once a step is below
 * 1e-13 relative). n >= 3. */
int krrn_bpnp_solve_f32(const float* pts2d, const float* pts3d, int z_per_crop, const float* K, const float* y_init,
                        const float* R_init, int B, int n, int iters, float* y_out, float* cost_out, void* stream);

/* BPnP backward (lib/network/dnn/BPnP.py:53-117): implicit-function gradients of the pose P6
 * [B][6] given grad_out [B][6]. grad_x [B][n][2]; grad_z [n][3] summed over crops (shared
 * points) or [B][n][3] (z_per_crop); grad_K [3][3] summed over crops. workspace:
 * B*(3n + 9) f64. Deterministic (crop-ordered sums). A singular J_fy gives NaN gradients for
 * that crop (the reference's torch.inverse raises). */
int krrn_bpnp_backward_f32(const float* pts2d, const float* P6, const float* pts3d, int z_per_crop, const float* K,
                           const float* grad_out, int B, int n, float* grad_x, float* grad_z, float* grad_K,
                           double* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* KRRN_HIP_H */
