/*
 * drn_wsod.h — C ABI of the MI355X-native DRN-WSOD / OICR hot path (libdrn_wsod_hip.so).
 *
 * Boundary contract:
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless a name ends in _host;
 *   - every entry point enqueues work on the given hipStream_t (passed as void*), never
 *     synchronises, never allocates, retains no pointers after returning; graph-capturable;
 *   - returns 0 (DRN_OK) or a negative code: -1 invalid argument, -2 launch failure,
 *     -3 unsupported; never throws across the ABI;
 *   - dtype codes: 0 = fp32 (parity mode, exact fp32 MFMA), 1 = bf16 (fast mode, fp32 accumulate);
 *   - feature maps are NHWC, matrices row-major with an explicit leading dimension in ELEMENTS.
 *
 * Each declaration cites the reference interface it replaces (paths relative to the reference
 * repository root).  INTEGRATION.md shows the Python-side binding a maintainer would add.
 */
#ifndef DRN_WSOD_H_
#define DRN_WSOD_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRN_OK 0
#define DRN_ERR_ARG (-1)
#define DRN_ERR_LAUNCH (-2)
#define DRN_ERR_UNSUPPORTED (-3)
#define DRN_F32 0
#define DRN_BF16 1

/* ---- backbone -------------------------------------------------------------------------------- */

/* GeneralizedRCNNWSL.preprocess_image, projects/WSL/wsl/modeling/meta_arch/rcnn.py:242-249 +
 * ImageList.from_tensors, detectron2/structures/image_list.py:57-119.
 * img_chw [C][H][W] f32 -> out_nhwc [Hp][Wp][Cp] (one image slot), (x-mean)/std, zero padded. */
int drn_preprocess_nhwc(const float* img_chw, int C, int H, int W, void* out_nhwc, int Hp, int Wp, int Cp,
                        const float* mean3_host, const float* std3_host, int dtype, void* stream);

/* ResizeTransform.apply_image on an 8-bit image (detectron2/data/transforms/transform.py:101-122: PIL.Image.resize(size,
 * BILINEAR)) [+ HFlipTransform], as DatasetMapperTTAAVG applies them 16 times per image
 * (projects/WSL/wsl/modeling/test_time_augmentation_avg.py:68-137), on the device.  Pillow (un-vendored, un-pinned dependency
 * of the reference; its published algorithm - Resample.c - is restated, and pinned bit for bit against the installed Pillow by
 * the tests): a horizontal then a vertical integer pass; output position i reads source positions [bounds[2i], bounds[2i] +
 * bounds[2i+1]) with coefficients coef[i * ks + j] scaled by 2^22, each pass rounds ((1 << 21) + sum) >> 22 and clips to 8 bits.
 * The caller computes bounds / coef with Pillow's double arithmetic (host side: ops.pil_bilinear_coeffs) and passes them as
 * DEVICE pointers; a NULL bounds pointer skips that pass (its size must not change).
 * src_hwc uint8 [H][W][C] (C <= 4), dst_chw fp32 [C][Ho][Wo] holding the integers 0 .. 255; flip != 0 mirrors the columns. */
int drn_resize_bilinear_u8(const void* src_hwc, int H, int W, int C, float* dst_chw, int Ho, int Wo, const int* xbounds,
                           const int* xcoef, int ksx, const int* ybounds, const int* ycoef, int ksy, int flip, void* stream);

/* The training DatasetMapper's image chain on the device, one launch per image: DatasetMapper.__call__
 * (detectron2/data/dataset_mapper.py:112-185) applies, to the decoded 8-bit image, fvcore's CropTransform (RandomCrop,
 * detectron2/data/transforms/augmentation_impl.py:232-281), ResizeTransform.apply_image
 * (detectron2/data/transforms/transform.py:101-122: PIL.Image.resize(size, BILINEAR)), fvcore's HFlipTransform and two
 * fvcore BlendTransforms (RandomBrightness / RandomSaturation, augmentation_impl.py:403-455).  fvcore and Pillow are
 * un-vendored dependencies of the reference; their published semantics are restated.
 * src_hwc uint8 [H][W][C], C in {1, 3, 4}; the crop window (x0, y0, cw, ch) must lie inside the image; the tables are those of
 * drn_resize_bilinear_u8 for cw -> Wo and ch -> Ho (DEVICE pointers; NULL skips that pass and its size must not change).
 * Per output pixel, op for op: R = the two-pass integer resample of the crop; the pixel goes to column Wo - 1 - x when flip;
 * brightness_on: B = (uint8) min(max(wb * (float) R, 0), 255), a float32 product, truncated; saturation_on (C == 3 only, else
 * DRN_ERR_ARG): g = ((double) B0 * 0.299 + (double) B1 * 0.587) + (double) B2 * 0.114 by channel index, uncontracted, and
 * out_c = (uint8) min(max(one_minus_ws * g + (double) (ws * (float) B_c), 0), 255), truncated; one_minus_ws is the host's
 * double 1 - w.  dst_chw fp32 [C][Ho][Wo] holding the integers 0 .. 255.  No byte outside [src, src + H*W*C) is read. */
int drn_augment_u8(const void* src_hwc, int H, int W, int C, int x0, int y0, int cw, int ch, float* dst_chw, int Ho, int Wo,
                   const int* xbounds, const int* xcoef, int ksx, const int* ybounds, const int* ycoef, int ksy, int flip,
                   int brightness_on, float wb, int saturation_on, double one_minus_ws, float ws, void* stream);
/* Host-side query, no launch: the LDS staging bytes drn_augment_u8 asks for at these sizes (xpass / ypass: whether that
 * direction has tables); 0 = the tile windows are too large to stage and the launch runs its one-thread-per-pixel path
 * (same bits).  Negative: invalid argument. */
long drn_augment_lds_bytes(int cw, int ch, int Ho, int Wo, int C, int xpass, int ypass);

/* Conv2d.forward = F.conv2d -> FrozenBatchNorm2d -> relu_ [+ residual add before the relu],
 * detectron2/layers/wrappers.py:94-99, detectron2/layers/batch_norm.py:45-65,
 * projects/WSL/wsl/modeling/backbone/resnet_ws.py:217-237, vgg.py:104-122.
 * x NHWC [Nb][H][W][Cin]; w [Cout][ldw] with k = (kh*KW + kw)*Cin + ci, rows zero-padded to a
 * multiple of 128 bytes; y [Nb*Ho*Wo][ldy]; y = act(conv*scale[c] + bias[c] (+ residual)). */
int drn_conv2d_nhwc(const void* x, const void* w, void* y, const float* scale, const float* bias,
                    const void* residual, int Nb, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                    int pad, int dil, long ldw, long ldy, long ldres, int relu, int dtype, void* stream);

/* The same convolution for the QUANTISED trunk (BASELINE configs[4], "fp8 MFMA conv path"; the reference is fp32 only -
 * SURVEY F5 - so the definition of record is the fp32 conv above with operands and activations rounded to fp8):
 * `dtype` (DRN_F32 / DRN_BF16 / DRN_FP8 = OCP e4m3fn, one byte) is the element type of x and w - DRN_FP8 runs
 * v_mfma_f32_32x32x16_fp8_fp8 with fp32 accumulation - while y is stored as `out_dtype` and the residual read as
 * `res_dtype` and multiplied by `res_mult`.  Per-tensor / per-output-channel quantisation scales live in the caller's
 * affine: with x stored as x*s_x, w[c] as w[c]*s_w[c], y as y*s_y and the residual as r*s_r the caller passes
 * scale[c] = bn_scale[c]*s_y/(s_x*s_w[c]), bias[c] = bn_bias[c]*s_y, res_mult = s_y/s_r (s_y = 1 for a bf16/fp32 y).
 * fp8 stores round to nearest even and saturate at +-448.  Cin*esize must be a multiple of 16 bytes. */
#define DRN_FP8 2
int drn_conv2d_nhwc_q(const void* x, const void* w, void* y, const float* scale, const float* bias,
                      const void* residual, int Nb, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                      int pad, int dil, long ldw, long ldy, long ldres, int relu, int dtype, int out_dtype,
                      int res_dtype, float res_mult, void* stream);

/* Host-side query, no launch: the kernel drn_conv2d_nhwc_q runs these arguments on, with the knobs (drn_tune) as they stand,
 * on a device of `cus` compute units (cus <= 0: the current device's; 256 when there is none).  The arguments are those of
 * drn_conv2d_nhwc_q without the stream; pointers are inspected for NULL and alignment, never dereferenced.  Returns a
 * DRN_CONV_KIND_* code, with DRN_CONV_KIND_FP8_K16 or-ed in when fp8 operands run the K = 16 MFMA form (DRN_TUNE_FP8_K64 = 0),
 * or DRN_ERR_ARG for exactly the arguments drn_conv2d_nhwc_q refuses.  Tests and tools read the kernel choice off it. */
#define DRN_CONV_KIND_PATCH_C64 1    /* conv3x3_c64_kernel: LDS-resident patch, 3x3 / 64 -> 64 channels of a large map */
#define DRN_CONV_KIND_PP256 2        /* conv1x1_pp_kernel: 1x1 on the 256x256 ping-pong GEMM mainloop */
#define DRN_CONV_KIND_PP8 3          /* pp8_kernel, the 128x128 form */
#define DRN_CONV_KIND_PP8_WIDE 4     /* pp8_kernel, the 256x128 form */
#define DRN_CONV_KIND_RING_64 5      /* conv_ring_kernel, 64x64 tile */
#define DRN_CONV_KIND_RING_128 6     /* conv_ring_kernel, 128x128 tile */
#define DRN_CONV_KIND_K2 7           /* conv_nhwc_k2_kernel: two K-groups per 64x64 tile */
#define DRN_CONV_KIND_KS 8           /* conv_nhwc_ks_kernel: 32x32 tile, wave-K-split */
#define DRN_CONV_KIND_TILED_64 9     /* conv_nhwc_kernel, 64x64 tile */
#define DRN_CONV_KIND_TILED_128X64 10 /* conv_nhwc_kernel, 128x64 tile */
#define DRN_CONV_KIND_TILED_128 11   /* conv_nhwc_kernel, 128x128 tile */
#define DRN_CONV_KIND_FP8_K16 0x100  /* flag: fp8 operands on the K = 16 non-scaled MFMA */
int drn_conv2d_plan(const void* x, const void* w, void* y, const float* scale, const float* bias, const void* residual, int Nb,
                    int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil, long ldw, long ldy, long ldres,
                    int relu, int dtype, int out_dtype, int res_dtype, float res_mult, int cus);

/* The tail of a 64-channel bottleneck block on a large map as ONE launch (BottleneckBlock.forward,
 * projects/WSL/wsl/modeling/backbone/resnet_ws.py:217-237: conv2 -> relu -> conv3 -> + shortcut -> relu [-> max pool]):
 * y = pool(act3((conv1x1(act2(conv3x3(x) * scale2 + bias2)) * scale3 + bias3) + residual * res_mult)), bf16;
 * x [Nb][H][W][64], w2 [64][ldw2] (3x3, pad = dil = stride = 1, packed as for drn_conv2d_nhwc), w3 [256][ldw3] (1x1 over
 * 64 channels), residual [Nb*H*W][256] or NULL, y [Nb*H*W][256].  The 3x3's output - rounded to bf16 exactly as
 * drn_conv2d_nhwc would store it - stays in LDS: bit for bit the result of the separate calls.
 * w3 == NULL: no 1x1 stage (the deep stem's last 3x3: y and the residual have 64 channels; needs pool).
 * pool != 0: nn.MaxPool2d(2, 2) (resnet_ws.py:214-215) applied in the epilogue - y is the pooled map
 * [Nb][(H - 2) / 2 + 1][(W - 2) / 2 + 1][channels], the full-resolution output is never written; needs the last ReLU.
 * Maps of >= 32768 pixels per image (the LDS-resident-patch kernel's class); DRN_ERR_UNSUPPORTED otherwise (callers then
 * run the separate launches). */
int drn_conv3x3_pw_nhwc(const void* x, const void* w2, const float* scale2, const float* bias2, int relu2, const void* w3,
                        const float* scale3, const float* bias3, const void* residual, void* y, int Nb, int H, int W,
                        long ldw2, long ldw3, float res_mult, int relu3, int pool, void* stream);

/* nn.MaxPool2d(kernel_size=2, stride=s, padding=0), resnet_ws.py:214-215,403; vgg.py:99-100.  DRN_FP8: non-negative
 * (post-ReLU) values only - they order like their bytes. */
int drn_maxpool2x2_nhwc(const void* x, void* y, int Nb, int H, int W, int C, int stride, int dtype, void* stream);

/* F.max_pool2d(x, kernel_size=3, stride=2, padding=1), the pool of the standard ResNet stem
 * (detectron2/modeling/backbone/resnet.py:355-359).  x [Nb][H][W][C] -> y [Nb][(H - 1) / 2 + 1][(W - 1) / 2 + 1][C]
 * (= (H + 2 - 3) / 2 + 1); padding never wins (it counts as -inf), any H, W >= 1; C * esize a multiple of 16 bytes.
 * DRN_F32 / DRN_BF16; DRN_FP8: non-negative (post-ReLU) values only, as for drn_maxpool2x2_nhwc. */
int drn_maxpool3x3s2_nhwc(const void* x, void* y, int Nb, int H, int W, int C, int dtype, void* stream);

/* The standard ResNet stem as ONE launch (BasicStem.forward, detectron2/modeling/backbone/resnet.py:355-359):
 * y = max_pool2d(relu(conv7x7(x, stride 2, pad 3) * scale + bias), 3, 2, 1), bf16.  x [Nb][H][W][8] (3 channels stored as
 * 8), w [64][ldw] packed as for drn_conv2d_nhwc (k = (kh * 7 + kw) * 8 + ci, zero padded), y the POOLED map
 * [Nb][(Ho - 1) / 2 + 1][(Wo - 1) / 2 + 1][64] with Ho = (H - 1) / 2 + 1; the half-resolution conv map is never written.
 * The conv output is rounded to bf16 exactly as drn_conv2d_nhwc stores it and the k order is that kernel's: bit for bit
 * the result of drn_conv2d_nhwc + drn_maxpool3x3s2_nhwc, for any H, W >= 1.
 * Class: dtype DRN_BF16, Cin (stored) 8, Cout 64, relu != 0, 16-byte aligned pointers; DRN_ERR_UNSUPPORTED otherwise
 * (callers then run the two launches). */
int drn_stem7x7_pool_nhwc(const void* x, const void* w, const float* scale, const float* bias, void* y, int Nb, int H, int W,
                          int Cin, int Cout, long ldw, int relu, int dtype, void* stream);

/* ---- backward of the conv trunk (MODEL.BACKBONE.FREEZE_AT < 5; torch.autograd of F.conv2d / max_pool2d) ---- *
 * conv dgrad runs drn_conv2d_nhwc on the flipped/transposed packed weights (every trained conv has stride 1,
 * resnet_ws.py:148-150), the FrozenBN-affine/ReLU backward runs drn_bias_act_bwd, and the weight gradient is
 * drn_gemm_nt(g^T, im2col_t): */

/* out[(ci*KH + kh)*KW + kw][p] = x[n, ho*s + kh*d - pad, wo*s + kw*d - pad, ci]  (x NHWC with channel stride ldc,
 * p = (n*Ho + ho)*Wo + wo, zeros outside the image; columns beyond p are left untouched). */
int drn_im2col_t(const void* x, void* out, int Nb, int H, int W, int Cin, int ldc, int KH, int KW, int stride, int pad,
                 int dil, long ld_out, int dtype, void* stream);

/* d(x) of nn.MaxPool2d(2, stride, 0): gradient goes to each window's first maximum (torch semantics). */
int drn_maxpool2x2_bwd_nhwc(const void* x, const void* dy, void* dx, int Nb, int H, int W, int C, int stride, int dtype,
                            void* stream);

/* out = a + b (gradient fan-in of a residual block). */
int drn_add(const void* a, const void* b, void* out, long n, int dtype, void* stream);

/* Hand-over from the staged NEXT batch to the buffers the heads read, one launch in front of the pooling kernel:
 * props[M][4] <- rois[M][1:5] (the proposal boxes `label_and_sample_proposals` / `get_pgt` work on,
 * roi_heads_oicr.py:320-421: the reference keeps them in the Instances it carries along) and, when n_words > 0,
 * words_dst[0:n_words] <- words_src (the image-level label block of `get_image_level_gt`, roi_heads_oicr.py:287-318).
 * Replaces two tensor copies of the host framework on the launch stream. */
int drn_stage_heads_inputs(const float* rois, float* props, int M, const int* words_src, int* words_dst, int n_words,
                           void* stream);

/* convert_boxes_to_pooler_format for ONE image (detectron2/modeling/poolers.py:69-96) in one launch: boxes [M][4] (+ objectness
 * logits [M] or NULL) -> rois [M][5] = (batch_index, x0, y0, x1, y1), obj [M] (NULL iff logits is NULL) and, when props != NULL, a
 * contiguous copy of the boxes for the pseudo-GT mining / box decoding (roi_heads_oicr.py:320-421 reads `proposals` there). */
int drn_stage_rois(const float* boxes, const float* logits, float batch_index, float* rois, float* obj, float* props, int M,
                   void* stream);

/* ---- region pooling -------------------------------------------------------------------------- */

/* ROIPooler.forward single-level path, detectron2/modeling/poolers.py:191-226:
 * mode 0 = torchvision RoIPool (poolers.py:162-165),
 * mode 1 = ROIAlign (detectron2/layers/csrc/ROIAlign/ROIAlign.h:54-128 roi_align_forward),
 * fused with `box_features * (objectness_logits + 1)` (roi_heads_oicr.py:342-343) when objectness != NULL.
 * feat NHWC; rois [M][5] = (batch_idx, x0, y0, x1, y1); out [M][ld_out] with column
 * c*P*P + ph*P + pw (the NCHW flatten order of box_head.py:85-86); argmax [M][C*P*P] or NULL.
 * out_t (optional, same dtype as out): the transposed copy [C*P*P][ld_out_t] (column = roi) that the fc6 dW GEMM
 * consumes as its K-major operand; written by the same launch when the feature map fits in LDS. */
int drn_roi_pool_nhwc(const void* feat, const float* rois, const float* objectness, void* out, void* out_t,
                      int32_t* argmax, int N, int H, int W, int C, int P, int M, float spatial_scale, long ld_out,
                      long ld_out_t, int mode, int sampling_ratio, int aligned, int in_dtype, int out_dtype,
                      void* stream);

/* drn_roi_pool_nhwc with a hint for out_t: only the rows of channels >= t_first_channel (row index c*P*P + bin) are
 * needed - the fc6 weight gradient reads `out` itself through drn_gemm_tn and keeps a transposed copy only for the few
 * trailing columns its tail-balancing launch takes (drn_gemm_nt_main_cols).  The 64-ROI training kernel skips the A^T
 * store loop of the other channel chunks; every other kernel writes all of out_t (a superset). */
int drn_roi_pool_nhwc_t(const void* feat, const float* rois, const float* objectness, void* out, void* out_t,
                        int32_t* argmax, int N, int H, int W, int C, int P, int M, float spatial_scale, long ld_out,
                        long ld_out_t, int mode, int sampling_ratio, int aligned, int in_dtype, int out_dtype,
                        int t_first_channel, void* stream);

/* drn_roi_pool_nhwc_t with a caller-owned scratch buffer (round 5).  Feature maps whose 8-channel slice leaves one chunk per
 * workgroup (43x58 cells and more: test-time scales, real-size training images; poolers.py:191-226 at those sizes) are first
 * copied chunk-major - [N][C/8][H*W] cells of 16 bytes - into `workspace`, so that the pooling kernel stages contiguous runs
 * instead of 16 bytes of every pixel's line (50x76 / R = 2000: 156 -> ~130 us).  Round 6: large maps with enough ROIs (the rule
 * is DRN_TUNE_ROI_ST's) are pooled from a SPARSE TABLE of block maxima built in LDS out of that copy - four table cells per bin
 * instead of every cell of its window (the stride-8 dilated-C5 map of an 800x1216 image, R = 2000: 929 -> 314 us; 1200x1600:
 * 4433 -> 677 us); the workspace then also holds a 256-byte record and a class byte per ROI.  drn_roi_pool_workspace_bytes
 * returns the size that helps for a shape (0: no workspace is used); workspace NULL or smaller: exactly drn_roi_pool_nhwc_t.
 * The workspace is read and written on `stream` only and holds nothing between calls; results are bit-identical with and
 * without it. */
long drn_roi_pool_workspace_bytes(int N, int H, int W, int C, int P, int M, int mode, int has_argmax, int in_dtype,
                                  int out_dtype);
int drn_roi_pool_nhwc_ws(const void* feat, const float* rois, const float* objectness, void* out, void* out_t,
                         int32_t* argmax, int N, int H, int W, int C, int P, int M, float spatial_scale, long ld_out,
                         long ld_out_t, int mode, int sampling_ratio, int aligned, int in_dtype, int out_dtype,
                         int t_first_channel, void* workspace, long workspace_bytes, void* stream);


/* Backward of the above w.r.t. the feature map: torchvision RoIPool's backward (scatter to the arg-max the forward
 * returned) and roi_align_backward (detectron2/layers/csrc/ROIAlign/ROIAlign.h:93-128, ROIAlign_cuda.cu:141-250),
 * with the forward's objectness scaling applied to grad_out.  grad_out [M][ld_g] (column c*P*P + bin, fp32 or bf16);
 * dfeat [N][H][W][C] fp32 is zeroed and accumulated with fp32 atomics like the reference's CUDA kernels. */
int drn_roi_pool_backward_nhwc(const void* grad_out, const float* rois, const float* objectness, const int32_t* argmax,
                               float* dfeat, int N, int H, int W, int C, int P, int M, float spatial_scale, long ld_g,
                               int mode, int sampling_ratio, int aligned, int grad_dtype, void* stream);

/* The same backward with a FIXED accumulation order and no float atomics (bit-reproducible training; the package's
 * deterministic mode).  Definition: dfeat[b][y][x][c] is the fp32 result of starting at +0.0f and adding the contributions
 * that land on that element one at a time in ascending order of (ROI index m, bin = ph*P + pw) - for ROIAlign the order
 * continues with iy, ix and the taps (y_low,x_low), (y_low,x_high), (y_high,x_low), (y_high,x_high).  A contribution is
 * fl32(g[m][c*P*P + bin] * (objectness[m] + 1)) for RoIPool when the arg-max is >= 0 (no product without objectness) and that
 * value * (hy*hx) / count per tap for ROIAlign, rounded to fp32 BEFORE it is added (no contraction).  ROIs of different
 * images may interleave; the order is by m.  An element no contribution reaches is +0.0f; every element of dfeat is stored
 * exactly once (no memset).  RoIPool: bit-equal to a sequential scatter over m, c, bin on the host.
 * Two launches: a tile-list pass (one wave per image x pixel tile compacts, by ballot, the ascending list of ROIs that can
 * reach the tile) and an accumulate pass (one wave per tile x 64 channels owns its accumulators in LDS and stores them).
 * Class: grad_out fp32 or bf16, any C (ragged last 64-channel chunk), any H, W <= 16384 (ragged edge tiles), P*P <= 64,
 * M >= 0 (M == 0 stores zeros; grad_out / rois / argmax may then be NULL); mode 0 expects the arg-max drn_roi_pool_nhwc
 * returned for the same rois and scale (an arg-max outside its bin's window, or outside the map, is dropped); a ROI whose
 * batch index is outside [0, N) is dropped.  DRN_ERR_ARG for a NULL, misaligned (8 bytes) or too small workspace.
 * Workspace: drn_roi_backward_det_ws_bytes(N, H, W, M) = 8 * (M + 1) * N * ceil(H / 4) * ceil(W / 4) bytes - per 4 x 4 pixel
 * tile of every image one count and up to M entries of 8 bytes (ROI index, bin-row mask | bin-column mask << 8); the kernels
 * use 8 x 8 tiles (a quarter of the records) when that still fills the device.  Host-only, needs no device; 0 for invalid sizes.
 * The workspace is written and read on `stream` only and holds nothing between calls. */
long drn_roi_backward_det_ws_bytes(int N, int H, int W, int M);
int drn_roi_pool_backward_det_nhwc(const void* grad_out, const float* rois, const float* objectness, const int32_t* argmax,
                                   float* dfeat, int N, int H, int W, int C, int P, int M, float spatial_scale, long ld_g,
                                   int mode, int sampling_ratio, int aligned, int grad_dtype, void* workspace,
                                   long workspace_bytes, void* stream);

/* out[c][r] = cast(in[r][c]) — builds the K-major operands of the dW GEMMs. */
int drn_transpose2d(const void* in, void* out, int rows, int cols, long ld_in, long ld_out, int in_dtype,
                    int out_dtype, void* stream);

/* out[r][c] = cast(in[r][c]) with independent leading dimensions (padded compute shadows of weights). */
int drn_cast2d(const void* in, void* out, int rows, int cols, long ld_in, long ld_out, int in_dtype, int out_dtype,
               void* stream);

/* ---- dense contractions ---------------------------------------------------------------------- */

/* Which output columns drn_gemm_nt's persistent 256x256 launch keeps for an [M, N] output: [0, n0); the columns from n0 on
 * are peeled into a small-tile launch first (tail balancing, DRN_TUNE_GEMM_TAIL_SPLIT).  n0 == N when nothing is peeled.
 * Lets a caller that issues several row slabs of one product (the fc6 weight gradient: F.linear's dW, box_head.py:82-91)
 * compute ALL slabs' peeled columns in one launch and hand the slabs' main columns - exact rounds - to drn_gemm_nt. */
long drn_gemm_nt_main_cols(int M, int N, int splits);

/* nn.Linear / F.linear and its autograd (fc6/fc7 of box_head.py:82-91, predictors of
 * fast_rcnn.py:453-461,1316-1327).  C[s][M][N] (fp32) = A[M][K] * B[N][K]^T over K-split s.
 * K*esize must be a multiple of 128 bytes (callers zero-pad K), lda/ldb multiples of 16 bytes.
 * c_dtype: DRN_F32, or DRN_BF16 (splits == 1, no accumulate) for weight-gradient buckets that are exchanged
 * between GPUs in bf16. */
int drn_gemm_nt(const void* A, const void* B, void* C, int M, int N, int K, long lda, long ldb, long ldc, int dtype,
                int c_dtype, int splits, long c_split_stride, int accumulate, void* stream);

/* drn_gemm_nt_pair: two independent drn_gemm_nt problems (bf16 operands, fp32 outputs; splits / accumulate per problem
 * as there) in ONE persistent launch of the 256x256 kernel - the workgroups of every XCD are divided between the two
 * problems in proportion to their work.  Serves pairs of launches that each leave CUs idle: the fc7 weight gradient and
 * the fc7 input gradient of the explicit backward (torch.autograd of box_head.py:82-91's fc2: dW = dY^T X, dX = dY W,
 * both from dY).  Bit-identical to the two separate calls. */
int drn_gemm_nt_pair(const void* A0, const void* B0, void* C0, int M0, int N0, int K0, long lda0, long ldb0, long ldc0,
                     int splits0, long stride0, int accumulate0, const void* A1, const void* B1, void* C1, int M1, int N1,
                     int K1, long lda1, long ldb1, long ldc1, int splits1, long stride1, int accumulate1, void* stream);

/* drn_gemm_tn: C[M,N] = A[M,K] . Bt[K,N] with the second operand given K-MAJOR (Bt row-major [kb_rows][ldb]; rows
 * kb_rows..K-1 - the K padding - are read as zeros and need not exist).  bf16 operands, fp32 accumulate, C fp32
 * (splits / accumulate as drn_gemm_nt) or bf16.  The fc6 weight gradient dW = dP1^T . A (the autograd of
 * box_head.py:82-91's fc1) reads the pooled matrix A [R][C*49] through it directly, so the pooling launch no longer
 * writes a transposed copy A^T.  256x256 ping-pong kernel with transposing LDS reads (ds_read_b64_tr_b16); results are
 * bit-identical to drn_gemm_nt on a materialised transpose.  K % 64 == 0, (ldb * 2) % 16 == 0, ldb >= N. */
int drn_gemm_tn(const void* A, const void* Bt, void* C, int M, int N, int K, int kb_rows, long lda, long ldb, long ldc,
                int c_dtype, int splits, long c_split_stride, int accumulate, void* stream);

/* The same pair of reference operations (dW = dY^T X of box_head.py:82-91's fc1 through torch.autograd, then
 * torch.optim.SGD.step on it: detectron2/solver/build.py:93-137, projects/WSL/tools/train_net.py:104-113) in the TN operand
 * form of drn_gemm_tn and with the gradient rounded to bf16 exactly as the unfused pair does (drn_gemm_tn into a bf16 bucket,
 * then drn_sgd_step / drn_sgd_step_block reading it): G = A[M][K] . Bt[K][N] is written to grad_bucket (bf16, [M][ldc]) and
 *   d = G*grad_scale + wd*W;  buf = first_step ? d : momentum*buf + d;  W -= lr*buf;  shadow = bf16(W)
 * is applied by the SAME launch: every workgroup of the persistent 256x256 kernel updates the tile it finished last while it
 * multiplies the next one (one 8-row chunk per K slab, loads / stores interleaved with the LDS-DMA pipeline), so the
 * optimizer's HBM traffic is a steady stream under the MFMA work and the gradient is read back from L2.  Bit-identical to
 * the unfused pair.  Shape class: K >= 128 with K % 64 == 0 (with fewer than 32 K slabs - fewer than 1985 proposals - the
 * chunks of a tile's update that find no slab follow the mainloop, exposed), M, N multiples of 256, a bf16 shadow, 16-byte
 * aligned pointers and pitches, more tiles than compute units; DRN_ERR_UNSUPPORTED for everything outside it (callers then run
 * the unfused pair), DRN_ERR_ARG only for null / negative arguments. */
int drn_gemm_tn_sgd(const void* A, const void* Bt, void* grad_bucket, int M, int N, int K, int kb_rows, long lda, long ldb,
                    long ldc, float* weights, float* momentum_buf, void* shadow, long ld_w, const void* seg_dev,
                    float momentum, int first_step, float grad_scale, void* stream);

/* drn_gemm_tn_acc_sgd: the closing micro-step of a gradient-accumulation window for the fc6 weight, as one launch.  The reference
 * accumulates WSL.ITER_SIZE micro-iterations before every optimizer step (projects/WSL/tools/train_net.py:100-113: each one
 * back-propagates loss / ITER_SIZE, optimizer.step() and zero_grad() run when iter % ITER_SIZE == 0); for box_head.py:82-91's fc1
 * the gradient of the window is the sum of its micro-steps' dW = dY^T X.  This entry is drn_gemm_tn_sgd with one more operand,
 * grad_acc (fp32, [M][ld_acc]) - the sum of the window's earlier micro-steps, as drn_gemm_tn (fp32 C, accumulate) leaves it:
 *   G = bf16(grad_acc + A[M][K] . Bt[K][N])
 * formed in fp32 and rounded to bf16 ONCE (the single rounding point the bf16 gradient bucket has without accumulation), written
 * to grad_bucket, and the update of drn_gemm_tn_sgd applied with it by the same launch.  Bit-identical to drn_gemm_tn (fp32,
 * accumulate = 1) on grad_acc, drn_cast2d to bf16, drn_sgd_step.  grad_acc is read, never written; what it holds afterwards is
 * unspecified to callers (the next window's first micro-step overwrites it).  Shape class and error codes of drn_gemm_tn_sgd,
 * plus ld_acc % 4 == 0, a 16-byte aligned grad_acc and M * ld_acc * 4 inside the 32-bit offset range (DRN_ERR_UNSUPPORTED
 * otherwise); grad_acc == NULL or ld_acc < N is DRN_ERR_ARG. */
int drn_gemm_tn_acc_sgd(const void* A, const void* Bt, const float* grad_acc, void* grad_bucket, int M, int N, int K, int kb_rows,
                        long lda, long ldb, long ld_acc, long ldc, float* weights, float* momentum_buf, void* shadow, long ld_w,
                        const void* seg_dev, float momentum, int first_step, float grad_scale, void* stream);

/* tuning / test hook: pin the GEMM tile to 64, 128 or 256 (0 = heuristic); returns the previous setting. */
int drn_gemm_set_tile(int tile);

/* tuning knobs for A/B measurements and tests (defaults = the measured best); returns the previous value, -1 for an
 * unknown knob.  A value a knob does not take is ignored (the setting stays, and is what drn_tune returns).  The knobs, by id
 * (the library keeps them in one table: csrc/tune.h holds the state and the defaults, drn_tune in csrc/tune.hip the rule
 * of every knob): */
#define DRN_TUNE_GEMM_PERSISTENT 1 /* 0/1 - 256x256 GEMM launches with more (tile, K-split) work items than CUs run as ONE resident workgroup per CU that loops over its share (default 1; same arithmetic, bit-identical results) */
#define DRN_TUNE_SGD_GRID 2 /* workgroups (x) of the optimizer kernel (8..65535, default 512) */
#define DRN_TUNE_GEMM_GROUP_ROWS 3 /* tile rows per group of the 256x256 GEMM's XCD patch mapping (0..64; 0 = heuristic) */
#define DRN_TUNE_ROI_MAP64 4 /* 64-ROI x 8-channel whole-map ROIPool for the bf16 (A, A^T) pair: 0 = off, else threads per workgroup (256 / 512 / 1024, default 512) */
#define DRN_TUNE_CONV_KSPLIT 5 /* 0/1: 32x32 wave-K-split conv kernel for latency-bound small-map layers (default 1) */
#define DRN_TUNE_GEMM_TAIL_SPLIT 6 /* 0/1: a persistent 256x256 launch whose last round would be < 3/8 full runs an exact number of rounds; the peeled tile columns go to the small-tile kernel first (default 1; bit-identical) */
#define DRN_TUNE_CONV_KS_TILES 7 /* largest number of 64x64 tiles of ONE image's layer that still runs on the wave-K-split conv kernel (0 = default: CUs / 4) */
#define DRN_TUNE_CONV_K2_TILES 8 /* largest number of 64x64 tiles of ONE image's layer that runs two K-groups per tile (conv_nhwc_k2_kernel); -1 = default (2 x CUs), 0 = off */
#define DRN_TUNE_CONV_PATCH 9 /* 0 = never use the LDS-resident-patch kernel for 3x3 / 64 -> 64 channel convs; 1 = default (maps of >= 32768 pixels); > 1 = that many pixels per image at least; drn_tune returns the pixel threshold while the kernel is on, 0 while it is off */
#define DRN_TUNE_ROI_CPB 10 /* 64-ROI ROIPool: most 8-channel chunks one workgroup walks (power of two, default 1; halved until two workgroups per CU remain): bin bounds / item table once per workgroup - faster stand-alone (4-8), slower inside the training step */
#define DRN_TUNE_ROI_PREFETCH 11 /* 0/1 (default 1): 64-ROI ROIPool keeps two map-slice buffers and fetches the next chunk's slice under the scan */
#define DRN_TUNE_GEMM_PINGPONG 12 /* 0/1 (default 1): bf16 256x256 GEMMs run the ping-pong mainloop - the two waves of a SIMD half a phase apart, four [reads + DMA | 8 MFMAs] phases per K slab, half-tile LDS-DMA spread over the slab; bit-identical to the lock-step pipeline it replaces (0) */
#define DRN_TUNE_FP8_K64 13 /* 0/1 (default 1): fp8 convolutions multiply with v_mfma_scale_f32_32x32x64_f8f6f4 (unit scales; the fp8 MFMA rate) instead of the K = 16 non-scaled form (bf16 rate); same exact products, another fp32 summation order */
#define DRN_TUNE_ROI_MAP64_A 14 /* 0/1 (default 0): the 64-ROI ROIPool kernel also when only A is asked for (no A^T) */
#define DRN_TUNE_ROI_LDS_KB 15 /* 60..154 (default 154): LDS a 64-ROI pooling block may take for map slice + tile; 76 stages larger maps in row bands so that two blocks share a CU */
#define DRN_TUNE_GEMM_NWG 18 /* resident workgroups of persistent 256x256 launches (multiple of 8; 0 = default: one per CU) - for launches on a CU-masked stream */
#define DRN_TUNE_ROI_LANE 19 /* 0/1 (default 1): the bf16 training operand A from the lane-per-bin ROIPool kernel (a wave per ROI, lane = bin: every channel leaves as one 98-byte run per store instruction); 0 = the 64-ROI kernel writes A; 2 = the lane kernel but never its walking form; 3 (tests) = 1 with one sub-group of 64 ROIs per block of the walking form instead of two - drn_tune then reports 1, and any other value brings the two sub-groups back */
#define DRN_TUNE_SGDP_EPILOGUE 20 /* 0/1 (default 1): the tile epilogue of drn_gemm_tn_sgd moves the bf16 gradient tile LDS -> global four 16-byte pieces per trip instead of one (A/B knob; bit-identical) */
#define DRN_TUNE_ROI_LANE_REPS 22 /* lane-per-bin ROIPool on maps that leave one block per CU: groups of 64 ROIs a block walks with one staged map slice (0 = default: 4, halved while fewer than two rounds of blocks would remain; 1 = a block per group) */
#define DRN_TUNE_CONV_RING 23 /* register-ring conv kernels (conv_ring.hip; bf16, Cin % 64 == 0, layers beyond the latency-bound small maps): 0 = off (the tiles of conv.hip), 1 = default (64x64 tile, class by measurement), 64 / 128 = pin the 64x64 / 128x128 tile (any other value is ignored: drn_tune returns the unchanged setting); every tile gives the same bits as the 64x64 / 128x128 tiled kernel */
#define DRN_TUNE_CONV_PP 24 /* 1x1 / stride-1 bf16 convs of large maps on the 256x256 ping-pong GEMM mainloop with the conv epilogue (conv1x1_pp_kernel): 0 = off, 1 = default (Cout >= 256 and >= 192 tiles of 256x256 per image, or >= 100 tiles with K >= 1024), n > 1 = at least n tiles, any Cout; same bits as the tiled kernels */
#define DRN_TUNE_PP8 25 /* eight-wave ping-pong kernel (pp8.hip: 128x128 or 256x128 tile, two waves per SIMD half a phase apart; bf16 convs with Cin % 64 == 0 and drn_linear_act_fwd): 0 = off, 1 = default class (measured per layer shape, see conv_fwd_plan), 2 = every layer in the kernel's class; same bits as the tiled kernels */
#define DRN_TUNE_PP8_STAGES 26 /* 3 / 4 / 5 (default 5): 32-KB LDS stages of the 128x128 form's ring = 1 / 2 / 3 K slabs in flight (A/B knob; bit-identical) */
#define DRN_TUNE_PP8_VARIANT 27 /* schedule variant of that kernel (A/B knob; bit-identical): 0 = a slab's four DMA pieces in the fragment-read phase, 1 (default) = two there and two between the MFMAs, 2 = all between the MFMAs, + 4 = no s_setprio around the MFMAs, + 8 = profile build (shader-clock split of the mainloop) */
#define DRN_TUNE_PP8_PROFILE 28 /* any value: print (stderr) and clear the per-phase shader-clock sums the profile builds (DRN_TUNE_PP8_VARIANT + 8) accumulated for workgroup 0; returns 0 */
#define DRN_TUNE_PP8_WIDE 29 /* the 256x128 form of that kernel (wave tile 64x64, three 48-KB stages): 0 = never, 1 = default (layers that give it >= 5/8 of the CUs' worth of tiles per image), 2 = always */
#define DRN_TUNE_PP8_WIDE_VARIANT 30 /* schedule variant of the 256x128 form (A/B knob; bit-identical): bit 0 = all six DMA pieces of a slab in the second fragment-read phase (else three there, three between the MFMAs), 4 = no s_setprio, 8 = profile build; default 4 */
#define DRN_TUNE_ROI_ST 31 /* RoIPool from a sparse table of block maxima (four table cells per bin instead of the window's cells; needs the workspace of drn_roi_pool_workspace_bytes): 0 = off, 1 (default) = where it beats the window kernels (maps of >= 1800 cells with >= 1500 ROIs, >= 3000 cells with >= 600 ROIs, and every map whose LDS slice holds only 4 channels per cell - the dilated-C5 stride-8 map of a real-size image - with >= 400 ROIs), 2 = every map whose slice fits (>= 64 ROIs); 10 / 11 = its profile builds on / off and 12 = print (stderr) and clear their counters - all three leave the setting */
#define DRN_TUNE_MSM_WAVE 32 /* 0/1 (default 1): drn_mean_softmax for heads of <= 64 columns as a wave per row / lane per class (one coalesced load per head, the denominator summed in class order: bit-identical); 0 = the thread-per-row kernel */
int drn_tune(int knob, int value);

/* relu_(fc(x)) + F.dropout(p) of DiscriminativeAdaptionNeck.forward (projects/WSL/wsl/modeling/roi_heads/box_head.py:82-91)
 * as ONE launch for bf16 operands: out [M][ld_out] (bf16) = dropout(relu(A [M][lda] . W [N][ldw]^T + bias)), and optionally
 * its transpose outT [N][ld_outT] (rows m >= M of outT are left untouched).  Same dropout rule as drn_bias_act_fwd (explicit
 * mask [M][N], else counter-based from seed (+ *seed_dev) when drop_p > 0; this entry never advances the counter); the
 * product is accumulated over K in one fp32 chain per element (= drn_gemm_nt with splits == 1 followed by
 * drn_bias_act_fwd, bit for bit).  K % 64 == 0, N % 8 == 0, 16-byte aligned rows; DRN_ERR_UNSUPPORTED outside that class
 * (the caller then runs the two-launch form). */
int drn_linear_act_fwd(const void* A, const void* W, const float* bias, const float* mask, unsigned long long seed,
                       const unsigned long long* seed_dev, float drop_p, void* out, long ld_out, void* outT, long ld_outT,
                       int M, int N, int K, long lda, long ldw, int relu, void* stream);

/* relu_(fc(x)) + F.dropout(p), box_head.py:88-90: sums split-K partials, adds bias, ReLU, dropout
 * (explicit multiplier mask [M][N] if given, else counter-based mask from seed (+ *seed_dev) when drop_p > 0; a launch
 * WITHOUT dropout (drop_p == 0, no mask) that is given seed_dev advances that counter: *seed_dev += seed - the heads'
 * logits pass does this behind the two dropout layers, so a replayed hipGraph draws fresh masks without a launch of its own);
 * writes out [M][ld_out] and/or its transpose outT [N][ld_outT]. */
int drn_bias_act_fwd(const float* partials, int splits, long split_stride, const float* bias, const float* mask,
                     unsigned long long seed, const unsigned long long* seed_dev, float drop_p, void* out, long ld_out,
                     void* outT, long ld_outT, int M, int N, long ld_in, int relu, int out_dtype, void* stream);

/* *counter += inc on the stream (the dropout seed lives on the device so a replayed hipGraph draws fresh masks). */
int drn_counter_add(unsigned long long* counter, unsigned long long inc, void* stream);

/* autograd of the above: dpre = grad_out * dropout_mult * (saved_out > 0); colsum[n] = sum_m dpre (bias
 * gradient, fixed summation order); saved_out == NULL means "no activation"; colscale [N] (optional)
 * multiplies grad_out per column (per-loss upstream gradients stay on the device): column n uses
 * colscale[colidx ? colidx[n] : n] (index -1 = 0); colpart = scratch of
 * ceil(M/64)*N floats for the two-stage (deterministic) column sums, required with colsum. */
int drn_bias_act_bwd(const void* grad_out, int grad_dtype, long ld_in, const float* colscale, const int* colidx,
                     const void* saved_out, const float* mask, float drop_p,
                     void* dpre, long ld_out, void* dpreT, long ld_outT, float* colsum, float* colpart,
                     int accumulate_colsum, int M, int N, int out_dtype, void* stream);

/* drn_bias_act_bwd with grad_out given as `splits` fp32 split-K partials, `split_stride` floats apart, summed on load in
 * order (the dX GEMM in front of it can then use a K-split like the forward GEMMs). */
int drn_bias_act_bwd_splits(const void* grad_out, int grad_dtype, long ld_in, int splits, long split_stride,
                            const float* colscale, const int* colidx, const void* saved_out, const float* mask,
                            float drop_p, void* dpre, long ld_out, void* dpreT, long ld_outT, float* colsum,
                            float* colpart, int accumulate_colsum, int M, int N, int out_dtype, void* stream);

/* drn_gemm_nt (fp32 out, one split) + drn_bias_act_bwd in ONE launch for a skinny contraction - the predictor's dX
 * feeding fc7's activation backward (box_head.py:82-91 autograd behind fast_rcnn.py:493-527): dpre = act'(saved_out) .*
 * (A [M][lda] . B [N][ldb]^T), its transposed copy and the bias-gradient column sums, bit for bit what the two calls
 * produce; the fp32 [M][N] product never goes to memory.  bf16 operands and outputs, K in {64, 128, 192, 256},
 * N % 64 == 0, 16-byte aligned rows; DRN_ERR_UNSUPPORTED otherwise (callers then run the two calls). */
int drn_gemm_nt_act_bwd(const void* A, const void* B, int M, int N, int K, long lda, long ldb, const void* saved_out,
                        const float* mask, float drop_p, void* dpre, long ld_out, void* dpreT, long ld_outT, float* colsum,
                        float* colpart, int accumulate_colsum, void* stream);

/* Second stage of drn_bias_act_bwd's column sums (bias gradients) on its own: with colsum == NULL and colpart != NULL
 * drn_bias_act_bwd only leaves the ceil(M/64) x N per-block partials; this adds them in a fixed order into colsum
 * (accumulate != 0: += ).  Lets the optimizer stream finish the bias gradients right in front of the SGD pass. */
int drn_colsum_reduce(const float* colpart, int nparts, int N, float* colsum, int accumulate, void* stream);

/* ---- MIL / OICR head ------------------------------------------------------------------------- */

/* WSDDNOutputLayers.forward (fast_rcnn.py:493-527) + predict_probs_img (:689-700) +
 * WSDDNOutputs.binary_cross_entropy_loss (:317-329) + their autograd.  logits [M][ld] fp32 with the
 * cls / det heads at columns c_cls / c_det; img_off [n_img+1] row offsets.  loss = sum(loss_part).
 * scratch: n_img * ceil(max_rows/32) * 384 floats, max_rows = largest per-image proposal count.  max_rows must be at
 * least the row count of every image: the grid has ceil(max_rows/32) blocks per image and rows beyond it are not
 * processed (a larger value only adds idle blocks and scratch).  K <= 128; K, n_img and max_rows >= 1, anything else is
 * refused before a launch.  dlogits (optional): only columns c_cls..+K and c_det..+K of rows < img_off[n_img] are written.
 * An image without proposals (img_off[i] == img_off[i+1]) is defined as predict_probs_img defines it on an empty split:
 * img_scores[i][:] = 1e-6 (the clamped zero sum), loss_part[i] = the BCE of that row, and no gradient (it has no rows). */
int drn_wsddn_fwd_bwd(const float* logits, long ld, int c_cls, int c_det, int K, const int* img_off, int n_img,
                      const float* gt_onehot, float* scores, float* row_softmax, float* img_scores, float* loss_part,
                      float* dlogits, long ld_d, float* scratch, int max_rows, int mean_loss, float loss_scale,
                      void* stream);

/* OICRROIHeads.get_pgt (roi_heads_oicr.py:491-567) + ROIHeads.label_and_sample_proposals
 * (roi_heads.py:255-353; pairwise_iou structures/boxes.py:329-361; Matcher modeling/matcher.py:61-103).
 * prev_boxes [M][box_cols] with box_cols = 4 (Boxes path) or 4K (class-specific decoded boxes);
 * zero_delta_decode = 1 applies apply_deltas(0, .) to the selected box (what a non-regressing head passes on).
 * gt_classes [n_img][gmax] (unique per image, any order; 1 <= gmax <= 128), of which the first gt_count[i] are used;
 * pgt_idx / pgt_boxes slots from gt_count[i] on are not written.  1 <= nthr <= 3; anything else is refused.
 * An image without ground truth (gt_count[i] == 0): labels K, weights 0, matched 0, gt_boxes 0 - the has_gt == False
 * branch of label_and_sample_proposals, whatever thr_labels[0] is.  An image without proposals
 * (img_off[i] == img_off[i+1]): no row is read or written; its first gt_count[i] slots are pgt_idx 0, pgt_boxes 0. */
int drn_oicr_targets(const float* prev_scores, long ld_s, const float* prev_boxes, int box_cols, int zero_delta_decode,
                     const float* props,
                     const int* img_off, int n_img, const int* gt_classes, const int* gt_count, int gmax,
                     const float* img_scores, int K, const float* thresholds_host, const int* thr_labels_host,
                     int nthr, int* labels, float* weights, int* matched, float* gt_boxes, int* pgt_idx,
                     float* pgt_boxes, void* stream);

/* The whole refinement cascade of OICRROIHeads._forward_box (roi_heads_oicr.py:372-395: for each branch k,
 * get_pgt on the previous branch's scores -> label_and_sample_proposals -> OICROutputs.losses) for n_heads
 * NON-regressing branches in four launches: = drn_softmax_ce(probs only) / drn_oicr_targets / drn_softmax_ce per head,
 * bit for bit.  scores0 [M][ld_s0] = the WSDDN scores feeding branch 0.  Per-head outputs are [n_heads] x the
 * single-head arrays, contiguous; scratch: n_heads * 2*ceil(M/16) floats; col0s_host: host array [n_heads]. */
int drn_oicr_refine_chain(const float* logits, long ld, const int* col0s_host, int n_heads, int K, const float* scores0,
                          long ld_s0, const float* props, const int* img_off, int n_img, const int* gt_classes,
                          const int* gt_count, int gmax, const float* img_scores, const float* thresholds,
                          const int* thr_labels, int nthr, float* probs, int* labels, float* weights, int* matched,
                          float* gt_boxes, int* pgt_idx, float* pgt_boxes, float* dlogits, long ld_d, float* losses,
                          float* scratch, int M, float loss_scale, void* stream);

/* The loss tail of one training step of OICRROIHeads._forward_box with non-regressing refinement branches
 * (roi_heads_oicr.py:351-395: predictor bias -> WSDDNOutputs.losses -> the refinement cascade) in SIX launches:
 * = drn_bias_act_fwd (fp32 logits from the predictor GEMM's split-K partials [splits][M][ld_part] + bias) +
 * drn_wsddn_fwd_bwd + drn_oicr_refine_chain (nine), bit for bit: WSDDN stage 0 and the heads' softmax read their logits
 * from the partials.  logits [M][ld] is an OUTPUT: columns c_cls..+K, c_det..+K and col0s_host[k]..+K+1 are written.
 * seed_dev (optional): the device-side dropout counter this pass advances by seed_inc (what the fp32 drn_bias_act_fwd
 * call without dropout does).  ws_scratch as drn_wsddn_fwd_bwd, ce_scratch as drn_oicr_refine_chain.  The WSDDN scores
 * feed branch 0. */
int drn_mil_oicr_losses(const float* partials, int splits, long split_stride, long ld_part, const float* bias,
                        unsigned long long seed_inc, unsigned long long* seed_dev, float* logits, long ld, int c_cls,
                        int c_det, int K, const int* img_off, int n_img, const float* gt_onehot, float* scores,
                        float* row_softmax, float* img_scores, float* loss_part, float* ws_scratch, int max_rows,
                        int mean_loss, const int* col0s_host, int n_heads, const float* props, const int* gt_classes,
                        const int* gt_count, int gmax, const float* thresholds, const int* thr_labels, int nthr, float* probs,
                        int* labels, float* weights, int* matched, float* gt_boxes, int* pgt_idx, float* pgt_boxes,
                        float* losses, float* ce_scratch, float* dlogits, long ld_d, int M, float loss_scale,
                        void* stream);

/* OICROutputs.softmax_cross_entropy_loss (fast_rcnn.py:1087-1096,1128-1144), predict_probs (:1561-1575)
 * and the backward: loss = sum_r w_r CE_r / #{w_r > 1e-12}.  labels == NULL => probabilities only.
 * scratch: 2*ceil(M/16) floats (two-stage deterministic reduction), required with labels. */
int drn_softmax_ce(const float* logits, long ld, int col0, int C, const int* labels, const float* weights,
                   float* probs, float* dlogits, long ld_d, float* loss, float* scratch, int M, float loss_scale,
                   void* stream);

/* OICROutputs.box_reg_loss, fast_rcnn.py:1146-1211 (WSL.REFINE_REG heads) with Box2BoxTransform.get_deltas,
 * detectron2/modeling/box_regression.py:38-71, smooth-L1 beta = 0: loss = sum_fg |pred - target| / M, and its
 * gradient written to dlogits columns col0 .. col0+4K.  scratch: ceil(M/256) floats. */
int drn_box_reg_loss(const float* logits, long ld, int col0, int K, const int* labels, const float* props,
                     const float* gt_boxes, const float* weights4_host, float* dlogits, long ld_d, float* loss,
                     float* scratch, int M, float loss_scale, void* stream);

/* OICROutputLayers.predict_probs_K, fast_rcnn.py:1577-1594.  bg_first = 1: the heads keep the background in their
 * column 0 (PCL) and the output is rotated so that it is the last column (`pcl_bg`, fast_rcnn.py:1463-1465). */
int drn_mean_softmax(const float* logits, long ld, const int* col0s_dev, int n_heads, int C, float* probs, int M,
                     int bg_first, void* stream);

/* Box2BoxTransform.apply_deltas, detectron2/modeling/box_regression.py:73-110 (deltas NULL = zeros). */
int drn_apply_deltas(const float* deltas, long ld_d, const float* boxes, float* out, int M, int K,
                     const float* weights4_host, float scale_clamp, void* stream);

int drn_sum_small(const float* in, int n, float scale, float* out, void* stream);

/* ---- box regression of the PCL heads (reg/pcl_* recipes) ------------------------------------------
 * PCLROIHeads labels its proposals against the ANNOTATED boxes (roi_heads_pcl.py:233-235 -> roi_heads.py:214-353: pairwise_iou,
 * Matcher, no sampling) and never relabels them against pseudo ground truth, so a regressing PCL branch (WSL.REFINE_REG[k])
 * regresses onto the matched annotated box (PCLOutputs.box_reg_loss, fast_rcnn.py:1746-1811): restated as it is.
 *
 * drn_annot_box_reg: labelling, target, loss and gradient of n_heads (1 .. DRN_BOXREG_MAX_HEADS) regressing branches and n_img
 * images in one launch pair.  logits = fp32 [M, ld]; col0s_host = HOST array of the branches' first delta column (their 4K deltas
 * are columns col0 .. col0 + 4K, class c in TRUE class indexing at 4c .. 4c + 3); proposals, img_off, gt_boxes, gt_classes,
 * gt_count, max_gt, thresholds, match_labels, nthr, K, max_rows: exactly drn_label_proposals' (below), and labels / matched
 * (each optional, int32 [M]) are BIT-EQUAL to what that entry writes for the same inputs - the same device code labels here.
 * weights4_host = Box2BoxTransform's four weights.  Per image i with M_i rows, fg = {r : 0 <= labels[r] < K}:
 *   t_r   = Box2BoxTransform.get_deltas(proposal r, annotated box matched[r] of image i)       (fp32, drn_box_reg_loss' order)
 *   L_i,h = (sum_fg-rows sum_e |logits[r, col0_h + 4 labels[r] + e] - t_r[e]|) / M_i
 * with the row sums, the 256-row tree and the ascending combine of drn_box_reg_loss; an image without rows contributes 0.
 *   loss[h] = L_0,h for one image, else the mean over the images: an fp64 sum in ascending image order, rounded to fp32 once
 *             (drn_pcl_refine_batch's definition)
 *   dlogits[r, col0_h + 4 labels[r] + e] = sign(pred - t) / M_i * (1.f / n_img) * loss_scale on fg rows, 0 in every other of the 4K
 *             columns of every row (dlogits optional; fp32 [M, ld_d]); for n_img == 1 bit-equal to drn_box_reg_loss fed with
 *             labels and the gathered matched boxes.
 * 256 rows of ONE image per workgroup, the image's boxes in LDS, the gradient block stored with the lanes along the columns; the
 * per-workgroup partial sums go to scratch = fp32 [n_heads * n_img * ceil(max_rows / 256)] and are combined in a fixed order.  No
 * atomics, no host sync, capturable.  loss = fp32 [n_heads].
 * Shape class: 0 <= n_img <= DRN_BOXREG_MAX_IMAGES, M >= 0, 1 <= max_gt <= DRN_LABEL_MAX_GT, 1 <= nthr <= 3, 1 <= n_heads <=
 * DRN_BOXREG_MAX_HEADS, 1 <= K <= DRN_BOXREG_MAX_K (n_img, M or max_rows == 0: no launch, nothing is written).
 * Errors: DRN_ERR_UNSUPPORTED (above the class), DRN_ERR_ARG (null / misaligned pointer, sizes, columns outside ld / ld_d, a Matcher
 * label outside {-1, 0, 1}).
 *
 * drn_apply_deltas_mean: OICROutputLayers.predict_boxes_K (fast_rcnn.py:1534-1559) as PCLROIHeads' inference uses it
 * (roi_heads_pcl.py:342-349): the deltas of ALL n_total = WSL.REFINE_NUM branches are averaged - a non-regressing branch
 * contributes zeros (fast_rcnn.py:1377-1386) - and decoded, in true class order (no pcl_bg rotation, :1465).  col0s_host = HOST
 * array of the n_heads (0 .. DRN_BOXREG_MAX_HEADS) REGRESSING branches' first delta columns, ascending.  Per element
 *   d = ((+0.0f + d_k0) + d_k1 + ...) / (float)n_total            (IEEE division)
 * then drn_apply_deltas' decode of d, by the same device function: bit-equal to drn_apply_deltas on that d.  n_heads == 0 is the
 * zero-delta decode (drn_apply_deltas with deltas == NULL).  out = fp32 [M, 4K]. */
#define DRN_BOXREG_MAX_HEADS 8
#define DRN_BOXREG_MAX_IMAGES 16
#define DRN_BOXREG_MAX_K 4096
int drn_annot_box_reg(const float* logits, long ld, const int* col0s_host, int n_heads, int K, const float* proposals,
                      const int* img_off, int n_img, int M, int max_rows, const float* gt_boxes, const int* gt_classes,
                      const int* gt_count, int max_gt, const float* thresholds, const int* match_labels, int nthr,
                      const float* weights4_host, float* dlogits, long ld_d, float loss_scale, float* loss, int* labels,
                      int* matched, float* scratch, void* stream);
int drn_apply_deltas_mean(const float* logits, long ld, const int* col0s_host, int n_heads, int n_total, const float* boxes,
                          float* out, int M, int K, const float* weights4_host, float scale_clamp, void* stream);

/* ---- optimizer ------------------------------------------------------------------------------- */

/* torch.optim.SGD(momentum) with the per-parameter groups of detectron2/solver/build.py:93-137, applied to a
 * flat parameter arena.  segs_dev: array of {int64 offset, int64 count, float lr, float weight_decay}.
 * shadow (optional, bf16, same flat layout) is refreshed in the same pass.  grads: fp32, or bf16 (gradient buckets
 * that were all-reduced in bf16); arena element j reads grads[j - grad_off], so a bucket buffer that only covers
 * one tensor can be passed with that tensor's arena offset. */
int drn_sgd_step(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                 int shadow_dtype, const void* segs_dev, int nseg, float momentum, int first_step, float grad_scale,
                 void* stream);

/* The same update (torch.optim.SGD.step, detectron2/solver/build.py:93-137; projects/WSL/tools/train_net.py:104-113 calls
 * it once per iteration) on a rectangular BLOCK of one 2-D parameter: rows r0 .. r0+rows, columns c0 .. c0+cols of the
 * [count / ld][ld] view of the tensor that seg_dev ({offset, count, lr, wd}, ONE entry) describes.  The fc6 weight
 * gradient is produced in column slabs of exactly one round of the persistent GEMM each, and a slab's update is
 * issued the moment its GEMM is queued - the optimizer pass of step t then trails the weight-gradient GEMM by one round
 * instead of by half of it.  Per-element arithmetic is drn_sgd_step's (bit-identical results); c0, cols, ld, grad_off
 * multiples of 4. */
int drn_sgd_step_block(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                       int shadow_dtype, const void* seg_dev, int r0, int rows, int c0, int cols, long ld, float momentum,
                       int first_step, float grad_scale, void* stream);

/* SOLVER.CLIP_GRADIENTS, detectron2/solver/build.py:19-90 (maybe_add_gradient_clipping): every parameter is clipped ON ITS OWN right
 * before SGD.step, on the gradient as it stands there - here g * grad_scale of one segment of the table.
 *
 * drn_grad_norms: norms[s] = || grads[segment s] * grad_scale ||_p in fp32 (the norm torch.nn.utils.clip_grad_norm_(p, CLIP_VALUE,
 * NORM_TYPE) takes of ONE tensor); norm_type 1, 2, or 0 for inf (a maximum; a NaN entry gives NaN, as torch's does).  grads / grad_dtype /
 * grad_off / segs_dev / nseg as for drn_sgd_step.  Shape class: any segment offset and length (16-byte non-temporal loads when the
 * segment's first gradient is 16-byte aligned, scalar loads otherwise and for the tail); every segment is spread over a fixed grid of
 * 512 workgroups.  No float atomics, fixed order of addition (wave butterfly, LDS tree, one fp32 partial per (segment, workgroup) in
 * `workspace`, second launch in a fixed order): the same input gives the same bits.  No host synchronisation: capturable.
 * workspace: drn_grad_norms_ws_bytes(nseg) = 2048 * nseg bytes (host-only function; 0 for nseg < 1), written, never read by the caller.
 * Errors: DRN_ERR_ARG (null pointer, nseg < 1, dtype, workspace too small), DRN_ERR_UNSUPPORTED (norm_type not 0 / 1 / 2). */
long drn_grad_norms_ws_bytes(int nseg);
int drn_grad_norms(const void* grads, int grad_dtype, long grad_off, const void* segs_dev, int nseg, int norm_type,
                   float grad_scale, float* norms, void* workspace, long workspace_bytes, void* stream);

/* drn_sgd_step / drn_sgd_step_block with the clipped gradient d in place of g * grad_scale (the rest of the update - weight decay,
 * momentum, lr, bf16 shadow - and its op order are unchanged; the same kernels, one more template parameter):
 *   clip_mode 0  d = g * grad_scale                                     (bit-identical to drn_sgd_step / drn_sgd_step_block)
 *   clip_mode 1  d = clamp(g * grad_scale, -clip_value, clip_value)      torch.nn.utils.clip_grad_value_, build.py:38-39
 *   clip_mode 2  d = (g * grad_scale) * min((1.f / (seg_norms[s] + 1e-6f)) * clip_value, 1)   torch.nn.utils.clip_grad_norm_, build.py:35-36
 *                (torch evaluates max_norm / (total_norm + 1e-6) as reciprocal(total_norm + 1e-6) * max_norm - Tensor.__rtruediv__ -
 *                and so does the kernel: the coefficient has torch's bits given the norm)
 * seg_norms (mode 2): device array from drn_grad_norms over the same table (the block form: pointer to the norm of the ONE tensor
 * seg_dev describes); the coefficient is formed on the device, nothing crosses to the host.  A NaN gradient or coefficient stays NaN
 * (torch.clamp's rule).  Shape class: that of the unclipped entry point.  Errors: those of the unclipped entry point, plus
 * DRN_ERR_ARG for clip_mode outside 0 .. 2, mode 2 without seg_norms, or a clip_value that is negative or NaN. */
int drn_sgd_step_clip(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                      int shadow_dtype, const void* segs_dev, int nseg, float momentum, int first_step, float grad_scale,
                      int clip_mode, float clip_value, const float* seg_norms, void* stream);
int drn_sgd_step_block_clip(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                            int shadow_dtype, const void* seg_dev, int r0, int rows, int c0, int cols, long ld, float momentum,
                            int first_step, float grad_scale, int clip_mode, float clip_value, const float* seg_norms,
                            void* stream);

/* ---- the anomaly guard: skip the update on a non-finite loss -----------------------------------------------------------------
 * The reference checks every iteration's summed loss on the host in front of the optimizer (detectron2/engine/train_loop.py:252-258:
 * `losses = sum(loss_dict.values())`, `if not torch.isfinite(losses).all(): raise FloatingPointError(...)`), so its weights and
 * momentum are always those of the last finite iteration.  Here the update runs inside the backward, so the check runs on the device
 * and the update kernels read its verdict.
 *
 * drn_loss_guard: losses = HOST array of n (1 .. 16) device pointers to the step's fp32 loss scalars, copied into the launch's
 * arguments.  One wave forms their fp32 sum in list order and tests isfinite(sum) - NaN, +-inf, inf + -inf and an overflowing sum of
 * finite terms are bad, as in the reference.  state = int32[4] in device memory, set to {0, 0, -1, 0} by the caller before the first call:
 *   state[0]  skip flag, read by the guarded update kernels below       state[1]  calls seen
 *   state[2]  index (0-based) of the first bad call, or -1              state[3]  number of bad calls
 * mode 1 (raise): the flag, once set, stays set.  mode 2 (skip): flag = bad_now || (flag && !window_first) - window_first marks the
 * first micro-step of a WSL.ITER_SIZE window, so a bad micro-step discards its whole window and nothing more.  state is written with
 * ordinary stores by one lane.  No synchronisation, no allocation, capturable (the pointers, mode and window_first are frozen into a
 * captured launch).  Errors: DRN_ERR_ARG (null pointer, n outside 1 .. 16, mode outside 1 .. 2).
 *
 * The guarded updates take one more argument, guard -> state[0] (device memory; NULL is DRN_ERR_ARG), and are otherwise
 * drn_sgd_step_clip / drn_sgd_step_block_clip / drn_gemm_tn_sgd / drn_gemm_tn_acc_sgd - shape classes and errors included:
 *   guard[0] == 0   bit-identical to the unguarded entry point
 *   guard[0] != 0   weights, momentum_buf and shadow keep their bits; the GEMM forms still write grad_bucket
 * The flat and block kernels leave by a wave-uniform early exit.  The fused dW + SGD launch keeps all three loads and three stores of
 * every chunk (its mainloop's counted waits depend on them) and stores back what it loaded: w, momentum, and bf16(w) for the shadow -
 * the shadow must hold bf16(weights) on entry, which is what every update entry point leaves there.
 * A skipped FIRST step (first_step = 1) leaves momentum_buf untouched: callers create it as zeros, and a later first_step = 0 update
 * on zeros computes exactly what a first step would (momentum * 0 + d == d). */
int drn_loss_guard(const void* const* losses, int n, int mode, int window_first, int* state, void* stream);
int drn_sgd_step_guard(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                       int shadow_dtype, const void* segs_dev, int nseg, float momentum, int first_step, float grad_scale,
                       int clip_mode, float clip_value, const float* seg_norms, const int* guard, void* stream);
int drn_sgd_step_block_guard(float* weights, float* momentum_buf, const void* grads, int grad_dtype, long grad_off, void* shadow,
                             int shadow_dtype, const void* seg_dev, int r0, int rows, int c0, int cols, long ld, float momentum,
                             int first_step, float grad_scale, int clip_mode, float clip_value, const float* seg_norms,
                             const int* guard, void* stream);
int drn_gemm_tn_sgd_guard(const void* A, const void* Bt, void* grad_bucket, int M, int N, int K, int kb_rows, long lda, long ldb,
                          long ldc, float* weights, float* momentum_buf, void* shadow, long ld_w, const void* seg_dev,
                          float momentum, int first_step, float grad_scale, const int* guard, void* stream);
int drn_gemm_tn_acc_sgd_guard(const void* A, const void* Bt, const float* grad_acc, void* grad_bucket, int M, int N, int K,
                              int kb_rows, long lda, long ldb, long ld_acc, long ldc, float* weights, float* momentum_buf,
                              void* shadow, long ld_w, const void* seg_dev, float momentum, int first_step, float grad_scale,
                              const int* guard, void* stream);

/* ---- per-step metrics from a device-side ring ---------------------------------------------------------------------------------
 * The reference floats every logged scalar on the host each iteration: the losses and their sum (detectron2/engine/train_loop.py:260-289,
 * _write_metrics), per refinement branch fast_rcnn/cls_accuracy_r{k}, fg_cls_accuracy_r{k}, false_negative_r{k}
 * (projects/WSL/wsl/modeling/roi_heads/fast_rcnn.py:1098-1126, _log_accuracy) and roi_head/num_{fg,bg,ig}_samples_r{k}
 * (roi_heads.py:338-349, roi_heads_oicr.py:366-374).  Here the device writes ONE record per step into a ring and the host copies the
 * ring every N steps; nothing on the step waits for it.  Two launches, both capturable, no argument that changes from step to step.
 *
 * drn_head_metrics: label statistics of nh refinement branches in one launch.  logits = the heads' fp32 logits [rows >= M, ldl]
 * (4-byte aligned; 16-byte loads are used wherever a row's columns allow); col0s = HOST array of nh first-column indices, labels = HOST
 * array of nh device pointers to int32 labels[M] (-1 ignore, K background) - both copied into the launch's arguments.  For row r of
 * branch k: p = the FIRST maximal index of logits[r, col0_k .. col0_k + K] (torch.argmax's tie rule; +0 and -0 tie), g = labels_k[r].
 * counts = int32[nh][DRN_METRICS_COUNT_STRIDE] in device memory, ZERO on entry; the kernel adds, as exact integers,
 *   [0] n_ig = #{g == -1}   [1] n_bg = #{g == K}   [2] n_fg = #{0 <= g < K}
 *   [3] n_acc = #{p == g}   [4] n_fg_acc = #{0 <= g < K, p == g}   [5] n_fneg = #{0 <= g < K, p == K}      ([6], [7] stay zero)
 * with one atomicAdd(int*) per non-zero counter and workgroup: the result does not depend on arrival order.  A workgroup of sixteen
 * waves owns DRN_METRICS_ROWS_PER_BLOCK consecutive rows of one branch; a row is read by L lanes of one wave, L = the smallest power of two
 * >= max(2, (K + 7) / 4) and <= 64, so a wave holds 64 / L rows at a time.  No column outside the branches' K + 1 columns and no row
 * >= M is read.  NaN logits: unspecified (the anomaly guard is the tool for such runs).
 * Shape class: 0 <= nh <= 8, 1 <= K, K + 1 <= 1024, col0_k + K + 1 <= ldl, any M >= 0 (nh == 0 or M == 0: nothing is launched).
 * Errors: DRN_ERR_UNSUPPORTED (nh > 8, K + 1 > 1024), DRN_ERR_ARG (null pointer, negative size, columns outside ldl).
 *
 * drn_metrics_record: one wave publishes the step's record.  losses = HOST array of n (1 .. 16) device pointers to the step's fp32
 * loss scalars (the list drn_loss_guard gets), copied into the launch's arguments.  ring = uint32[slots][DRN_METRICS_RECORD_WORDS],
 * state = int32[4], both device memory; state[0] = records written so far (0 before the first call; [1..3] reserved).  The record of
 * call i goes to slot i % slots:
 *   word 0        i (the record index)                 word 1   n          word 2   nh          word 3   M
 *   words 4..19   bit patterns of the n losses, then zeros
 *   words 20..67  counts[k][0..5] of branch k at 20 + 6 k, zeros for k >= nh
 *   words 68..70  zero                                 word 71  i again (a reader accepts a record only if both index words agree)
 * then state[0] = i + 1, and all 64 words of `counts` are stored back as ZERO: the next step's drn_head_metrics finds its scratch
 * cleared without a memset node.  The slot comes from device memory, so a replayed graph advances through the ring; the kernel
 * boundary between the two launches is their only hand-off (no flag, no spinning).  Ordinary vector stores only.
 * Errors: DRN_ERR_UNSUPPORTED (n > 16, nh > 8), DRN_ERR_ARG (null pointer, n < 1, nh < 0, M < 0, slots < 1).
 *
 * The annotated-box block (opt-in; ROIHeads.enable_metrics(annotated=True)).  Every head class of the reference first labels its
 * proposals against the ANNOTATED boxes (label_and_sample_proposals, roi_heads.py:256-353, called from roi_heads_oicr.py:266,
 * roi_heads_wsddn.py:218, roi_heads_pcl.py:235, roi_heads_csc.py:252) and logs roi_head/num_{fg,bg,ig}_samples; its MIL predictor
 * then logs fast_rcnn/{cls_accuracy,fg_cls_accuracy,false_negative} of the MIL scores against those labels
 * (WSDDNOutputs._log_accuracy, fast_rcnn.py:213-235).  The boxes feed these six scalars and no loss.
 *
 * drn_label_proposals: proposals = fp32 [M, 4] (16-byte aligned), img_off = int32[n_img + 1] row offsets, gt_boxes = fp32
 * [n_img, max_gt, 4], gt_classes = int32 [n_img, max_gt], gt_count = int32[n_img] (all device memory; a count is clamped to
 * 0 .. max_gt), thresholds / match_labels = HOST arrays of nthr (1 .. 3) IoU thresholds and nthr + 1 Matcher labels in {-1, 0, 1},
 * max_rows = an upper bound of the rows of one image (sizes the grid).  For row r of image i and annotated box j of that image, in
 * fp32, this operation order, no contraction (detectron2/structures/boxes.py:329-361):
 *   a1 = (X2 - X1) * (Y2 - Y1) of the annotated box, a2 = (x2 - x1) * (y2 - y1) of the proposal,
 *   inter = max(min(X2, x2) - max(X1, x1), 0) * max(min(Y2, y2) - max(Y1, y1), 0),   iou = inter > 0 ? inter / (a1 + a2 - inter) : 0
 * which equals torch's pairwise_iou bit for bit.  v = the maximum over j, matched[r] = its j; DEFINITION: on equal IoU the LOWEST
 * box index wins (so a row that overlaps nothing is matched to box 0).  Matcher (detectron2/modeling/matcher.py,
 * allow_low_quality_matches = False): with t_0 = -inf, t_1 .. t_nthr = thresholds, t_nthr+1 = +inf, the Matcher label is
 * match_labels[q] for the q with t_q <= v < t_q+1; labels[r] = K for 0, -1 for -1, the class of box matched[r] for 1.  An image with
 * no annotated box: labels K, matched 0 (roi_heads.py:234-246).  counts = int32[>= 3], device memory: [0] += #{label == -1},
 * [1] += #{label == K}, [2] += the rest, over all images, as exact integers (one atomicAdd(int*) per non-zero counter and workgroup;
 * no float atomic, no host sync, capturable).  One thread per row, 256 rows of ONE image per workgroup, the image's boxes in LDS.
 * NaN coordinates: unspecified.
 * Shape class: n_img >= 0, M >= 0, 1 <= max_gt <= DRN_LABEL_MAX_GT, 1 <= nthr <= 3, K >= 1 (n_img, M or max_rows == 0: no launch).
 * Errors: DRN_ERR_UNSUPPORTED (max_gt > DRN_LABEL_MAX_GT, nthr > 3), DRN_ERR_ARG (null / misaligned pointer, sizes, a label outside
 * {-1, 0, 1}).
 *
 * drn_mil_metrics: drn_head_metrics' statistics of ONE fp32 matrix scores[rows >= M, lds] with an explicit column count and
 * background index - what fast_rcnn.py:213-235 computes of the MIL scores [M, K]: bg_ind = shape[1] - 1 = ncol - 1 (the LAST CLASS
 * column stands in for the background there; restated as it is).  p = the FIRST maximal index of scores[r, 0 .. ncol), g = labels[r]:
 *   counts[3] += #{p == g}   [4] += #{0 <= g < bg_ind, p == g}   [5] += #{0 <= g < bg_ind, p == bg_ind}   [6] += #{0 <= g < bg_ind}
 * ([0..2] are drn_label_proposals').  Shape class: 1 <= ncol <= 1024, bg_ind == ncol - 1, lds >= ncol, any M >= 0.
 * Errors: DRN_ERR_UNSUPPORTED (ncol > 1024, another bg_ind), DRN_ERR_ARG.
 *
 * drn_metrics_record_annot: drn_metrics_record with one more argument; annot == 0 is drn_metrics_record.  annot != 0: row
 * DRN_METRICS_ANNOT_ROW of `counts` is the annotated-box block and is published in the record's unused space,
 *   words 62..67  counts[7][0..5] (the last head slot)     word 68  counts[7][6]     word 70  DRN_METRICS_ANNOT_FLAG
 * so nh may be at most 7 (DRN_ERR_UNSUPPORTED otherwise).  A record without the block has zeros there, as before. */
#define DRN_METRICS_MAX_HEADS 8
#define DRN_METRICS_MAX_LOSSES 16
#define DRN_METRICS_COUNTERS 6
#define DRN_METRICS_COUNT_STRIDE 8
#define DRN_METRICS_ROWS_PER_BLOCK 64
#define DRN_METRICS_RECORD_WORDS 72
int drn_head_metrics(const float* logits, long ldl, const int* col0s, int nh, int K, const void* const* labels, int M, int* counts,
                     void* stream);
int drn_metrics_record(const void* const* losses, int n, int* counts, int nh, int M, unsigned* ring, int slots, int* state,
                       void* stream);
#define DRN_LABEL_MAX_GT 256
#define DRN_METRICS_ANNOT_ROW 7
#define DRN_METRICS_ANNOT_WORD_FG 68
#define DRN_METRICS_ANNOT_WORD_FLAG 70
#define DRN_METRICS_ANNOT_FLAG 1u
int drn_label_proposals(const float* proposals, const int* img_off, int n_img, int M, int max_rows, const float* gt_boxes,
                        const int* gt_classes, const int* gt_count, int max_gt, const float* thresholds, const int* match_labels,
                        int nthr, int K, int* labels, int* matched, int* counts, void* stream);
int drn_mil_metrics(const float* scores, long lds, int ncol, int bg_ind, const int* labels, int M, int* counts, void* stream);
int drn_metrics_record_annot(const void* const* losses, int n, int* counts, int nh, int M, int annot, unsigned* ring, int slots,
                             int* state, void* stream);

/* ---- inference tail -------------------------------------------------------------------------- */

/* fast_rcnn_inference_single_image, fast_rcnn.py:88-141 + batched_nms, detectron2/layers/nms.py:10-29. */
long drn_detect_workspace_bytes(int cap);
int drn_detect_topk(const float* boxes, const float* scores, int R, int K, int nreg, float img_h, float img_w,
                    float score_thresh, float nms_thresh, int topk, void* workspace, long workspace_bytes, int cap,
                    int* keep_ids, int* n_keep, void* stream);
int drn_detect_gather(const void* workspace, long workspace_bytes, int cap, const int* keep_ids, const int* n_keep,
                      int topk, float* out_boxes, float* out_scores, int* out_classes, int* out_rows, void* stream);

/* The single-image tail without the cap (fast_rcnn.py:88-141 with any topk_per_image; `topk < 0` = "return all detections",
 * fast_rcnn.py:65,133): the candidate stages of drn_detect_topk (finite-row filter, background column dropped, clip,
 * score > thresh, row-major compaction, stable descending sort), then the panelled NMS of drn_batched_nms over ALL sorted
 * candidates (class offset by the largest clipped coordinate + 1 below 40000 candidates, per-class on the raw boxes from 40000
 * on - decided by the candidate count on the device), then the gather.  topk < 0 keeps every survivor, topk >= 1 the first topk
 * (no 1024 limit; later panels retire at once when topk is reached); topk == 0 is DRN_ERR_ARG.  Outputs are sized by the caller for
 * cap entries: out_boxes [cap][4], out_scores / out_classes / out_rows [cap]; out_count [1] on the device; slots at and beyond
 * the count are not written.  cap >= R, and cap = R * K is always enough; R * K and cap above DRN_NMS_MAX_N are
 * DRN_ERR_UNSUPPORTED before any launch.  Workspace: 16-byte aligned, drn_detect_all_workspace_bytes(cap) bytes (linear in cap).
 * Nothing is read back; the launch count depends on R * K and cap alone.  drn_detect_topk and the batched tails keep their form
 * and their limits. */
long drn_detect_all_workspace_bytes(int cap);
int drn_detect_all(const float* boxes, const float* scores, int R, int K, int nreg, float img_h, float img_w,
                   float score_thresh, float nms_thresh, int topk, void* workspace, long workspace_bytes, int cap,
                   float* out_boxes, float* out_scores, int* out_classes, int* out_rows, int* out_count, void* stream);

/* The batched, sync-free inference tail: all images of a call through ONE launch chain whose length does not depend on
 * n_images, and nothing is read back by the host.
 * boxes [M][4*nreg], scores [M][K+1] with the rows of image b contiguous: img_off_host [n_images + 1] (HOST, ascending from 0
 * to M).  geom_host [n_images][6] (HOST) = per image (h, w, out_h, out_w, sx, sy): the candidates are clipped to (h, w) as the
 * single-image entry clips them; with postprocess != 0 the kept boxes then go through detector_postprocess
 * (projects/WSL/wsl/modeling/postprocessing.py) - x * sx, y * sy in fp32 (sx = out_w / w, sy = out_h / h formed in double and
 * rounded once by the caller, what Boxes.scale does with a Python float on an fp32 tensor), clip to (out_h, out_w), boxes with
 * w <= 0 or h <= 0 dropped keeping the order.  With postprocess == 0 the raw tail is delivered (out_h, out_w, sx, sy unused).
 * Outputs are padded blocks: out_boxes [n_images][topk][4], out_scores / out_classes / out_rows [n_images][topk], out_count
 * [n_images].  Image b's first out_count[b] slots equal, bit for bit, the single-image entries on that image's rows (followed by
 * the postprocess); out_rows are row indices WITHIN the image, after its own finite-row filter.  Slots at and beyond the count
 * hold boxes / scores 0 and classes / rows -1: the buffers are a function of the inputs alone.  Per image, as in the reference:
 * the finite-row filter, the boxes.max() + 1 class offset (integer-bits atomic max), the >= 40000 candidates switch to per-class
 * NMS decided by the image's own candidate count, the clip, the early exit at topk <= 1024.
 * Limits (DRN_ERR_UNSUPPORTED before any launch; callers chunk): 1 <= n_images <= DRN_DETECT_MAX_IMAGES,
 * M * K <= DRN_DETECT_BATCH_MAX_ENTRIES (the sort's tile table).  total_cap >= M * K sizes the workspace. */
#define DRN_DETECT_MAX_IMAGES 16
#define DRN_DETECT_BATCH_MAX_ENTRIES 4194304
long drn_detect_batch_workspace_bytes(int total_cap, int n_images);
int drn_detect_topk_batch(const float* boxes, const float* scores, const int* img_off_host, int n_images, int K, int nreg,
                          const float* geom_host, int postprocess, float score_thresh, float nms_thresh, int topk,
                          void* workspace, long workspace_bytes, int total_cap, float* out_boxes, float* out_scores,
                          int* out_classes, int* out_rows, int* out_count, void* stream);
/* Padded blocks -> packed detections: n_blocks blocks of topk slots, concatenated (boxes [n_blocks][topk][4], scores / classes
 * [n_blocks][topk]), count [n_blocks] (held to 0 .. topk) and image_index [n_blocks].  The live slots are packed in block order
 * then slot order into out_boxes [n][4], out_scores / out_classes / out_images [n] (capacity n_blocks * topk), and n is written
 * to out_n [1] on the device.  offsets [n_blocks + 1] is scratch.  Two launches: a prefix over count, a gather. */
int drn_detect_compact(const float* boxes, const float* scores, const int* classes, const int* count, const int* image_index,
                       int n_blocks, int topk, int* offsets, float* out_boxes, float* out_scores, int* out_classes,
                       int* out_images, int* out_n, void* stream);

/* ---- stand-alone box operators: nms, batched_nms, pairwise_iou, Matcher ---------------------------------------------
 * drn_nms: torchvision nms as oracle/roi_ops.c:223-252 states it.  boxes [n][4] fp32 XYXY, scores [n]; neither is written.
 *   Order: descending score, stable - equal scores keep ascending input index (the tie rule of the inference tail).
 *   Box j is suppressed by a kept earlier box i iff inter / (area_i + area_j - inter) > iou_thr in fp32 with exactly that operation
 *   order, uncontracted; the comparison is strict; a NaN ratio (two zero-area boxes) compares false, so both stay.
 *   keep [n] int64: keep[0 .. n_keep[0]) = original indices in descending-score order; words beyond n_keep[0] are unspecified.
 *   A NaN score is undefined and stays undefined (nothing is read or written out of bounds).
 * drn_batched_nms: detectron2/layers/nms.py:10-29 with idxs [n] int32.  n < 40000: every box is offset by
 *   (float) idx * (max over all 4 n coordinates + 1.f) in fp32 - the maximum is reduced on the device (integer max of order-preserving
 *   keys) - and the rule above runs on the offset boxes.  n >= 40000: boxes suppress only boxes of their own class, on the raw
 *   coordinates; the result is in descending-score order with the same tie rule.
 * Form: the package's stable radix passes, then per panel of 512 sorted rows one launch of 64 x 64 IoU tiles over many workgroups
 * (64-bit suppression words) and one launch that resolves the panel in order and ORs the kept rows' words into a removed-bitmap;
 * 12 + 2 * ceil(n / 512) launches (11 for drn_nms, and for n >= 40000), a function of n alone: capturable.  No host read, no
 * allocation, no float atomics; everything on the caller's stream.  n = 0 launches one store of n_keep = 0 (the other pointers
 * may be NULL).  Cap: n <= DRN_NMS_MAX_N, beyond it DRN_ERR_UNSUPPORTED before any launch.
 * Workspace: 16-byte aligned, DRN_NMS_WS_BYTES(n) = drn_nms_workspace_bytes(n) bytes - a 512-row panel of n / 64 words plus the
 * sort and the sorted boxes, linear in n (never n^2). */
#define DRN_NMS_MAX_N 524288
#define DRN_NMS_WS_BYTES(n) (104L * (n) + 65536L)
long drn_nms_workspace_bytes(long n);
int drn_nms(const float* boxes, const float* scores, long n, float iou_thr, void* workspace, long workspace_bytes,
            long long* keep, int* n_keep, void* stream);
int drn_batched_nms(const float* boxes, const float* scores, const int* idxs, long n, float iou_thr, void* workspace,
                    long workspace_bytes, long long* keep, int* n_keep, void* stream);
/* pairwise_iou (detectron2/structures/boxes.py:329-361): a [N][4], b [M][4] fp32 XYXY -> out [N][M] fp32, the fp32 formula of
 * drn_label_proposals and drn_proposal_recall (inter > 0 ? inter / (area_a + area_b - inter) : 0, uncontracted).  An empty N or M
 * launches nothing. */
int drn_pairwise_iou(const float* a, const float* b, long N, long M, float* out, void* stream);
/* Matcher.__call__ (detectron2/modeling/matcher.py:61-103) for allow_low_quality_matches = False: quality [N][M] fp32 on the
 * device; thresholds [n_thr] and labels [n_thr + 1] (each -1, 0 or 1) are HOST arrays, n_thr <= 3 (DRN_ERR_UNSUPPORTED beyond).
 * matches [M] int64 = the row of the column's maximum (the first row on ties), match_labels [M] int8 = labels[t] for the interval
 * thresholds[t - 1] <= max < thresholds[t] over (-inf, thresholds.., +inf).  N = 0: matches = 0, match_labels = labels[0]. */
int drn_match(const float* quality, long N, long M, const float* thresholds, int n_thr, const int* labels, long long* matches,
              signed char* match_labels, void* stream);

/* ---- test-time augmentation ------------------------------------------- */

/* GeneralizedRCNNWithTTAAVG._get_augmented_boxes (projects/WSL/wsl/modeling/test_time_augmentation_avg.py:269-294):
 * fold one augmentation's predictions into the running averages.  boxes [n_boxes][4] (the [R, 4K] prediction viewed
 * as boxes, in the augmented image's coordinates) are mapped back through HFlipTransform.inverse (flip_w = width of
 * the augmented image, < 0 = not flipped) and ResizeTransform.inverse (sx = w / new_w, sy = h / new_h, float32 like
 * the reference's numpy code) and added to acc_boxes; scores [n_scores] are added to acc_scores.  first = 1 starts the
 * sums, n_final = number of augmentations on the last call (the means are written then), 0 otherwise. */
int drn_tta_accumulate(const float* boxes, const float* scores, float* acc_boxes, float* acc_scores, long n_boxes,
                       long n_scores, float sx, float sy, float flip_w, int first, int n_final, void* stream);

/* GeneralizedRCNNWithTTAUNION._get_augmented_boxes + _merge_detections (projects/WSL/wsl/modeling/
 * test_time_augmentation_union.py:228-264): the detections of every augmentation's own inference tail, mapped back to the
 * original image and merged by ONE more threshold / NMS / top-k over their union, for all images of a call in one launch chain
 * (2 launches that build the candidates + the tail drn_detect_topk_batch runs behind its own candidates); nothing is read back.
 * Inputs are the padded blocks drn_detect_topk_batch leaves: blk_boxes [n_blocks][blk_topk][4], blk_scores / blk_classes
 * [n_blocks][blk_topk], blk_count [n_blocks] on the device.  The blocks of image i are img_off_host[i] .. img_off_host[i + 1]
 * (HOST, ascending from 0 to n_blocks).  tfm_host [n_blocks][3] (HOST) = per block (sx, sy, flip_w) of drn_tta_accumulate;
 * geom_host [n_images][2] (HOST) = (h, w) of the original image.
 * Slot s of block b is a union row iff s < min(blk_count[b], blk_topk); nothing beyond a block's count is read.  Its box goes
 * through the float32 inverse transform of drn_tta_accumulate; a row whose mapped box or score is not finite is dropped before
 * numbering (detectron2 fast_rcnn.py:95-98), and out_rows index the image's remaining union rows in (block, slot) order.  A row
 * is a candidate iff score > score_thresh (the reference passes 1e-8) and 0 <= class < K; its box is clipped to (h, w).
 * Candidate order = (block, slot) = the row-major nonzero() order of the reference's one-hot [n, K + 1] score matrix, so the
 * stable sort keeps score ties in union order.  Outputs: padded blocks [n_images][topk] with the layout and fill rule of
 * drn_detect_topk_batch (no postprocess: merged instances stay on the original image's (h, w)).
 * Limits (DRN_ERR_UNSUPPORTED before any launch): 1 <= n_images <= DRN_DETECT_MAX_IMAGES, 1 <= n_blocks <=
 * DRN_DETECT_UNION_MAX_BLOCKS, 1 <= blk_topk <= 1024, 1 <= topk <= 1024.  total_cap >= n_blocks * blk_topk sizes the workspace. */
#define DRN_DETECT_UNION_MAX_BLOCKS 256
long drn_detect_union_workspace_bytes(int total_cap, int n_images);
int drn_detect_union_batch(const float* blk_boxes, const float* blk_scores, const int* blk_classes, const int* blk_count,
                           int n_blocks, int blk_topk, const int* img_off_host, int n_images, const float* tfm_host,
                           const float* geom_host, int K, float score_thresh, float nms_thresh, int topk, void* workspace,
                           long workspace_bytes, int total_cap, float* out_boxes, float* out_scores, int* out_classes,
                           int* out_rows, int* out_count, void* stream);

/* ---- COCO box-AP evaluation (COCOEvaluator -> COCOeval_opt; detectron2/layers/csrc/cocoeval/cocoeval.cpp) -----------
 * The two native stages of the reference's evaluator, EvaluateImages (:141-198) and Accumulate (:371-497), on the device
 * and bit-identical to the C++: integer counts and single IEEE fp64 operations in its order.  The IoU is pycocotools'
 * bbIou on [x, y, w, h] in fp64 (w = min(dx + dw, gx + gw) - max(dx, gx), zero overlap -> 0, i = w * h,
 * u = crowd ? da : da + ga - i, i / u, uncontracted), restated because the reference tree does not hold it.  No threshold
 * is built in: IoU thresholds, area ranges, maxDets and recall thresholds are device arrays the caller computes in fp64.
 *
 * Caps: at most DRN_COCO_MAX_GT ground-truth boxes per (image, category) pair (the pair's LDS layout), A <=
 * DRN_COCO_MAX_AREAS area ranges with A * T <= 64 (one lane per (area range, IoU threshold)), R <= DRN_COCO_MAX_REC
 * recall thresholds; beyond a cap both entry points answer DRN_ERR_UNSUPPORTED before anything is launched - nothing is
 * truncated.  Scores are float32 (what a detector emits; the reference widens them to double, which keeps their order) and
 * must not be NaN.  Workspaces: 16-byte aligned, DRN_COCO_WS_BYTES(n, segments) bytes, segments = P for the matching and
 * K for the accumulation.  stages: bit 0 = the ordering passes, bit 1 = the matching / curve kernels; 3 runs both, and a
 * call with bit 1 alone continues from the same workspace that a call with bit 0 alone left (used to time them apart).
 *
 * drn_coco_match: n detections in input order: det_box [n][4] fp64 XYWH, det_score [n], det_pair [n] = image index * K +
 * category index (P = images * K pairs; indices are ranks of the ascending image / category ids).  Ground truth grouped
 * by pair in annotation order: gt_box [G][4] fp64 XYWH, gt_area [G] (the annotation's area field), gt_crowd [G], gt_off
 * [P + 1]; max_gt = the largest gt_off[p + 1] - gt_off[p], which the caller knows on the host.  iou_thr [T], area_rng
 * [A][2] (inclusive bounds).  Output, detections ordered by (pair, descending score, input order - stable): order [n]
 * (input index), s_score / s_cat / s_rank [n] (score, category index, rank inside the pair); dm / di [n]: bit a * T + t
 * of dm = matched, of di = ignored, for area range a and threshold t (both 0 for rank >= max_det: the reference drops
 * those detections); npig [P][A] = GT of the pair not ignored in area range a; gt_ign [G]: bit a = GT ignored
 * (iscrowd || area < lo || area > hi). */
#define DRN_COCO_MAX_GT 512
#define DRN_COCO_MAX_AREAS 4
#define DRN_COCO_MAX_REC 128
#define DRN_COCO_WS_BYTES(n, segments) (40L * ((n) + 4) + 8192L * (((n) + 4095) / 4096 + 1) + 32L * (segments) + 1024L)
int drn_coco_match(const double* det_box, const float* det_score, const int* det_pair, int n, const double* gt_box,
                   const double* gt_area, const unsigned char* gt_crowd, const int* gt_off, int P, int K, int max_gt,
                   const double* iou_thr, int T, const double* area_rng, int A, int max_det, void* workspace,
                   long workspace_bytes, int stages, int* order, float* s_score, int* s_cat, int* s_rank,
                   unsigned long long* dm, unsigned long long* di, int* npig, unsigned char* gt_ign, void* stream);
/* drn_coco_accumulate: the records drn_coco_match left (any order that lists every image's pairs by ascending image index
 * and every pair's detections by rank) and npig [I * K][A].  Per (category k, area range a, maxDet m, threshold t): the
 * detections of category k with rank < max_dets[m] (max_dets [M], none above the matching's max_det), by descending score
 * (stable), tp / fp counted over the not-ignored ones, recall = tp / npig, precision = tp / (tp + fp) (no eps: the C++,
 * not pycocotools), the backward running-max envelope, sampled at lower_bound(recall, rec_thr[r]) (0 beyond the end).
 * Writes precision / scores [T][R][K][A][M] and recall [T][K][A][M], fp64; entries stay -1 where the category has no
 * not-ignored GT in the area range. */
int drn_coco_accumulate(const float* s_score, const int* s_cat, const int* s_rank, const unsigned long long* dm,
                        const unsigned long long* di, int n, const int* npig, int I, int K, int T, int A,
                        const int* max_dets, int M, const double* rec_thr, int R, void* workspace, long workspace_bytes,
                        int stages, double* precision, double* scores, double* recall, void* stream);

/* ---- Box-proposal recall: AR@k by area (COCOEvaluator's box_proposals task; detectron2/evaluation/coco_evaluation.py) ---
 * _evaluate_box_proposals (:372-480) for every (area range, limit) pair at once, on the device.  Per image that has at least
 * one ground-truth box and one proposal (others are skipped before anything is counted, :424-425): the boxes with
 * lo <= area <= hi (both ends inclusive, fp32; `area` is the annotation's field) are kept and counted into num_pos - also
 * when none is left, and before the proposals are cut; the proposals are taken by descending objectness logit and cut to
 * the limit; then min(P', G') rounds of greedy matching on pairwise_iou (fp32, detectron2/structures/boxes.py:329-361 in
 * torch's operation order, uncontracted): every live box's best live proposal, the best-covered live box, its IoU recorded
 * as entry j, box and proposal retired.  Entries past min(P', G') stay 0.
 *
 * Three rules the reference leaves open are this package's definition:
 *   1. the objectness order is stable: equal logits keep their input order;
 *   2. the first index wins, twice: among proposals of equal IoU for a box the lowest position in the sorted order, among
 *      boxes of equal best IoU the lowest annotation index (what torch.max does on the CPU);
 *   3. a NaN logit is undefined and stays undefined (nothing is read or written out of bounds).
 *
 * Caps: at most DRN_PROPOSAL_MAX_GT boxes per image and DRN_PROPOSAL_MAX_PER_IMAGE proposals per image after the cut;
 * max_gt / max_prop are the largest such numbers, which the caller knows on the host; beyond a cap the entry answers
 * DRN_ERR_UNSUPPORTED before anything is launched - nothing is truncated.
 *
 * Input, all on the device: the images' proposals concatenated, prop_box [P][4] fp32 XYXY (16-byte aligned), prop_logit
 * [P], prop_off [I + 1] (ascending, 0 .. P); the ground truth that is not crowd, concatenated in annotation order, gt_box
 * [G][4] fp32 XYXY, gt_area [G], gt_off [I + 1]; area_rng [A][2]; limits [L] int (<= 0: no cut); thresholds [T].
 * Output: overlaps [A][L][G] fp32 - per (area range, limit) every image's segment holds its recorded entries first and -1
 * (IoUs are >= 0) in the slots of boxes outside the range or of skipped images; counts [A][L][T] = entries >=
 * thresholds[t]; num_pos [A].  P = 0: every slot -1, counts and num_pos 0.  One stream-ordered chain of launches whatever
 * I is, no host read, capturable; integer atomics only, so the result is the same bits on every run.
 * Workspace: 16-byte aligned, at least the bytes the workspace query answers for P.  stages: bit 0 = the ordering passes,
 * bit 1 = the matching; 3 runs both, and a call with bit 1 alone continues from the workspace that a call with bit 0 alone
 * left (used to time them apart). */
#define DRN_PROPOSAL_MAX_GT 256
#define DRN_PROPOSAL_MAX_PER_IMAGE 4096
long drn_proposal_recall_workspace_bytes(int P);
int drn_proposal_recall(const float* prop_box, const float* prop_logit, const int* prop_off, int P, const float* gt_box,
                        const float* gt_area, const int* gt_off, int G, int I, int max_gt, int max_prop,
                        const float* area_rng, int A, const int* limits, int L, const float* thresholds, int T,
                        void* workspace, long workspace_bytes, int stages, float* overlaps, unsigned long long* counts,
                        unsigned long long* num_pos, void* stream);

/* ---- PASCAL VOC evaluation: AP and CorLoc (PascalVOCDetectionEvaluator; detectron2/evaluation/pascal_voc_evaluation.py) -
 * voc_eval (:237-350), voc_eval_corloc (:353-447) and voc_ap (:182-234) on the device, in fp64, operation for operation
 * (uncontracted), on the numbers the reference's text files hold: score "%.3f" = rint((double)s * 1000) / 1000, xmin / ymin
 * "%.1f" after an fp32 + 1, xmax / ymax "%.1f" = rint((double)x * 10) / 10 - exact for fp32 inputs.  Scores
 * and boxes must be finite.  Tie order is a definition: within a class, equal quantised scores keep their input order
 * (the reference's np.argsort is not stable, so its answer on ties is not a function of its inputs).  No threshold is built
 * in: the IoU thresholds and the VOC07 recall thresholds are device arrays the caller computes in fp64.
 *
 * Caps: at most DRN_VOC_MAX_GT ground-truth boxes per (image, class) pair (the per-lane `det` flag registers), T <= 64
 * (one lane per IoU threshold), R <= DRN_VOC_MAX_REC recall thresholds; beyond a cap the entry points answer
 * DRN_ERR_UNSUPPORTED before anything is launched - nothing is truncated.  Workspace: 16-byte aligned,
 * DRN_VOC_WS_BYTES(n, P) bytes.  stages: bit 0 = quantise + rank, bit 1 = overlaps + the per-pair walk; 3 runs both, and
 * one call with bit 1 alone continues from the workspace that a call with bit 0 alone left (used to time them apart).
 *
 * drn_voc_match: n detections in processing order: det_box [n][4] fp32 XYXY as predicted (0-based), det_score [n], det_pair
 * [n] = image index * K + class (P = images * K pairs).  Ground truth grouped by pair in annotation order: gt_box [G][4]
 * fp64, gt_diff [G] (difficult), gt_off [P + 1]; max_gt = the largest gt_off[p + 1] - gt_off[p], known on the host.
 * iou_thr [T].  Output in rank order - class ascending, quantised score descending, input order on ties: order [n] (input
 * index), s_score [n] (quantised), cls_off [K + 1] (the classes' segments), ovmax [n] / jmax [n] (_max_overlap over the
 * pair's GT, first index on equal maxima, -inf / -1 without GT), tp / fp [n]: bit t = the detection is a true / false
 * positive at iou_thr[t] (strict >; a match with a difficult box is neither; a second match with a box is a false
 * positive).  hit [P]: bit t = the pair has a box that is not difficult and its top-ranked detection has ovmax >
 * iou_thr[t] (0 for every other pair). */
#define DRN_VOC_MAX_GT 128
#define DRN_VOC_MAX_REC 16
#define DRN_VOC_WS_BYTES(n, P) (24L * ((n) + 4) + 8192L * (((n) + 4095) / 4096 + 1) + 4L * (P) + 1024L)
int drn_voc_match(const float* det_box, const float* det_score, const int* det_pair, int n, const double* gt_box,
                  const unsigned char* gt_diff, const int* gt_off, int P, int K, int max_gt, const double* iou_thr, int T,
                  void* workspace, long workspace_bytes, int stages, int* order, double* s_score, int* cls_off,
                  double* ovmax, int* jmax, unsigned long long* tp, unsigned long long* fp, unsigned long long* hit,
                  void* stream);
/* drn_voc_accumulate: the tp / fp words, cls_off and hit that drn_voc_match left; npos [K] (boxes that are not difficult)
 * and npos_im [K] (images with such a box) from the annotations.  Per (class k, threshold t), in rank order: cumulative tp
 * / fp, rec = tp / npos (0 when npos = 0), prec = tp / max(tp + fp, DBL_EPSILON); use_07_metric != 0: for r in rec_thr [R]
 * (np.arange(0.0, 1.1, 0.1), R = 11) p = max prec over rec >= rec_thr[r] (0 if none), ap = ap + p / R in that order; else
 * the area under the monotone envelope, one term per recall step, summed in a fixed order (rec_thr unused).  Writes ap
 * [T][K] and corloc [T][K] = set hit bits / npos_im (0 for a class without detections or with npos_im = 0) and, when rec
 * and prec are given, the curves [n] (rank order) of threshold index t_curve. */
int drn_voc_accumulate(const unsigned long long* tp, const unsigned long long* fp, int n, const int* cls_off,
                       const unsigned long long* hit, const int* npos, const int* npos_im, int I, int K, int T,
                       const double* rec_thr, int R, int use_07_metric, int t_curve, double* ap, double* corloc,
                       double* rec, double* prec, void* stream);

/* ---- PCL refinement (PCLROIHeads) ------------------------------------------------------------------
 * The reference computes these on the HOST: the targets in numpy + scikit-learn after a device->host copy of the scores
 * (projects/WSL/wsl/modeling/roi_heads/third_party/pcl.py:26-200, called from fast_rcnn.py:1725-1745), the loss in C++ on
 * the CPU (projects/WSL/wsl/layers/csrc/pcl_loss/pcl_loss.h:52-131 always dispatches to pcl_loss_cpu.cpp:8-117).  One
 * image per call (the reference asserts a batch of one, pcl.py:94,149); R <= 4096, K <= 128.  Image batches: the two
 * *_batch entries below.
 *
 * drn_pcl_adjacency: `_build_graph` (pcl.py:78-87): bit r2 of word adj[r1][r2/32] = IoU(box r1, box r2) > iou_thr
 * (pairwise_iou, detectron2/structures/boxes.py:329-361).  adj: [R, ceil(R/32)] uint32.  Shared by every branch. */
int drn_pcl_adjacency(const float* boxes, int R, float iou_thr, uint32_t* adj, void* stream);

/* drn_pcl_refine: every refinement branch b < n_branch in one call.  logits [R, ld] fp32 holds branch b's K+1 columns
 * at cols[b] (host array; column 0 of a branch = background, class c at 1 + c - the PCL convention).  Branch 0 clusters
 * on wsddn_scores [R, ld_ws] (class c at column c), branch b > 0 on the softmax of branch b-1 (roi_heads_pcl.py:321-334).
 * onehot [K]: image-level labels.  Writes: probs [n_branch, R, K+1] (row softmax, fast_rcnn.py:1561-1575);
 * labels / cls_w / assign [n_branch, R] (pcl.py:166-181; assign = -1 for background rows); the proposal clusters
 * pc_labels / pc_probs / pc_count / img_w / pc_rows (row of the centre box) / pc_scores [n_branch, pmax] with their
 * number in n_pc [n_branch] (pmax >= 5 * labelled classes, <= 640); losses [n_branch] = pcl_loss forward summed over
 * classes / R (pcl_loss.py:51); dlogits [R, ld] at the same columns = d loss / d logits (pcl_loss_cpu.cpp:60-115 through
 * the softmax).  k-means and equal-degree ties follow the fixed definitions of oracle/pcl_oracle.py (the reference's
 * scikit-learn draw / numpy sort order are not functions of the inputs). */
int drn_pcl_refine(const float* logits, int ld, const int* cols, int n_branch, int K, const float* wsddn_scores,
                   int ld_ws, const float* boxes, const uint32_t* adj, const float* onehot, int R, float* probs,
                   int* labels, float* cls_w, int* assign, int* pc_labels, float* pc_probs, int* pc_count,
                   float* img_w, int* pc_rows, float* pc_scores, int* n_pc, int pmax, float* losses, float* dlogits,
                   void* stream);

/* ---- PCL refinement on image batches ------------------------------------------------------------------------------------
 * The reference has no batched PCL (pcl.py:90 asserts one image and its recipes run IMS_PER_BATCH = 4 as four processes
 * of one image); the definition is this package's.  A batch holds n_img images; image i owns rows
 * [img_off[i], img_off[i+1]) of boxes / logits / wsddn_scores (R_i rows, M rows in all) and the labels onehot[i].
 * img_off: DEVICE int32 [n_img + 1], ascending from 0 to M (what the MIL entries take); max_rows: a HOST bound on every
 * R_i.  Nothing is read back, so both entries can be captured into a graph.
 *   targets   every per-row and per-cluster output of image i and branch b, n_pc and probs are what drn_pcl_adjacency +
 *             drn_pcl_refine give for that image alone, bit for bit; pc_rows / assign hold rows LOCAL to the image
 *   loss_img  [n_img, n_branch]: the single-image loss (sum / R_i), bit for bit
 *   losses    [n_branch]: (float)((sum over i ascending of (double)loss_img[i][b]) / n_img) - the mean over images, in a
 *             fixed order without float atomics
 *   dlogits   the rows of image i are the single-image rows, every entry multiplied once more by 1.f / (float)n_img
 *             (exact for n_img = 1, 2, 4, 8, 16)
 *   an image without labels follows oracle/pcl_oracle.py like the single-image entry (no centres, loss 0, dlogits 0)
 * Limits: 1 <= n_img <= DRN_PCL_MAX_IMAGES, max_rows <= 4096 (the per-image limit of the single entries), K <= 128,
 * pmax <= 640: beyond them DRN_ERR_UNSUPPORTED.  M > n_img * max_rows (some image must exceed the bound) is DRN_ERR_ARG.
 * What the host cannot see: an image whose R_i on the device is outside 1 .. max_rows (or runs past M) is skipped by
 * both entries - none of its rows is written, its n_pc is 0 and its loss_img NaN, which makes the batch loss NaN.
 *
 * drn_pcl_adjacency_batch: adj [M, W] uint32 with W = ceil(max_rows / 32), the same for every image: bit c of word
 * adj[img_off[i] + r][c / 32] = IoU(box r, box c of image i) > iou_thr, c LOCAL to the image.  Every word of an image's
 * rows is written: bits at and beyond R_i, and whole words beyond ceil(R_i / 32), are zero.  Grid: (word, 256-row block,
 * image). */
#define DRN_PCL_MAX_IMAGES 16
int drn_pcl_adjacency_batch(const float* boxes, const int* img_off, int n_img, int M, int max_rows, float iou_thr,
                            uint32_t* adj, void* stream);

/* drn_pcl_refine_batch: drn_pcl_refine for every (branch, image) pair in one launch of n_branch * n_img workgroups, behind
 * one row softmax over all M rows and in front of the one-wave mean.  Arguments as for drn_pcl_refine, with: onehot
 * [n_img, K]; adj as written by drn_pcl_adjacency_batch with the same max_rows; probs [n_branch, M, K+1]; labels / cls_w /
 * assign [n_branch, M] (image i at columns img_off[i] ..); pc_* / img_w [n_img, n_branch, pmax]; n_pc and loss_img
 * [n_img, n_branch]; losses [n_branch]; dlogits [M, ld]. */
int drn_pcl_refine_batch(const float* logits, int ld, const int* cols, int n_branch, int K, const float* wsddn_scores,
                         int ld_ws, const float* boxes, const uint32_t* adj, const float* onehot, const int* img_off,
                         int n_img, int M, int max_rows, float* probs, int* labels, float* cls_w, int* assign,
                         int* pc_labels, float* pc_probs, int* pc_count, float* img_w, int* pc_rows, float* pc_scores,
                         int* n_pc, int pmax, float* loss_img, float* losses, float* dlogits, void* stream);

/* ---- CSC head (CSCROIHeads) -------------------------------------------------------------------------
 * projects/WSL/wsl/modeling/roi_heads/roi_heads_csc.py:423-510 and wsl/layers/csrc/csc/csc_cuda.cu.  One image per
 * call (the reference head reads image_sizes[0] / gt_classes_img_oh[0]); K <= 128.
 *
 * drn_csc_cpg: the per-class map of `_forward_cpg` (roi_heads_csc.py:456-464) from d (sum_r score[r, c]) / d image
 * (NHWC, `cpad` stored channels, the first C are colours; dtype DRN_F32 / DRN_BF16): |.|, max over the C channels,
 * divided by the maximum of the map -> cpg [H*W] fp32.  scratch: 4 bytes. */
int drn_csc_cpg(const void* dimg, int dtype, int cpad, int C, int H, int W, float* cpg, void* scratch, void* stream);

/* drn_csc_weights: `csc_forward_cuda` for ONE labelled class c (csc_cuda.cu:398-535): cpg >= fg_threshold ->
 * summed-area table (binary_and_integral_cpu :132-161; exact integer counts, H*W < 2^24) -> CSCPool (:184-350) per ROI
 * (rois [M][5] = batch index + box in image coordinates) -> max / min normalisation to [-1, 1] -> blend with the
 * image-level prediction sum_r scores[r][c] -> W[:, c] of W [M][K].  table: H*W floats of scratch.  The reference does
 * the table, the normalisation and the blend on the host; this stays on the stream. */
int drn_csc_weights(const float* cpg, int H, int W, float fg_threshold, const float* rois, int M, const float* scores,
                    int K, int c, int area_sqrt, float context_scale, float* table, float* Wout, void* stream);

/* drn_csc_loss: CSCOutputs.csc_loss (fast_rcnn.py:887-931) on the WSDDN scores (scores / row_softmax [M][K] as written
 * by drn_wsddn_fwd_bwd, logits as given to it).
 * mode 0: loss[0] = loss_cls_pos = BCE(clamp(sum_r s * max(W, 0)), onehot), loss[1] = loss_cls_neg =
 *         BCE(clamp(sum_r s * max(-W, 0)), 0) (W NULL = ones: past WSL.CSC_MAX_ITER) and, when dlogits != NULL, the
 *         cls / det columns of dlogits [M][ld_d] = d (loss[0] + loss[1]) / d logits.
 * mode 1: dlogits = d (sum_r scores[r][cstar]) / d logits - the seed of the image-gradient pass
 *         (roi_heads_csc.py:441-455, grad_outputs[:, c] = 1). */
int drn_csc_loss(const float* logits, long ld, int c_cls, int c_det, int K, int M, const float* scores,
                 const float* row_softmax, const float* W, const float* onehot, int mode, int cstar, int mean_loss,
                 float* loss, float* dlogits, long ld_d, void* stream);

/* ---- CSC on image batches (CSCROIHeads.enable_image_batches) ---------------------------------------------------------------
 * The reference has no batched CSC (roi_heads_csc.py:433-466 reads image_sizes[0] / gt_classes_img_oh[0]; its recipes run
 * IMS_PER_BATCH = 4 as four processes of one image); the definition is this package's.  A batch holds n_img images;
 * image i has its own size (H_i, W_i) inside the padded batch tensor [n_img, Hmax, Wmax, cpad], owns rows
 * [img_off[i], img_off[i+1]) of logits / scores / rois / W (M rows in all) and the labels onehot[i].
 *   map of image i, class c   the image gradient of (sum over image i's rows of score[r, c]) w.r.t. the padded batch tensor,
 *             cropped to (H_i, W_i), then |.|, max over the colours, divided by the maximum OF THAT CROP.  The padding is
 *             never read and never enters a maximum, a table or a box sum; CSCPool clamps image i's boxes to (H_i, W_i).
 *   per image the seed rows, the map, the table, W[rows of i, :] and loss_img[i] are what drn_csc_loss (mode 1) / drn_csc_cpg
 *             / drn_csc_weights / drn_csc_loss (mode 0) give for that image's slice alone, bit for bit: the same kernel
 *             bodies run on the slice.  (The image-gradient pass between seed and map is the trunk's and has its own tolerance.)
 *   loss      [2] = (float)((sum over i ascending of (double)loss_img[i][j]) / n_img): the mean over images in a fixed order,
 *             no float atomics; W NULL (past WSL.CSC_MAX_ITER: W = ones, no maps) takes the same mean
 *   dlogits   the rows of image i are the single-image rows, every entry multiplied once more by 1.f / (float)n_img
 * Slots: per image the labelled classes whose image score reaches tau, ascending, are its active classes; slot j carries the
 * j-th active class of every image (-1 where an image has fewer), so max_i |A_i| image-gradient passes over ALL rows serve the
 * batch.  A labelled class below tau keeps a zero map and still goes through drn_csc_weights_batch, as in the reference.
 * Integers that describe the step (hw, slot_cls, map_off, pairs, tab_off) are DEVICE int64 words: one upload per step holds
 * them all.  img_off: DEVICE int32 [n_img + 1], ascending from 0 to M (what the MIL entries take).
 * Limits: 1 <= n_img <= DRN_CSC_MAX_IMAGES, K <= 128 (as drn_csc_loss), H_i * W_i < 2^24 (as drn_csc_weights): beyond them
 * DRN_ERR_UNSUPPORTED, on the host, before any launch.  What the host cannot see - a row range outside 0 .. M, a size outside
 * 1 .. (Hmax, Wmax), a pair's image or class out of range - skips that image / pair: nothing of it is written (mode 0: its
 * loss_img is NaN, which makes the batch loss NaN).
 *
 * drn_csc_seed_batch: one workgroup per image, drn_csc_loss (mode 1) with cstar = slot_cls[i] on the image's rows.  Rows of an
 * image with slot_cls[i] = -1 are written as zeros (cls / det columns), so the d/dx pass carries an exact zero for it. */
#define DRN_CSC_MAX_IMAGES 16
int drn_csc_seed_batch(const float* logits, long ld, int c_cls, int c_det, int K, const float* scores,
                       const float* row_softmax, const int* img_off, int n_img, int M, const long* slot_cls,
                       float* dlogits, long ld_d, void* stream);

/* drn_csc_cpg_batch: dimg = the padded gradient [n_img, Hmax, Wmax, cpad] (the first C channels are colours).  For every image
 * with slot_cls[i] >= 0: drn_csc_cpg of the crop [H_i, W_i] -> maps + map_off[i] + slot_cls[i] * H_i * W_i (image i's
 * [K, H_i, W_i] block, offsets in floats); hw [n_img][2] = (H_i, W_i).  An image with -1 is not touched.  The maxima are per
 * image (integer atomicMax on the bits of non-negative floats: exact).  scratch: 4 * n_img bytes. */
int drn_csc_cpg_batch(const void* dimg, int dtype, int cpad, int C, int n_img, int Hmax, int Wmax, const long* hw,
                      const long* slot_cls, int K, const long* map_off, float* maps, void* scratch, void* stream);

/* drn_csc_weights_batch: drn_csc_weights for every pair p = (image pairs[2p], class pairs[2p+1]) of the step in three launches:
 * row scans over (row, pair), column scans over (64-column block, pair) - integer counts, exact in any order - and one CSCPool
 * workgroup per pair with csc_pool's fixed reduction order (`pred` is an fp32 sum) -> W[rows of the image, class].  Pairs must be
 * distinct.  tables + tab_off[p]: H_i * W_i floats of scratch per pair, the pair's summed-area table afterwards.  max_px: HOST
 * bound on every H_i * W_i (< 2^24).  Columns of W that no pair names are not touched. */
int drn_csc_weights_batch(const float* maps, const long* map_off, const long* hw, int n_img, int Hmax, int Wmax,
                          long max_px, const long* pairs, const long* tab_off, int n_pairs, float fg_threshold,
                          const float* rois, const int* img_off, int M, const float* scores, int K, int area_sqrt,
                          float context_scale, float* tables, float* Wout, void* stream);

/* drn_csc_loss_batch: one workgroup per image, drn_csc_loss (mode 0) on the image's rows with onehot[i] -> loss_img [n_img][2]
 * and, when dlogits != NULL, the 1 / n_img-scaled rows; then one wave forms loss [2] as defined above. */
int drn_csc_loss_batch(const float* logits, long ld, int c_cls, int c_det, int K, const float* scores,
                       const float* row_softmax, const float* W, const float* onehot, const int* img_off, int n_img, int M,
                       int mean_loss, float* loss_img, float* loss, float* dlogits, long ld_d, void* stream);

/* ---- CSC weight statistics (CSCROIHeads.enable_csc_stats; metrics.CscStats) ------------------------------------------------
 * The reference's `Statistic` (projects/WSL/wsl/modeling/roi_heads/third_party/cpg_stats.py, driven from CSCOutputs.csc_loss,
 * fast_rcnn.py:910-918) copies W_pos / W_neg [M, K] to the host every iteration and walks M x labelled classes in Python; every
 * LOG_PERIOD iterations it prints a table to csc.txt.  drn_csc_stats counts the same table on the device, one call per training
 * forward for all n_img images of the step, on the stream the losses run on, once W is final.
 * For image i with rows [img_off[i], img_off[i+1]) (R of them) and every class c with onehot[i][c] > 0.5:
 *   pred = clamp((float)(sum_r scores[r][c]), 1e-6, 1 - 1e-6)              predict_probs_img, fast_rcnn.py:950-962
 *   ori_label[c] += 1, ori_pred[c] += pred, ori_num_roi[c] += R
 *   and if (i, c) is ACTIVE:
 *   csc_label[c] += 1, csc_pred[c] += pred, csc_num_roi[c] += R
 *   csc_pred_pos[c] += clamp((float)(sum_r scores * max(W, 0)), 1e-20, 1.0),  csc_pred_neg[c] likewise with max(-W, 0)
 *   csc_roi_pos[c] += #{r: W[r][c] > 0}, csc_roi_neg[c] += #{W < 0}, csc_roi_zero[c] += #{neither} (-0.0 and NaN are zero
 *   weights, as the reference's `if > 0 / elif < 0 / else`)
 * num_img += 1 per image, steps += 1 per call.
 * ACTIVE is "this step built a map for (i, c)".  The host takes that decision (image score >= tau, CSCROIHeads._csc_weights /
 * csc_slot_schedule) and hands it over as the slot rows of the step - slots [n_slots][n_img] DEVICE int64, slots[j][i] = the
 * class image i carries in slot j or -1, exactly the plan of "CSC on image batches" (a single image: its active classes, one per
 * row).  The kernel never re-derives it from its own sums: a tie with tau in the last bit would make the log contradict the step.
 * Arithmetic: every row sum is ONE fp64 chain in ascending row order (the products scores * max(+-W, 0) are exact in fp64),
 * rounded to fp32 once and clamped; the table's sums are fp64, its counts int64; the images are folded into the table in
 * ascending image order by one thread per class.  No floating-point atomics, no atomics at all: the table after a call does not
 * depend on the launch geometry.
 * On an image batch each image is one `UpdateIterStats` call, in ascending image order - this package's definition, like the
 * batch itself (the reference's IMS_PER_BATCH = 4 are four processes that each write their own csc.txt).
 * table: DRN_CSC_STATS_WORDS(K) 8-byte words - int64 steps, num_img; int64 [DRN_CSC_STATS_INT][K] = ori_label, ori_num_roi,
 * csc_label, csc_num_roi, csc_roi_pos, csc_roi_neg, csc_roi_zero; fp64 [DRN_CSC_STATS_FP][K] = ori_pred, csc_pred, csc_pred_pos,
 * csc_pred_neg.  The caller zeroes it (and re-zeroes it after reading it).  scratch: DRN_CSC_STATS_SCRATCH_WORDS(n_img, K)
 * 8-byte words.  Limits as the batch entries: n_img <= DRN_CSC_MAX_IMAGES, K <= 128 (DRN_ERR_UNSUPPORTED beyond), n_slots <= K.
 * An image whose device-side row range is invalid (outside 0 .. M, or empty) is skipped whole: nothing of it is counted. */
#define DRN_CSC_STATS_HEAD 2
#define DRN_CSC_STATS_INT 7
#define DRN_CSC_STATS_FP 4
#define DRN_CSC_STATS_WORDS(K) (DRN_CSC_STATS_HEAD + (DRN_CSC_STATS_INT + DRN_CSC_STATS_FP) * (K))
#define DRN_CSC_STATS_SCRATCH_WORDS(n_img, K) ((n_img) * (1 + 6 * (K)))
int drn_csc_stats(const float* scores, const float* W, int K, const int* img_off, int n_img, int M, const float* onehot,
                  const long* slots, int n_slots, void* scratch, long* table, void* stream);

/* ---- launch plans (round 3): the frozen trunk's whole layer sequence in ONE call ----
 * Replaces the per-layer Python walk of `ResNet.forward` / `BasicStem.forward` / `BottleneckBlock.forward` /
 * `BasicBlock.forward` (projects/WSL/wsl/modeling/backbone/resnet_ws.py:479-502, :405-416, :217-237, :93-112) and
 * `VGG16.forward` / `PlainBlock.forward` (vgg.py:213-231, :104-122) when nothing has to be kept for a backward pass.
 * A plan is an array of ops over numbered activation SLOTS (buffers the caller owns; an op never writes its own input
 * or residual slot).  Geometry per op follows from the input size; every op runs through drn_conv2d_nhwc_q /
 * drn_maxpool2x2_nhwc, so the kernels, their selection and the results are those of the per-layer calls.
 * DRN_TRUNK_MAXPOOL is nn.MaxPool2d(2, stride): it reads `stride` alone, as it always did (ksize / pad are ignored).
 * DRN_TRUNK_MAXPOOL3X3 is F.max_pool2d(3, 2, 1) = drn_maxpool3x3s2_nhwc, the standard ResNet stem's pool
 * (detectron2/modeling/backbone/resnet.py:358): ksize = 3, stride = 2, pad = 1 must be set, anything else is an
 * argument error; output (H + 2 - 3) / 2 + 1 rows. */
#define DRN_TRUNK_CONV 0
#define DRN_TRUNK_MAXPOOL 1
#define DRN_TRUNK_MAXPOOL3X3 2
#define DRN_TRUNK_MAX_SLOTS 16
#define DRN_TRUNK_KIND_MASK 0xff
#define DRN_TRUNK_FUSE_POOL 0x200 /* flag on a conv op: its output is read by the NEXT op alone, a 2x2 / stride-2 max pool - may run inside the conv's launch (drn_conv3x3_pw_nhwc with pool = 1; with DRN_TRUNK_FUSE_NEXT on the op before it: three ops, one launch) */
#define DRN_TRUNK_FUSE_STEM 0x400 /* flag on a 7x7 / stride-2 / pad-3 conv op (8 stored -> 64 channels, ReLU): its output is read by the NEXT op alone, a DRN_TRUNK_MAXPOOL3X3 - the executor may run the pair as one drn_stem7x7_pool_nhwc launch (the conv's dst slot is then not written; bit-identical), and runs the two launches where that entry point answers DRN_ERR_UNSUPPORTED */
#define DRN_TRUNK_FUSE_NEXT 0x100 /* flag on a 3x3 / 64 -> 64 conv op: its output is read by the NEXT op alone, a 1x1 conv to 256 channels - the executor may run the pair as one drn_conv3x3_pw_nhwc launch (the dst slot is then not written) */
typedef struct DrnTrunkOp {
  int kind;           /* DRN_TRUNK_CONV | DRN_TRUNK_MAXPOOL | DRN_TRUNK_MAXPOOL3X3, optionally | DRN_TRUNK_FUSE_NEXT */
  int src, dst, res;  /* slot indices; res = -1: no residual (conv only) */
  const void* w;      /* conv: packed weights [cout][ldw] as for drn_conv2d_nhwc_q */
  const float* scale; /* per-cout affine (folded FrozenBN / quantisation scales) or NULL */
  const float* bias;
  int cin, cout, ksize, stride, pad, dil, relu; /* cin = stored channels of the input slot; DRN_TRUNK_MAXPOOL: stride only; DRN_TRUNK_MAXPOOL3X3: ksize 3, stride 2, pad 1 */
  long ldw;
  int dtype, out_dtype, res_dtype; /* element types of x / w, of y, of the residual (pool: dtype) */
  float res_mult;
} DrnTrunkOp;

/* Bytes every slot must hold for an [Nb, H, W, C0] input of element type in_dtype sitting in slot in_slot
 * (slot_bytes[n_slots]; 0 for slots the plan never writes), and the (h, w, c) each slot holds when the plan ends
 * (slot_hwc[3 * n_slots], may be NULL).  Host-only: launches nothing. */
int drn_trunk_shapes(const DrnTrunkOp* ops_host, int n_ops, int n_slots, int in_slot, int Nb, int H, int W, int C0,
                     int in_dtype, long* slot_bytes_host, int* slot_hwc_host);

/* Enqueue the whole plan.  slots_host[n_slots]: device pointers (16-byte aligned), each at least as large as
 * drn_trunk_shapes reported. */
int drn_trunk_forward(const DrnTrunkOp* ops_host, int n_ops, int n_slots, int in_slot, void* const* slots_host, int Nb,
                      int H, int W, int C0, int in_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DRN_WSOD_H_ */
