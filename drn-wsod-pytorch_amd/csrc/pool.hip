// HBM-bound feature-map utilities for gfx950: input normalisation, the 8-bit resize of the TTA mapper, the max pools and their
// backward, the transposed im2col, add, ROI staging, and a tiled cast + transpose.  NHWC everywhere: a wave reads 64
// consecutive channels = one 128-B (bf16) / 256-B (f32) line per spatial tap.  Built with -ffp-contract=off: the arithmetic is
// the oracle's, op for op.  (RoI pooling lives in roi.hip.)
//
// Replaces: GeneralizedRCNNWSL.preprocess_image (projects/WSL/wsl/modeling/meta_arch/rcnn.py:242-249),
// nn.MaxPool2d(2, stride) (resnet_ws.py:214-215,403; vgg.py:99-100) and convert_boxes_to_pooler_format
// (detectron2/modeling/poolers.py:69-96).
#include "drn_common.h"
#include <float.h>

namespace {

template <int DT>
__global__ void preprocess_kernel(const float* __restrict__ img, int C, int H, int W, typename ElemOf<DT>::type* out,
                                  int Hp, int Wp, int Cp, float m0, float m1, float m2, float s0, float s1, float s2) {
  const long total = (long)Hp * Wp * Cp;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = i % Cp;
    const long hw = i / Cp;
    const int w = hw % Wp, h = hw / Wp;
    float v = 0.f;
    if (c < C && h < H && w < W) {
      const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2);
      const float sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
      v = (img[((long)c * H + h) * W + w] - mean) / sd;
    }
    ElemOf<DT>::st(out + i, v);
  }
}

// Pillow's BILINEAR resample of an 8-bit image (ResizeTransform.apply_image, detectron2/data/transforms/transform.py:101-122, calls
// PIL.Image.resize(..., BILINEAR) for uint8 images; the 16 augmented images of one TTA image take ~0.4 s of it on the host,
// projects/WSL/wsl/modeling/test_time_augmentation_avg.py:68-137).  Pillow resamples in two integer passes - horizontal, the
// result rounded to 8 bits, then vertical - with per-output-position windows [xmin, xmin + n) and coefficients scaled by 2^22
// (Resample.c: precompute_coeffs / normalize_coeffs_8bpc; the host computes them with Pillow's own double arithmetic); here
// one thread forms one output pixel: the horizontal results of its vertical window's rows on the fly, rounded exactly as
// Pillow stores them, then the vertical sum.  Output: fp32 [C][Ho][Wo] (the integers 0 .. 255), optionally mirrored
// (HFlipTransform) - what preprocess_kernel reads.
__global__ void resize_u8_kernel(const unsigned char* __restrict__ src, int H, int W, int C, float* __restrict__ dst, int Ho,
                                 int Wo, const int* __restrict__ xb, const int* __restrict__ xk, int ksx,
                                 const int* __restrict__ yb, const int* __restrict__ yk, int ksy, int flip) {
  constexpr int PB = 22, HALF = 1 << (PB - 1);
  const long total = (long)Ho * Wo;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xx = (int)(i % Wo), yy = (int)(i / Wo);
    const int xmin = xb ? xb[2 * xx] : xx, xn = xb ? xb[2 * xx + 1] : 1;
    const int ymin = yb ? yb[2 * yy] : yy, yn = yb ? yb[2 * yy + 1] : 1;
    int acc[4] = {HALF, HALF, HALF, HALF};
    for (int y = 0; y < yn; ++y) {
      const unsigned char* row = src + ((long)(ymin + y) * W + xmin) * C;
      int h[4];
      if (xb) {
        int a[4] = {HALF, HALF, HALF, HALF};
        for (int x = 0; x < xn; ++x) {
          const int k = xk[(long)xx * ksx + x];
          for (int c = 0; c < C; ++c) a[c] += (int)row[x * C + c] * k;
        }
        for (int c = 0; c < C; ++c) h[c] = min(max(a[c] >> PB, 0), 255);
      } else {
        for (int c = 0; c < C; ++c) h[c] = row[c];
      }
      if (yb) {
        const int k = yk[(long)yy * ksy + y];
        for (int c = 0; c < C; ++c) acc[c] += h[c] * k;
      } else {
        for (int c = 0; c < C; ++c) acc[c] = h[c];
      }
    }
    const int xo = flip ? Wo - 1 - xx : xx;
    for (int c = 0; c < C; ++c)
      dst[((long)c * Ho + yy) * Wo + xo] = (float)(yb ? min(max(acc[c] >> PB, 0), 255) : acc[c]);
  }
}

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

// one thread = one 16-B channel vector of one output pixel
template <int DT>
__global__ void maxpool2x2_kernel(const char* __restrict__ x, char* __restrict__ y, int Nb, int H, int W, int C,
                                  int Ho, int Wo, int stride) {
  constexpr int ES = EsOf<DT>::value;
  constexpr int V = 16 / ES;
  const int cv = C / V;
  const long total = (long)Nb * Ho * Wo * cv;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (i % cv) * V;
    long t = i / cv;
    const int wo = t % Wo; t /= Wo;
    const int ho = t % Ho;
    const int n = t / Ho;
    const char* p00 = x + (((long)(n * H + ho * stride) * W + wo * stride) * C + c) * ES;
    const long dw = (long)C * ES, dh = (long)W * C * ES;
    char* dst = y + (((long)(n * Ho + ho) * Wo + wo) * C + c) * ES;
    if constexpr (DT == DRN_FP8) {
      // the quantised trunk pools post-ReLU tensors only: non-negative e4m3 values order like their bytes
      const u32x4_t a = *(const u32x4_t*)p00, b = *(const u32x4_t*)(p00 + dw);
      const u32x4_t d = *(const u32x4_t*)(p00 + dh), e = *(const u32x4_t*)(p00 + dh + dw);
      auto mx = [](unsigned ua, unsigned ub, unsigned ud, unsigned ue) -> unsigned {
        unsigned o = 0;
#pragma unroll
        for (int k = 0; k < 32; k += 8) {
          const unsigned m0 = max((ua >> k) & 0xffu, (ub >> k) & 0xffu), m1 = max((ud >> k) & 0xffu, (ue >> k) & 0xffu);
          o |= max(m0, m1) << k;
        }
        return o;
      };
      u32x4_t o;
      o.x = mx(a.x, b.x, d.x, e.x);
      o.y = mx(a.y, b.y, d.y, e.y);
      o.z = mx(a.z, b.z, d.z, e.z);
      o.w = mx(a.w, b.w, d.w, e.w);
      *(u32x4_t*)dst = o;
    } else if constexpr (DT == DRN_F32) {
      const f32x4_t a = *(const f32x4_t*)p00, b = *(const f32x4_t*)(p00 + dw);
      const f32x4_t d = *(const f32x4_t*)(p00 + dh), e = *(const f32x4_t*)(p00 + dh + dw);
      f32x4_t o;
      o.x = fmaxf(fmaxf(a.x, b.x), fmaxf(d.x, e.x));
      o.y = fmaxf(fmaxf(a.y, b.y), fmaxf(d.y, e.y));
      o.z = fmaxf(fmaxf(a.z, b.z), fmaxf(d.z, e.z));
      o.w = fmaxf(fmaxf(a.w, b.w), fmaxf(d.w, e.w));
      *(f32x4_t*)dst = o;
    } else {
      const u32x4_t a = *(const u32x4_t*)p00, b = *(const u32x4_t*)(p00 + dw);
      const u32x4_t d = *(const u32x4_t*)(p00 + dh), e = *(const u32x4_t*)(p00 + dh + dw);
      auto mx = [](unsigned ua, unsigned ub, unsigned ud, unsigned ue) -> unsigned {
        // two packed bf16 per dword; bf16 -> f32 is a shift, the max of bf16 values is again bf16
        const float lo = fmaxf(fmaxf(__builtin_bit_cast(float, ua << 16), __builtin_bit_cast(float, ub << 16)),
                               fmaxf(__builtin_bit_cast(float, ud << 16), __builtin_bit_cast(float, ue << 16)));
        const float hi = fmaxf(fmaxf(__builtin_bit_cast(float, ua & 0xffff0000u), __builtin_bit_cast(float, ub & 0xffff0000u)),
                               fmaxf(__builtin_bit_cast(float, ud & 0xffff0000u), __builtin_bit_cast(float, ue & 0xffff0000u)));
        return (__builtin_bit_cast(unsigned, lo) >> 16) | (__builtin_bit_cast(unsigned, hi) & 0xffff0000u);
      };
      u32x4_t o;
      o.x = mx(a.x, b.x, d.x, e.x);
      o.y = mx(a.y, b.y, d.y, e.y);
      o.z = mx(a.z, b.z, d.z, e.z);
      o.w = mx(a.w, b.w, d.w, e.w);
      *(u32x4_t*)dst = o;
    }
  }
}

// F.max_pool2d(x, kernel_size=3, stride=2, padding=1) of the standard ResNet stem (detectron2/modeling/backbone/resnet.py:358).
// One thread = one 16-B channel vector of one output pixel; the window is clipped to the map, which is what -inf padding
// amounts to (its centre tap (2 ho, 2 wo) always lies inside, so no window is empty).
template <int DT>
__global__ void maxpool3x3s2_kernel(const char* __restrict__ x, char* __restrict__ y, int Nb, int H, int W, int C, int Ho,
                                    int Wo) {
  constexpr int ES = EsOf<DT>::value;
  constexpr int V = 16 / ES;
  const int cv = C / V;
  const long total = (long)Nb * Ho * Wo * cv;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (i % cv) * V;
    long t = i / cv;
    const int wo = t % Wo; t /= Wo;
    const int ho = t % Ho;
    const int n = t / Ho;
    const int h0 = max(2 * ho - 1, 0), h1 = min(2 * ho + 1, H - 1);
    const int w0 = max(2 * wo - 1, 0), w1 = min(2 * wo + 1, W - 1);
    char* dst = y + (((long)(n * Ho + ho) * Wo + wo) * C + c) * ES;
    if constexpr (DT == DRN_F32) {
      f32x4_t o = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      for (int h = h0; h <= h1; ++h)
        for (int w = w0; w <= w1; ++w) {
          const f32x4_t a = *(const f32x4_t*)(x + (((long)(n * H + h) * W + w) * C + c) * ES);
          o.x = fmaxf(o.x, a.x);
          o.y = fmaxf(o.y, a.y);
          o.z = fmaxf(o.z, a.z);
          o.w = fmaxf(o.w, a.w);
        }
      *(f32x4_t*)dst = o;
    } else if constexpr (DT == DRN_BF16) {
      // two packed bf16 per dword; bf16 -> f32 is a shift, the max of bf16 values is again bf16
      float lo[4], hi[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) lo[k] = hi[k] = -INFINITY;
      for (int h = h0; h <= h1; ++h)
        for (int w = w0; w <= w1; ++w) {
          const u32x4_t a = *(const u32x4_t*)(x + (((long)(n * H + h) * W + w) * C + c) * ES);
          const unsigned u[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            lo[k] = fmaxf(lo[k], __builtin_bit_cast(float, u[k] << 16));
            hi[k] = fmaxf(hi[k], __builtin_bit_cast(float, u[k] & 0xffff0000u));
          }
        }
      unsigned r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        r[k] = (__builtin_bit_cast(unsigned, lo[k]) >> 16) | (__builtin_bit_cast(unsigned, hi[k]) & 0xffff0000u);
      u32x4_t o;
      o.x = r[0]; o.y = r[1]; o.z = r[2]; o.w = r[3];
      *(u32x4_t*)dst = o;
    } else {
      // the quantised trunk pools post-ReLU tensors only: non-negative e4m3 values order like their bytes
      unsigned r[4] = {0u, 0u, 0u, 0u};
      for (int h = h0; h <= h1; ++h)
        for (int w = w0; w <= w1; ++w) {
          const u32x4_t a = *(const u32x4_t*)(x + (((long)(n * H + h) * W + w) * C + c) * ES);
          const unsigned u[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            unsigned o = 0;
#pragma unroll
            for (int s = 0; s < 32; s += 8) o |= max((r[k] >> s) & 0xffu, (u[k] >> s) & 0xffu) << s;
            r[k] = o;
          }
        }
      u32x4_t o;
      o.x = r[0]; o.y = r[1]; o.z = r[2]; o.w = r[3];
      *(u32x4_t*)dst = o;
    }
  }
}

// ---- backward of the conv trunk (only when MODEL.BACKBONE.FREEZE_AT < 5) -------------------------------------
// Transposed im2col: out[(ci*KH + kh)*KW + kw][p] = x[n, ho*s + kh*d - pad, wo*s + kw*d - pad, ci] (0 outside),
// p = (n*Ho + ho)*Wo + wo.  It is the K-major B operand of the weight-gradient GEMM  dW[co][ci,kh,kw] = g^T . out^T,
// whose row order makes dW come out in the [Cout, Cin, KH, KW] state_dict layout.  64 pixels x 64 channels per block
// for one tap: channel-contiguous reads, pixel-contiguous writes through an LDS tile.
template <int DT>
__global__ __launch_bounds__(256) void im2col_t_kernel(const char* __restrict__ x, char* __restrict__ out, int Nb, int H,
                                                       int W, int Cin, int ldc, int KH, int KW, int stride, int pad,
                                                       int dil, int Ho, int Wo, long ld_out) {
  using E = ElemOf<DT>;
  using T = typename E::type;
  __shared__ T t[64][66];
  const int tap = blockIdx.z, kh = tap / KW, kw = tap - kh * KW;
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int P = Nb * Ho * Wo;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int p = p0 + i, c = c0 + tx;
    T v = (T)0;
    if (p < P && c < Cin) {
      const int wo = p % Wo, ho = (p / Wo) % Ho, n = p / (Wo * Ho);
      const int hi = ho * stride + kh * dil - pad, wi = wo * stride + kw * dil - pad;
      if (hi >= 0 && hi < H && wi >= 0 && wi < W) v = ((const T*)x)[((long)(n * H + hi) * W + wi) * ldc + c];
    }
    t[i][tx] = v;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int c = c0 + i, p = p0 + tx;
    if (c < Cin && p < P) ((T*)out)[((long)(c * KH + kh) * KW + kw) * ld_out + p] = t[tx][i];
  }
}

// d(x) of MaxPool2d(2, stride s, padding 0): every input pixel gathers from the (at most 4) windows that contain it
// and takes a window's gradient iff it is that window's first maximum in scan order (torch: `val > maxval`) -
// deterministic, no atomics even for the overlapping stride-1 windows of the dilated configs.
template <int DT>
__global__ void maxpool2x2_bwd_kernel(const char* __restrict__ x, const char* __restrict__ dy, char* __restrict__ dx,
                                      int Nb, int H, int W, int C, int Ho, int Wo, int stride) {
  using E = ElemOf<DT>;
  using T = typename E::type;
  const long total = (long)Nb * H * W * C;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = i % C;
    long r = i / C;
    const int w = r % W; r /= W;
    const int h = r % H;
    const int n = r / H;
    float acc = 0.f;
    for (int dh = 0; dh < 2; ++dh) {
      const int hs = h - dh;  // window start row if this pixel is row dh of the window
      if (hs < 0 || hs % stride) continue;
      const int ho = hs / stride;
      if (ho >= Ho) continue;
      for (int dw = 0; dw < 2; ++dw) {
        const int ws = w - dw;
        if (ws < 0 || ws % stride) continue;
        const int wo = ws / stride;
        if (wo >= Wo) continue;
        const T* base = (const T*)x + ((long)(n * H + hs) * W + ws) * C + c;
        float best = E::ld(base);
        int arg = 0;
        const float v1 = E::ld(base + C), v2 = E::ld(base + (long)W * C), v3 = E::ld(base + (long)W * C + C);
        if (v1 > best) { best = v1; arg = 1; }
        if (v2 > best) { best = v2; arg = 2; }
        if (v3 > best) { best = v3; arg = 3; }
        if (arg == dh * 2 + dw) acc += E::ld((const T*)dy + ((long)(n * Ho + ho) * Wo + wo) * C + c);
      }
    }
    E::st((T*)dx + i, acc);
  }
}

template <int DT>
__global__ void add_kernel(const char* __restrict__ a, const char* __restrict__ b, char* __restrict__ out, long n) {
  using E = ElemOf<DT>;
  using T = typename E::type;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    E::st((T*)out + i, E::ld((const T*)a + i) + E::ld((const T*)b + i));
}

// bf16 -> bf16 transpose with 16-B global accesses on both sides (the A -> A^T copy of the fc6 operand is
// 2 x 205 MB per step): 64x64 tile, rows read as 8-element vectors, written transposed into LDS, re-read as vectors.
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out,
                                                             int rows, int cols, long ld_in, long ld_out) {
  __shared__ bf16_t t[64][72];  // [c][r], row pitch 144 B keeps the 16-B reads aligned and spreads banks
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int v = threadIdx.x & 7, rr = threadIdx.x >> 3;  // 8 vectors per 64-element row, 32 rows per pass
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int r = r0 + rr + 32 * pass, c = c0 + v * 8;
    i32x4_t x = {0, 0, 0, 0};
    if (r < rows && c + 8 <= cols) x = *(const i32x4_t*)(in + (long)r * ld_in + c);
    else if (r < rows)
      for (int e = 0; e < 8; ++e)
        if (c + e < cols) ((bf16_t*)&x)[e] = in[(long)r * ld_in + c + e];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[v * 8 + e][rr + 32 * pass] = ((const bf16_t*)&x)[e];
  }
  __syncthreads();
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int c = c0 + rr + 32 * pass, r = r0 + v * 8;
    if (c >= cols) continue;
    const i32x4_t x = *(const i32x4_t*)(&t[rr + 32 * pass][v * 8]);
    if (r + 8 <= rows) *(i32x4_t*)(out + (long)c * ld_out + r) = x;
    else
      for (int e = 0; e < 8; ++e)
        if (r + e < rows) out[(long)c * ld_out + r + e] = ((const bf16_t*)&x)[e];
  }
}

// out[c][r] = (T_OUT) in[r][c]; 64x64 tiles through LDS, both sides coalesced.
template <int DT_IN, int DT_OUT>
__global__ __launch_bounds__(256) void transpose_kernel(const char* __restrict__ in, char* __restrict__ out, int rows,
                                                        int cols, long ld_in, long ld_out) {
  using EI = ElemOf<DT_IN>;
  using EO = ElemOf<DT_OUT>;
  __shared__ float t[64][65];
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    const int r = r0 + i, c = c0 + tx;
    t[i][tx] = (r < rows && c < cols) ? EI::ld((const typename EI::type*)in + (long)r * ld_in + c) : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 64; i += 4) {
    const int c = c0 + i, r = r0 + tx;
    if (c < cols && r < rows) EO::st((typename EO::type*)out + (long)c * ld_out + r, t[tx][i]);
  }
}

template <int DT_IN, int DT_OUT>
__global__ void cast2d_kernel(const char* __restrict__ in, char* __restrict__ out, int rows, int cols, long ld_in,
                              long ld_out) {
  using EI = ElemOf<DT_IN>;
  using EO = ElemOf<DT_OUT>;
  const long total = (long)rows * cols;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / cols, c = i - r * cols;
    EO::st((typename EO::type*)out + r * ld_out + c, EI::ld((const typename EI::type*)in + r * ld_in + c));
  }
}

inline int grid_for(long total, int block) {
  long g = (total + block - 1) / block;
  return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" {

int drn_resize_bilinear_u8(const void* src_hwc, int H, int W, int C, float* dst_chw, int Ho, int Wo, const int* xbounds,
                           const int* xcoef, int ksx, const int* ybounds, const int* ycoef, int ksy, int flip, void* stream) {
  if (!src_hwc || !dst_chw || H <= 0 || W <= 0 || C < 1 || C > 4 || Ho <= 0 || Wo <= 0) return DRN_ERR_ARG;
  if ((xbounds && (!xcoef || ksx < 1)) || (ybounds && (!ycoef || ksy < 1))) return DRN_ERR_ARG;
  if ((!xbounds && Wo != W) || (!ybounds && Ho != H)) return DRN_ERR_ARG;  // no pass in a direction: the size stays
  const long total = (long)Ho * Wo;
  hipLaunchKernelGGL(resize_u8_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)src_hwc, H, W, C, dst_chw, Ho, Wo, xbounds, xcoef, ksx, ybounds, ycoef, ksy, flip);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_preprocess_nhwc(const float* img_chw, int C, int H, int W, void* out_nhwc, int Hp, int Wp, int Cp,
                        const float* mean3, const float* std3, int dtype, void* stream) {
  if (!img_chw || !out_nhwc || C > 3 || C < 1 || Cp < C || H > Hp || W > Wp) return DRN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)Hp * Wp * Cp;
  if (dtype == DRN_BF16)
    hipLaunchKernelGGL(preprocess_kernel<DRN_BF16>, dim3(grid_for(total, 256)), dim3(256), 0, st, img_chw, C, H, W,
                       (bf16_t*)out_nhwc, Hp, Wp, Cp, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
  else if (dtype == DRN_F32)
    hipLaunchKernelGGL(preprocess_kernel<DRN_F32>, dim3(grid_for(total, 256)), dim3(256), 0, st, img_chw, C, H, W,
                       (float*)out_nhwc, Hp, Wp, Cp, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
  else
    return DRN_ERR_ARG;
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_maxpool2x2_nhwc(const void* x, void* y, int Nb, int H, int W, int C, int stride, int dtype, void* stream) {
  if (!x || !y || (stride != 1 && stride != 2) || H < 2 || W < 2) return DRN_ERR_ARG;
  const int es = drn_esize(dtype);
  if ((C * es) % 16) return DRN_ERR_ARG;
  const int Ho = (H - 2) / stride + 1, Wo = (W - 2) / stride + 1;
  const long total = (long)Nb * Ho * Wo * (C * es / 16);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DRN_BF16)
    hipLaunchKernelGGL(maxpool2x2_kernel<DRN_BF16>, dim3(grid_for(total, 256)), dim3(256), 0, st, (const char*)x,
                       (char*)y, Nb, H, W, C, Ho, Wo, stride);
  else if (dtype == DRN_F32)
    hipLaunchKernelGGL(maxpool2x2_kernel<DRN_F32>, dim3(grid_for(total, 256)), dim3(256), 0, st, (const char*)x,
                       (char*)y, Nb, H, W, C, Ho, Wo, stride);
  else if (dtype == DRN_FP8)
    hipLaunchKernelGGL(maxpool2x2_kernel<DRN_FP8>, dim3(grid_for(total, 256)), dim3(256), 0, st, (const char*)x,
                       (char*)y, Nb, H, W, C, Ho, Wo, stride);
  else
    return DRN_ERR_ARG;
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_maxpool3x3s2_nhwc(const void* x, void* y, int Nb, int H, int W, int C, int dtype, void* stream) {
  if (!x || !y || Nb < 1 || H < 1 || W < 1 || C < 1) return DRN_ERR_ARG;
  if (dtype != DRN_BF16 && dtype != DRN_F32 && dtype != DRN_FP8) return DRN_ERR_ARG;
  const int es = drn_esize(dtype);
  if ((C * es) % 16) return DRN_ERR_ARG;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;  // (H + 2 * 1 - 3) / 2 + 1
  const long total = (long)Nb * Ho * Wo * (C * es / 16);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DRN_BF16)
    hipLaunchKernelGGL(maxpool3x3s2_kernel<DRN_BF16>, dim3(grid_for(total, 256)), dim3(256), 0, st, (const char*)x,
                       (char*)y, Nb, H, W, C, Ho, Wo);
  else if (dtype == DRN_F32)
    hipLaunchKernelGGL(maxpool3x3s2_kernel<DRN_F32>, dim3(grid_for(total, 256)), dim3(256), 0, st, (const char*)x,
                       (char*)y, Nb, H, W, C, Ho, Wo);
  else
    hipLaunchKernelGGL(maxpool3x3s2_kernel<DRN_FP8>, dim3(grid_for(total, 256)), dim3(256), 0, st, (const char*)x,
                       (char*)y, Nb, H, W, C, Ho, Wo);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_im2col_t(const void* x, void* out, int Nb, int H, int W, int Cin, int ldc, int KH, int KW, int stride, int pad,
                 int dil, long ld_out, int dtype, void* stream) {
  if (!x || !out || Nb < 1 || Cin < 1 || ldc < Cin || KH < 1 || KW < 1 || stride < 1 || dil < 1) return DRN_ERR_ARG;
  const int Ho = (H + 2 * pad - dil * (KH - 1) - 1) / stride + 1, Wo = (W + 2 * pad - dil * (KW - 1) - 1) / stride + 1;
  if (Ho < 1 || Wo < 1 || ld_out < (long)Nb * Ho * Wo) return DRN_ERR_ARG;
  dim3 grid((Nb * Ho * Wo + 63) / 64, (Cin + 63) / 64, KH * KW), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DRN_BF16)
    hipLaunchKernelGGL(im2col_t_kernel<DRN_BF16>, grid, block, 0, st, (const char*)x, (char*)out, Nb, H, W, Cin, ldc, KH,
                       KW, stride, pad, dil, Ho, Wo, ld_out);
  else if (dtype == DRN_F32)
    hipLaunchKernelGGL(im2col_t_kernel<DRN_F32>, grid, block, 0, st, (const char*)x, (char*)out, Nb, H, W, Cin, ldc, KH,
                       KW, stride, pad, dil, Ho, Wo, ld_out);
  else
    return DRN_ERR_ARG;
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_maxpool2x2_bwd_nhwc(const void* x, const void* dy, void* dx, int Nb, int H, int W, int C, int stride, int dtype,
                            void* stream) {
  if (!x || !dy || !dx || (stride != 1 && stride != 2) || H < 2 || W < 2) return DRN_ERR_ARG;
  const int Ho = (H - 2) / stride + 1, Wo = (W - 2) / stride + 1;
  const long total = (long)Nb * H * W * C;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DRN_BF16)
    hipLaunchKernelGGL(maxpool2x2_bwd_kernel<DRN_BF16>, dim3(grid_for(total, 256)), dim3(256), 0, st, (const char*)x,
                       (const char*)dy, (char*)dx, Nb, H, W, C, Ho, Wo, stride);
  else if (dtype == DRN_F32)
    hipLaunchKernelGGL(maxpool2x2_bwd_kernel<DRN_F32>, dim3(grid_for(total, 256)), dim3(256), 0, st, (const char*)x,
                       (const char*)dy, (char*)dx, Nb, H, W, C, Ho, Wo, stride);
  else
    return DRN_ERR_ARG;
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// props[M][4] <- rois[M][1:5] and (optional) words_dst[n_words] <- words_src: the two hand-overs from the staged next
// batch to the buffers the heads read (proposal boxes for pseudo-GT mining / IoU labelling; the image-level label block),
// in ONE launch in front of the pooling kernel.  See include/drn_wsod.h.
__global__ void stage_rois_kernel(const float* __restrict__ boxes, const float* __restrict__ logits, float batch_index,
                                  float* __restrict__ rois, float* __restrict__ obj, float* __restrict__ props, int M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const float x0 = boxes[4 * (long)i], y0 = boxes[4 * (long)i + 1], x1 = boxes[4 * (long)i + 2], y1 = boxes[4 * (long)i + 3];
  float* r = rois + 5 * (long)i;
  r[0] = batch_index; r[1] = x0; r[2] = y0; r[3] = x1; r[4] = y1;
  if (props) { float* q = props + 4 * (long)i; q[0] = x0; q[1] = y0; q[2] = x1; q[3] = y1; }
  if (obj) obj[i] = logits[i];
}

__global__ void stage_heads_kernel(const float* __restrict__ rois, float* __restrict__ props, int M,
                                   const int* __restrict__ words_src, int* __restrict__ words_dst, int n_words) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M * 4) props[i] = rois[(i >> 2) * 5 + 1 + (i & 3)];
  if (i < n_words) words_dst[i] = words_src[i];
}

int drn_stage_heads_inputs(const float* rois, float* props, int M, const int* words_src, int* words_dst, int n_words,
                           void* stream) {
  if (M < 0 || n_words < 0 || (M > 0 && (!rois || !props)) || (n_words > 0 && (!words_src || !words_dst))) return DRN_ERR_ARG;
  const long n = (long)M * 4 > n_words ? (long)M * 4 : n_words;
  if (n == 0) return DRN_OK;
  hipLaunchKernelGGL(stage_heads_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, rois, props, M,
                     words_src, words_dst, n_words);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// boxes [M][4] + objectness logits [M] of ONE image -> the pooler's rois [M][5] = (batch index, x0, y0, x1, y1)
// (convert_boxes_to_pooler_format, detectron2/modeling/poolers.py:69-96), a contiguous copy of the logits and of the boxes:
// one launch for what was torch.full + two torch.cat + two copies in front of every forward
int drn_stage_rois(const float* boxes, const float* logits, float batch_index, float* rois, float* obj, float* props, int M,
                   void* stream) {
  if (M < 0 || (M > 0 && (!boxes || !rois))) return DRN_ERR_ARG;
  if ((obj != nullptr) != (logits != nullptr)) return DRN_ERR_ARG;
  if (M == 0) return DRN_OK;
  hipLaunchKernelGGL(stage_rois_kernel, dim3(grid_for(M, 256)), dim3(256), 0, (hipStream_t)stream, boxes, logits, batch_index,
                     rois, obj, props, M);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_add(const void* a, const void* b, void* out, long n, int dtype, void* stream) {
  if (!a || !b || !out || n < 0) return DRN_ERR_ARG;
  if (n == 0) return DRN_OK;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DRN_BF16)
    hipLaunchKernelGGL(add_kernel<DRN_BF16>, dim3(grid_for(n, 256)), dim3(256), 0, st, (const char*)a, (const char*)b, (char*)out, n);
  else if (dtype == DRN_F32)
    hipLaunchKernelGGL(add_kernel<DRN_F32>, dim3(grid_for(n, 256)), dim3(256), 0, st, (const char*)a, (const char*)b, (char*)out, n);
  else
    return DRN_ERR_ARG;
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_transpose2d(const void* in, void* out, int rows, int cols, long ld_in, long ld_out, int in_dtype,
                    int out_dtype, void* stream) {
  if (!in || !out || rows < 0 || cols < 0) return DRN_ERR_ARG;
  if (rows == 0 || cols == 0) return DRN_OK;
  dim3 grid((cols + 63) / 64, (rows + 63) / 64), block(256);
  hipStream_t st = (hipStream_t)stream;
#define TR_LAUNCH(DI, DO) hipLaunchKernelGGL((transpose_kernel<DI, DO>), grid, block, 0, st, (const char*)in, (char*)out, rows, cols, ld_in, ld_out)
  if (in_dtype == DRN_BF16 && out_dtype == DRN_BF16 && (ld_in % 8) == 0 && (ld_out % 8) == 0 &&
      ((((uintptr_t)in) | ((uintptr_t)out)) & 15) == 0)
    hipLaunchKernelGGL(transpose_bf16_kernel, grid, block, 0, st, (const bf16_t*)in, (bf16_t*)out, rows, cols, ld_in, ld_out);
  else if (in_dtype == DRN_BF16 && out_dtype == DRN_BF16) TR_LAUNCH(DRN_BF16, DRN_BF16);
  else if (in_dtype == DRN_F32 && out_dtype == DRN_F32) TR_LAUNCH(DRN_F32, DRN_F32);
  else if (in_dtype == DRN_F32 && out_dtype == DRN_BF16) TR_LAUNCH(DRN_F32, DRN_BF16);
  else if (in_dtype == DRN_BF16 && out_dtype == DRN_F32) TR_LAUNCH(DRN_BF16, DRN_F32);
  else return DRN_ERR_ARG;
#undef TR_LAUNCH
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// out[r][c] = cast(in[r][c]) with independent leading dimensions (refreshes padded compute shadows).
int drn_cast2d(const void* in, void* out, int rows, int cols, long ld_in, long ld_out, int in_dtype, int out_dtype,
               void* stream) {
  if (!in || !out || rows < 0 || cols < 0) return DRN_ERR_ARG;
  if (rows == 0 || cols == 0) return DRN_OK;
  const long total = (long)rows * cols;
  dim3 grid(grid_for(total, 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define CA_LAUNCH(DI, DO) hipLaunchKernelGGL((cast2d_kernel<DI, DO>), grid, block, 0, st, (const char*)in, (char*)out, rows, cols, ld_in, ld_out)
  if (in_dtype == DRN_BF16 && out_dtype == DRN_BF16) CA_LAUNCH(DRN_BF16, DRN_BF16);
  else if (in_dtype == DRN_F32 && out_dtype == DRN_F32) CA_LAUNCH(DRN_F32, DRN_F32);
  else if (in_dtype == DRN_F32 && out_dtype == DRN_BF16) CA_LAUNCH(DRN_F32, DRN_BF16);
  else if (in_dtype == DRN_BF16 && out_dtype == DRN_F32) CA_LAUNCH(DRN_BF16, DRN_F32);
  else return DRN_ERR_ARG;
#undef CA_LAUNCH
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // extern "C"
