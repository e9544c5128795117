// The standard ResNet stem as ONE launch (detectron2/modeling/backbone/resnet.py:355-359, BasicStem.forward):
//   conv 7x7 / stride 2 / pad 3 (3 channels stored as 8, bf16) -> folded FrozenBN -> ReLU -> max_pool2d(3, 2, 1).
// As two launches the 64-channel map at half resolution is written and read back (800 x 1216: 31 MB each way) to produce a
// quarter-resolution one (7.8 MB).  Here a workgroup owns a 7 x 8 block of POOLED pixels of one image: the 15 x 17 conv
// pixels under it (rows 2 py - 1 .. 2 py + 1: one conv row / column is shared with - and recomputed by - the neighbouring
// block, 255 conv pixels for 224 owned) are multiplied out of an LDS-resident 35 x 39-pixel input patch (16 bytes = one
// tap per pixel) against ALL weights (64 x 49 taps, resident for the workgroup's life: the launch is persistent), rounded
// to bf16 into LDS exactly as drn_conv2d_nhwc would store them, and pooled from there.  The conv map never leaves the chip.
//
// Same arithmetic as the two launches, bit for bit: the tiled conv kernels (conv.hip on mfma_mainloop.h: mainloop + mma_step) give an
// output element ONE fp32 accumulator that takes v_mfma_f32_32x32x16_bf16 steps over k = (kh, kw, ci) ascending, 16 k-values
// = two taps per step (lanes 0-31 the even tap, lanes 32-63 the odd one); this kernel issues the same steps in the same
// order (the all-zero padding steps of the 448-value rows add +0 and are skipped), the same `acc * scale + bias`, ReLU and
// bf16 rounding, and the pool takes its maxima in drn_maxpool3x3s2_nhwc's order (rows, then columns, padding skipped).
// Built WITHOUT -ffp-contract=off, like conv.hip: the affine contracts to the same fma there and here.
#include "drn_common.h"
#include "../../include/drn_wsod.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

constexpr int ST_PH = 7, ST_PW = 8;                        // pooled pixels per block
constexpr int ST_CH = 2 * ST_PH + 1, ST_CW = 2 * ST_PW + 1;  // 15 x 17 conv pixels under them (255 <= 4 waves x 64 rows)
constexpr int ST_IH = 2 * ST_CH + 5, ST_IW = 2 * ST_CW + 5;  // 35 x 39 input pixels under those (7x7 taps, stride 2)
constexpr int ST_TAPS = 49, ST_STEPS = 25;                 // 16 k-values (two taps of 8 stored channels) per MFMA step
constexpr int ST_WCH = 2 * ST_STEPS;                       // 16-byte chunks of a weight row that are read (tap 49 = zeros)
constexpr int ST_WROW = 912;                               // LDS pitch of a weight row: 57 chunks - ds_read_b128 of 16 rows hits 16 slots
constexpr int ST_WTS = 64 * ST_WROW, ST_PATCH = ST_IH * ST_IW * 16, ST_CONV = 256 * 128;
constexpr int ST_LDS = ST_WTS + ST_PATCH + ST_CONV;        // 112,976 bytes of the 160 KB
constexpr int ST_NPX = ST_IH * ST_IW, ST_NIT = (ST_NPX + 255) / 256;  // patch pixels, per-thread share (6)
static_assert(ST_CH * ST_CW <= 256 && ST_PATCH % 16 == 0 && ST_WTS % 16 == 0, "tile geometry");

struct StemParams {
  const char* X;       // [Nb][H][W][8] bf16
  const char* Wt;      // [64][ldw] bf16, k = (kh * 7 + kw) * 8 + ci
  const float* scale;  // [64] or null
  const float* bias;
  char* Y;             // [Nb][Hp][Wp][64] bf16
  int Nb, H, W, Ho, Wo, Hp, Wp;
  long ldw;
  int tiles_y, tiles_x;
};

__device__ __forceinline__ void stem_fetch(const StemParams& p, int t, int tid, i32x4_t (&r)[ST_NIT]) {
  const int per = p.tiles_y * p.tiles_x;
  const int n = t / per, rem = t - n * per;
  const int ty = rem / p.tiles_x, tx = rem - ty * p.tiles_x;
  const int iy0 = 2 * (2 * ty * ST_PH - 1) - 3, ix0 = 2 * (2 * tx * ST_PW - 1) - 3;
#pragma unroll
  for (int q = 0; q < ST_NIT; ++q) {
    const int c = tid + 256 * q;
    const int rr = c / ST_IW, cc = c - rr * ST_IW;
    const int iy = iy0 + rr, ix = ix0 + cc;
    const bool ok = c < ST_NPX && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
    // (a clamped address + select instead of a branch: the loads of one thread stay in flight together)
    const long off = ok ? (((long)n * p.H + iy) * p.W + ix) * 16 : 0;
    const i32x4_t v = *(const i32x4_t*)(p.X + off);
    const i32x4_t z = {0, 0, 0, 0};
    r[q] = ok ? v : z;
  }
}

__global__ __launch_bounds__(256) void stem7x7_pool_kernel(StemParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* wts = smem;
  char* patch = smem + ST_WTS;
  char* convt = patch + ST_PATCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  const int ntiles = p.Nb * p.tiles_y * p.tiles_x;
  int t = blockIdx.x;
  if (t >= ntiles) return;
  i32x4_t pre[ST_NIT];
  stem_fetch(p, t, tid, pre);
  for (int c = tid; c < 64 * ST_WCH; c += 256) {
    const int row = c / ST_WCH, ch = c - row * ST_WCH;
    *(i32x4_t*)(wts + row * ST_WROW + ch * 16) = *(const i32x4_t*)(p.Wt + (long)row * p.ldw * 2 + ch * 16);
  }
  // this lane's A rows (conv pixels of the block, row-major over 15 x 17; row 255 repeats 254 and is dropped) and B rows
  int abase[2], bbase[2];
  float sc[2], bi[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int m = wave * 64 + i * 32 + l31;
    m = m < ST_CH * ST_CW ? m : ST_CH * ST_CW - 1;
    const int ty = m / ST_CW, tx = m - ty * ST_CW;
    abase[i] = ((2 * ty) * ST_IW + 2 * tx) * 16;
    const int n = i * 32 + l31;
    bbase[i] = n * ST_WROW + half * 16;
    sc[i] = p.scale ? p.scale[n] : 1.f;
    bi[i] = p.bias ? p.bias[n] : 0.f;
  }
  for (; t < ntiles; t += gridDim.x) {
    const int per = p.tiles_y * p.tiles_x;
    const int n = t / per, rem = t - n * per;
    const int tyi = rem / p.tiles_x, txi = rem - tyi * p.tiles_x;
    const int py0 = tyi * ST_PH, px0 = txi * ST_PW;
#pragma unroll
    for (int q = 0; q < ST_NIT; ++q)
      if (tid + 256 * q < ST_NPX) *(i32x4_t*)(patch + (tid + 256 * q) * 16) = pre[q];
    __syncthreads();  // patch (and, the first time, the weights) in LDS; everybody is past the previous block's pooling
    if (t + (int)gridDim.x < ntiles) stem_fetch(p, t + gridDim.x, tid, pre);  // the next block's patch, under this one's MFMAs
    f32x16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
    for (int s = 0; s < ST_STEPS; ++s) {
      constexpr int LAST = ST_TAPS - 1;
      const int t0 = 2 * s, t1 = 2 * s + 1 < ST_TAPS ? 2 * s + 1 : LAST;  // (tap 49: zero weights; any finite A will do)
      const int o0 = ((t0 / 7) * ST_IW + t0 % 7) * 16, o1 = ((t1 / 7) * ST_IW + t1 % 7) * 16;
      const int toff = half ? o1 : o0;
      i32x4_t fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = *(const i32x4_t*)(patch + abase[i] + toff);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = *(const i32x4_t*)(wts + bbase[j] + s * 32);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, fa[i]),
                                                              __builtin_bit_cast(bf16x8_t, fb[j]), acc[i][j], 0, 0, 0);
    }
    // affine + ReLU + bf16 rounding (conv_epilogue of conv.hip), into the conv tile [pixel][64 channels]
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nl = j * 32 + l31;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = wave * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          float v = acc[i][j][r] * sc[j] + bi[j];
          v = fmaxf(v, 0.f);
          if (m < ST_CH * ST_CW) *(bf16_t*)(convt + m * 128 + nl * 2) = f32_to_bf16(v);
        }
    }
    __syncthreads();
    // max_pool2d(3, 2, 1) over the tile: one task = one 16-byte channel vector of one pooled pixel (drn_maxpool3x3s2_nhwc's
    // arithmetic and order; conv pixels outside the conv map are the padding and are skipped)
    for (int task = tid; task < ST_PH * ST_PW * 8; task += 256) {
      const int pp = task >> 3, c8 = task & 7;
      const int py = pp / ST_PW, px = pp - py * ST_PW;
      const int gy = py0 + py, gx = px0 + px;
      if (gy >= p.Hp || gx >= p.Wp) continue;
      float lo[4], hi[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) lo[k] = hi[k] = -INFINITY;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int cy = 2 * gy - 1 + dy;
        if (cy < 0 || cy >= p.Ho) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int cx = 2 * gx - 1 + dx;
          if (cx < 0 || cx >= p.Wo) continue;
          const u32x4_t a = *(const u32x4_t*)(convt + ((2 * py + dy) * ST_CW + 2 * px + dx) * 128 + c8 * 16);
          const unsigned u[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            lo[k] = fmaxf(lo[k], __builtin_bit_cast(float, u[k] << 16));
            hi[k] = fmaxf(hi[k], __builtin_bit_cast(float, u[k] & 0xffff0000u));
          }
        }
      }
      u32x4_t o;
      o.x = (__builtin_bit_cast(unsigned, lo[0]) >> 16) | (__builtin_bit_cast(unsigned, hi[0]) & 0xffff0000u);
      o.y = (__builtin_bit_cast(unsigned, lo[1]) >> 16) | (__builtin_bit_cast(unsigned, hi[1]) & 0xffff0000u);
      o.z = (__builtin_bit_cast(unsigned, lo[2]) >> 16) | (__builtin_bit_cast(unsigned, hi[2]) & 0xffff0000u);
      o.w = (__builtin_bit_cast(unsigned, lo[3]) >> 16) | (__builtin_bit_cast(unsigned, hi[3]) & 0xffff0000u);
      *(u32x4_t*)(p.Y + ((((long)n * p.Hp + gy) * p.Wp + gx) * 64 + c8 * 8) * 2) = o;
    }
  }
}

}  // namespace

extern "C" int drn_stem7x7_pool_nhwc(const void* x, const void* w, const float* scale, const float* bias, void* y, int Nb,
                                     int H, int W, int Cin, int Cout, long ldw, int relu, int dtype, void* stream) {
  if (!x || !w || !y || Nb < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return DRN_ERR_ARG;
  // the class: bf16, 3 channels stored as 8, 64 output channels, the ReLU in front of the pool (the pool's padding is then
  // "skip", and every shipped stem has it), 16-byte aligned operands
  if (dtype != DRN_BF16 || Cin != 8 || Cout != 64 || !relu || ldw < ST_WCH * 8 || (ldw * 2) % 16 != 0 ||
      ((((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)y)) & 15) != 0)
    return DRN_ERR_UNSUPPORTED;
  StemParams p;
  p.X = (const char*)x; p.Wt = (const char*)w; p.scale = scale; p.bias = bias; p.Y = (char*)y;
  p.Nb = Nb; p.H = H; p.W = W;
  p.Ho = (H + 6 - 7) / 2 + 1; p.Wo = (W + 6 - 7) / 2 + 1;
  p.Hp = (p.Ho + 2 - 3) / 2 + 1; p.Wp = (p.Wo + 2 - 3) / 2 + 1;
  p.ldw = ldw;
  p.tiles_y = (p.Hp + ST_PH - 1) / ST_PH; p.tiles_x = (p.Wp + ST_PW - 1) / ST_PW;
  const long ntiles = (long)Nb * p.tiles_y * p.tiles_x;
  if (ntiles > 0x7fffffffL) return DRN_ERR_UNSUPPORTED;
  if (!drn_launch::allow_lds((const void*)stem7x7_pool_kernel, ST_LDS)) return DRN_ERR_LAUNCH;
  const int grid = (int)(ntiles < drn_launch::cu_count() ? ntiles : drn_launch::cu_count());
  hipLaunchKernelGGL(stem7x7_pool_kernel, dim3(grid), dim3(256), ST_LDS, (hipStream_t)stream, p);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}
