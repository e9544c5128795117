// Implicit-GEMM NHWC convolution for gfx950: the tiled kernels on the mainloops of mfma_mainloop.h, the LDS-resident 3x3 /
// 64-channel kernel, the forward plan (conv_fwd_plan) and the entry points.
//
// Replaces on the reference path: F.conv2d + FrozenBatchNorm2d + relu_ + residual add (detectron2/layers/wrappers.py:94-99,
// detectron2/layers/batch_norm.py:45-65, projects/WSL/wsl/modeling/backbone/resnet_ws.py:217-237).
#include "mfma_mainloop.h"
#include "conv_launch.h"
#include "../../include/drn_wsod.h"

namespace {

using drn_conv::ConvParams;
using drn_launch::cu_count;

// im2col-on-the-fly operand of an NHWC convolution: row = output pixel, k = (kh, kw, ci).  Branch-free: every lane
// issues a bounds-checked buffer load, and lanes that fall into the zero padding, beyond the last tap or beyond M
// use an offset past the descriptor's range, for which the hardware returns zeros.  (Conditional global loads made
// the compiler drain each one before leaving its branch, so a slab cost a full memory latency whatever the prefetch
// depth: 0.85 us per slab on the res4 3x3 convs.)
template <int DT, int ROWS>
struct ConvLoader {
  static constexpr int ES = EsOf<DT>::value;
  static constexpr unsigned OOB = 0xFFFFFFF0u;
  __amdgpu_buffer_rsrc_t rsrc;  // whole input tensor (launcher guarantees < 4 GB - 16)
  int H, W, Cin, KW, dil, ntaps;
  int hi0[ROWS / 32], wi0[ROWS / 32];
  unsigned nbase[ROWS / 32];  // byte offset of image n, or OOB for rows beyond M
  // (tap, channel) of this lane's 16-byte chunk in slab `at`: the mainloop asks for consecutive slabs, so the position is
  // advanced by one slab (128 bytes of k) instead of being re-derived with two integer divisions per slab - ~80 VALU
  // instructions that sat on the critical path of the latency-bound small-map layers
  int at = -1, tap = 0, ci = 0, kh = 0, kw = 0;
  __device__ __forceinline__ void seek(int slab, int tid) {
    const int k = (slab * 128 + (tid & 7) * 16) / ES;
    tap = k / Cin; ci = k - tap * Cin;
    kh = tap / KW; kw = tap - kh * KW;
    at = slab;
  }
  template <int R>
  __device__ __forceinline__ void load(i32x4_t (&r)[R / 32], int slab, int tid) {
    static_assert(R == ROWS, "tile rows");
    if (slab != at) seek(slab, tid);
    else if (Cin * ES < 128) seek(slab, tid);  // several taps per slab (the 3-channel stem): no single-step advance
#pragma unroll
    for (int p = 0; p < ROWS / 32; ++p) {
      const int hi = hi0[p] + kh * dil, wi = wi0[p] + kw * dil;
      const bool ok = nbase[p] != OOB && tap < ntaps && hi >= 0 && hi < H && wi >= 0 && wi < W;
      const unsigned off = ok ? nbase[p] + (unsigned)(((hi * W + wi) * Cin + ci) * ES) : OOB;
      r[p] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
    }
    ci += 128 / ES;  // next slab (exact when Cin * ES >= 128: at most one tap boundary per slab; otherwise re-sought)
    if (ci >= Cin) {
      ci -= Cin;
      ++tap;
      if (++kw == KW) { kw = 0; ++kh; }
    }
    at = slab + 1;
  }
};

// ------------------------------------------------------------------------------------------------
// 1x1 convolution (stride 1, no padding) of a LARGE map as a GEMM on the 256x256 ping-pong mainloop (round 5): the bf16
// bottleneck 1x1s of the shipped dilated-C5 trunk at a real image size are [15000 x Cin] . [Cout x Cin]^T with Cout = 1024 /
// 2048 - 236 / 472 tiles of 256 x 256 - and ran at 300-640 TFLOP/s on the 128x128 register-staged tile (profiles/r5_12_*).
// A = the NHWC input itself (row = pixel), B = the packed weights; the epilogue is the conv's: per-channel affine (folded
// FrozenBN), shortcut add, ReLU, bf16 store.  The accumulators leave through LDS as fp32, one 128-row half of the tile (128 KB
// = both operand stages, free behind the mainloop) at a time, 16-byte chunk c of row r at c ^ (r & 15): a lane then owns 4
// consecutive channels of one pixel, a wave instruction one whole 512-byte row - 8-byte shortcut loads and 8-byte stores of
// complete rows instead of the MFMA layout's 32 rows x 16 bytes per instruction.
// Same slab order, k-steps and MFMA per output element as the tiled conv kernels: bit-identical to them.
__global__ __launch_bounds__(512) void conv1x1_pp_kernel(ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int Mtot = p.Nb * p.Ho * p.Wo;
  const int tiles_m = (Mtot + 255) / 256, tiles_n = (p.Cout + 255) / 256;
  int tm, tn;
  tile_coords(xcd_remap(blockIdx.x, tiles_m * tiles_n), tiles_m, tiles_n, tm, tn, 4);
  const int bm = tm * 256, bn = tn * 256;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const RowLoader la = make_row_loader(p.X, bm, Mtot, 256, (long)p.Cin * 2);
  const RowLoader lb = make_row_loader(p.Wt, bn, p.Cout, 256, p.ldw * 2);
  unsigned pva[4], pvb[4];
  pp_offsets<false>(la.ld_bytes, lb.ld_bytes, tid, pva, pvb);
  f32x16_t acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int nslab = p.Cin >> 6;
  pp_issue_first(smem, la.rsrc, lb.rsrc, pva, pvb, wave, 0);
  pp_mainloop<DRN_BF16, 1>(acc, smem, la.rsrc, lb.rsrc, pva, pvb, 0, nslab, lane, wave);
  // D^T layout: lane -> m (A row) = lane & 31, register r -> n = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
  const int l31 = lane & 31, hi = lane >> 5;
  float* tile = (float*)smem;  // [128][256] fp32, 16-byte chunks XOR-swizzled with the row
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  const int nn = bn + lane * 4;  // this lane's 4 channels in the read-back phase
  const bool col_ok = nn < p.Cout;
  f32x4_t sc = {1.f, 1.f, 1.f, 1.f}, bi = {0.f, 0.f, 0.f, 0.f};
  if (col_ok && p.scale) sc = *(const f32x4_t*)(p.scale + nn);
  if (col_ok && p.bias) bi = *(const f32x4_t*)(p.bias + nn);
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    __syncthreads();  // every wave is done with the operand stages / with the previous half
    // shortcut rows of this half, fetched ahead of the staging: wave w owns rows w, w + 8, ... of the half
    u32x2_t rv[16];
    if (p.residual && col_ok) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = bm + half * 128 + q * 8 + wave;
        rv[q] = *(const u32x2_t*)(p.residual + ((long)(m < Mtot ? m : Mtot - 1) * p.ldres + nn) * 2);
      }
    }
    if (wm == half) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = i * 32 + l31;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = wn * 16 + j * 8 + 2 * q + hi;  // 16-byte chunk = 4 channels
            const f32x4_t v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
            *(f32x4_t*)(tile + row * 256 + ((c ^ (row & 15)) << 2)) = v;
          }
      }
    }
    __syncthreads();
    if (col_ok) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = q * 8 + wave, m = bm + half * 128 + row;
        if (m >= Mtot) break;
        const f32x4_t a = *(const f32x4_t*)(tile + row * 256 + ((lane ^ (row & 15)) << 2));
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = a[e] * sc[e] + bi[e];
        if (p.residual) {
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            v[2 * e] += __builtin_bit_cast(float, rv[q][e] << 16) * p.res_mult;
            v[2 * e + 1] += __builtin_bit_cast(float, rv[q][e] & 0xffff0000u) * p.res_mult;
          }
        }
        if (p.relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        u32x2_t o;
        o.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
        o.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
        *(u32x2_t*)(p.Y + ((long)m * p.ldy + nn) * 2) = o;
      }
    }
  }
}


// Epilogue of the tiled conv kernels: per-channel affine (+ residual, ReLU) and the store.  `tid` = 0..255 within the
// four waves that own the accumulators; `active` = false for waves that only take part in the barriers (the second
// K-group of conv_nhwc_k2_kernel, whose partial sums were already added in).
// 8 consecutive channels of one pixel, packed: bf16 = 16 bytes, fp8 = 8 bytes (the vector epilogues below)
__device__ __forceinline__ bool vec8_ok(int dt, const void* ptr, long ld) {
  return dt == DRN_BF16 ? ((ld & 7) == 0 && (((uintptr_t)ptr) & 15) == 0)
                        : dt == DRN_FP8 ? ((ld & 7) == 0 && (((uintptr_t)ptr) & 7) == 0) : false;
}
__device__ __forceinline__ i32x4_t load8(int dt, const char* base, long elem) {
  if (dt == DRN_BF16) return *(const i32x4_t*)(base + elem * 2);
  const uint2 v = *(const uint2*)(base + elem);
  return i32x4_t{(int)v.x, (int)v.y, 0, 0};
}
__device__ __forceinline__ void add8(int dt, const i32x4_t& rv, float mult, float (&v)[8]) {
  if (dt == DRN_BF16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t w = (uint32_t)rv[e];
      v[2 * e] += __builtin_bit_cast(float, w << 16) * mult;
      v[2 * e + 1] += __builtin_bit_cast(float, w & 0xffff0000u) * mult;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      v[4 * e] += __builtin_amdgcn_cvt_f32_fp8(rv[e], 0) * mult;
      v[4 * e + 1] += __builtin_amdgcn_cvt_f32_fp8(rv[e], 1) * mult;
      v[4 * e + 2] += __builtin_amdgcn_cvt_f32_fp8(rv[e], 2) * mult;
      v[4 * e + 3] += __builtin_amdgcn_cvt_f32_fp8(rv[e], 3) * mult;
    }
  }
}
__device__ __forceinline__ void store8(int dt, char* base, long elem, const float (&v)[8]) {
  if (dt == DRN_BF16) {
    i32x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (int)((uint32_t)f32_to_bf16(v[2 * e]) | ((uint32_t)f32_to_bf16(v[2 * e + 1]) << 16));
    *(i32x4_t*)(base + elem * 2) = o;
  } else {  // saturating RNE like f32_to_fp8, two values per v_cvt_pk_fp8_f32
    float c[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) c[e] = fminf(fmaxf(v[e], -448.f), 448.f);
    uint2 o;
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], 0, false);
    o.x = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], w, true);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c[4], c[5], 0, false);
    o.y = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c[6], c[7], w, true);
    *(uint2*)(base + elem) = o;
  }
}

template <int DT, int BM, int BN>
__device__ __forceinline__ void conv_epilogue(const ConvParams& p, f32x16_t (&acc)[BM / 64][BN / 64], char* smem, int bm,
                                              int bn, int Mtot, int tid, bool active) {
  constexpr int MI = BM / 64, NJ = BN / 64;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // bf16 output (+ bf16 residual): the affine result goes through LDS as fp32 [BM][BN] (exactly the mainloop's LDS, now
  // free) so that every lane then owns 8 consecutive channels of a pixel - 16-byte residual loads and 16-byte stores,
  // whole 128/256-byte row segments per instruction.  The MFMA layout gives a lane ONE channel of 16 * MI pixels: written
  // straight from the accumulators that is 2-byte accesses, which ran the write-heavy 1x1 convs of large maps at
  // ~1 TB/s (res2 conv3 at 200 x 304: 72 us for 70 MB; tools/conv_bench.py).  Same arithmetic, same rounding.
  // (round 3: fp8 outputs / residuals take the same path with 8-byte accesses - written from the accumulators an fp8
  // layer stores single BYTES)
  const bool vec_epi = (p.Cout & 7) == 0 && vec8_ok(p.out_dt, p.Y, p.ldy) &&
                       (!p.residual || vec8_ok(p.res_dt, p.residual, p.ldres));
  if (vec_epi) {
    float* tile = (float*)smem;
    __syncthreads();  // the last slab's LDS reads are done
    if (active) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int nl = wn * (BN / 2) + j * 32 + (lane & 31), n = bn + nl;
        const float sc = (n < p.Cout && p.scale) ? p.scale[n] : 1.f;
        const float bi = (n < p.Cout && p.bias) ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ml = wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            tile[ml * BN + nl] = acc[i][j][r] * sc + bi;
          }
      }
    }
    __syncthreads();
    if (!active) return;
    constexpr int LPR = BN / 8, RPP = 256 / LPR, NR = BM / RPP;  // lanes per row, rows per pass, rows per lane
    const int cl = tid % LPR, rl = tid / LPR;
    const int n = bn + cl * 8;
    if (n >= p.Cout) return;
    i32x4_t rv[NR];
    if (p.residual) {
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        const int m = bm + rl + q * RPP;
        rv[q] = load8(p.res_dt, p.residual, (long)(m < Mtot ? m : Mtot - 1) * p.ldres + n);
      }
    }
#pragma unroll
    for (int q = 0; q < NR; ++q) {
      const int ml = rl + q * RPP, m = bm + ml;
      if (m >= Mtot) break;
      const f32x4_t lo = *(const f32x4_t*)(tile + ml * BN + cl * 8), hi = *(const f32x4_t*)(tile + ml * BN + cl * 8 + 4);
      float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      if (p.residual) add8(p.res_dt, rv[q], p.res_mult, v);
      if (p.relu) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
      }
      store8(p.out_dt, p.Y, (long)m * p.ldy + n, v);
    }
    return;
  }
  if (!active) return;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int n = bn + wn * (BN / 2) + j * 32 + (lane & 31);
    if (n >= p.Cout) continue;
    const float sc = p.scale ? p.scale[n] : 1.f;
    const float bi = p.bias ? p.bias[n] : 0.f;
    // every residual value of this lane's column is fetched BEFORE the first store: Y and the residual may alias as far
    // as the compiler knows, so a load placed behind a store stays there and each of the 16 * MI row steps would pay a
    // full memory latency (measured: 36 us for the K = 256 res4 conv3 at 50 x 76, most of it here)
    float rres[MI][16];
    if (p.residual) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = bm + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          const long ri = (long)(m < Mtot ? m : Mtot - 1) * p.ldres + n;
          rres[i][r] = p.res_dt == DRN_BF16 ? bf16_to_f32(((const bf16_t*)p.residual)[ri])
                       : p.res_dt == DRN_FP8 ? fp8_to_f32(((const uint8_t*)p.residual)[ri])
                                             : ((const float*)p.residual)[ri];
        }
    }
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = bm + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < Mtot) {
          float v = acc[i][j][r] * sc + bi;
          if (p.residual) v += rres[i][r] * p.res_mult;
          if (p.relu) v = fmaxf(v, 0.f);
          const long yi = (long)m * p.ldy + n;
          if (p.out_dt == DRN_BF16) ((bf16_t*)p.Y)[yi] = f32_to_bf16(v);
          else if (p.out_dt == DRN_FP8) ((uint8_t*)p.Y)[yi] = f32_to_fp8(v);
          else ((float*)p.Y)[yi] = v;
        }
      }
  }
}

template <int DT, int BM, int BN, bool K64 = true>
__global__ __launch_bounds__(256, (DT == DRN_FP8 && K64 && BM == 128) ? 2 : 1) void conv_nhwc_kernel(ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = EsOf<DT>::value;
  constexpr int MI = BM / 64, NJ = BN / 64;
  const int Mtot = p.Nb * p.Ho * p.Wo;
  const int tiles_m = (Mtot + BM - 1) / BM, tiles_n = (p.Cout + BN - 1) / BN;
  int tm, tn;
  tile_coords(xcd_remap(blockIdx.x, tiles_m * tiles_n), tiles_m, tiles_n, tm, tn);
  const int bm = tm * BM, bn = tn * BN;
  ConvLoader<DT, BM> la;
  la.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, (unsigned)((long)p.Nb * p.H * p.W * p.Cin * ES), 0x00020000);
  la.H = p.H; la.W = p.W; la.Cin = p.Cin; la.KW = p.KW; la.dil = p.dil; la.ntaps = p.KH * p.KW;
  const int r0 = threadIdx.x >> 3;
#pragma unroll
  for (int q = 0; q < BM / 32; ++q) {
    const int m = bm + r0 + 32 * q;
    if (m < Mtot) {
      const int n = m / (p.Ho * p.Wo), rem = m - n * p.Ho * p.Wo;
      const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
      la.hi0[q] = ho * p.stride - p.pad;
      la.wi0[q] = wo * p.stride - p.pad;
      la.nbase[q] = (unsigned)((long)n * p.H * p.W * p.Cin * ES);
    } else {
      la.hi0[q] = 0; la.wi0[q] = 0; la.nbase[q] = ConvLoader<DT, BM>::OOB;
    }
  }
  const RowLoader lb = make_row_loader(p.Wt, bn, p.Cout, BN, p.ldw * ES);
  f32x16_t acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int nslab = (p.Ktot * ES + 127) / 128;
  mainloop<DT, BM, BN, decltype(la), decltype(lb), (BM == 64 && BN == 64) ? 1 : 2, K64>(acc, smem, la, lb, 0, nslab);
  conv_epilogue<DT, BM, BN>(p, acc, smem, bm, bn, Mtot, threadIdx.x, true);
}

// 3x3 / stride 1 / 64 -> 64 channels on LARGE maps (stem.conv2/3 and the res2 3x3s of a real-size image: 60k-240k pixels).
// The im2col tiling fetches every input pixel nine times - 128-row tiles x 9 slabs x 16 KB + the weights again per tile:
// 420 MB through L2 for the 31-MB stem layer at 800x1216, which bounds it at ~52 us = 8 TB/s of L2 traffic.  Here a
// workgroup owns an 8 x 32 block of output pixels of one image: the 10 x 34 x 64-channel input patch (43.5 KB) and ALL
// weights (9 taps x 64 x 64 = 73.7 KB) are brought into LDS ONCE (zero padding = out-of-range buffer offsets), then the
// whole K loop - 9 taps x 4 k-steps x (2 x 2) MFMAs per wave - runs out of LDS with no barrier and no global load: the
// A fragment of tap (dy, dx) is the patch row of pixel (y + dy, x + dx), 16 bytes per lane, swizzled like every other
// 128-byte-row LDS image here.  Same k order and MFMA as the tiled kernels (tap-major, channels ascending).
constexpr int P3_TH = 8, P3_TW = 32, P3_PH = P3_TH + 2, P3_PW = P3_TW + 2;
constexpr int P3_PATCH = P3_PH * P3_PW * 128, P3_WTS = 9 * 64 * 128;
constexpr int P3_NCH = P3_PH * P3_PW * 8, P3_NIT = (P3_NCH + 255) / 256;  // 16-byte chunks of a patch, per-thread share
// PERSISTENT: one workgroup per CU keeps the weights in LDS and walks its XCD's share of the pixel blocks; the patch of
// the NEXT block is fetched into registers while the current one is multiplied, so per block only the LDS store of the
// patch, the MFMA phase and the epilogue (two 128-pixel halves staged as fp32 in the dead patch area) remain.
// PW = true (round 4, the tail of a res2 bottleneck as ONE kernel - resnet_ws.py:217-237 conv2 -> conv3 + shortcut): the
// 3x3's output tile [256 pixels x 64 channels] (affine, ReLU, rounded to bf16 exactly as the 3x3 alone would store it) goes
// to the dead patch area in A-fragment layout instead of to memory, and each wave multiplies its 64 pixels with the 1x1's
// weights [256 x 64] (32 KB more of LDS, resident like the 3x3's) - four chunks of 64 output channels, each through the
// same staged epilogue (affine, residual, ReLU, 16-byte stores).  Same MFMA and k order as the two kernels it replaces.
constexpr int P3_PW_WTS = 256 * 128;
// LDS-only barrier: __syncthreads() also waits (vmcnt) for every global store and prefetch load in flight - the block loop
// below used to drain its output stores and the next block's patch fetch at each of its barriers
#define LDS_BARRIER() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); } while (0)
template <bool RES, bool PW = false, bool POOL = false>
__global__ __launch_bounds__(256) void conv3x3_c64_kernel(ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* patch = smem;
  char* wts = smem + P3_PATCH;
  [[maybe_unused]] char* w3s = smem + P3_PATCH + P3_WTS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (p.Wo + P3_TW - 1) / P3_TW, tiles_y = (p.Ho + P3_TH - 1) / P3_TH;
  const int per_img = tiles_y * tiles_x, total = p.Nb * per_img;
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, (unsigned)((long)p.Nb * p.H * p.W * 128), 0x00020000);
  // this thread's 16-byte chunks of a patch: position inside the patch and byte offset relative to the block's first output
  // pixel, once per workgroup (26 VALU instructions per load otherwise - divisions, 64-bit products - 10 % of a block's cycles
  // with one wave per SIMD); the buffer offsets are 32-bit (the launcher checks the tensor is < 4 GB)
  int pyx[P3_NIT], poff[P3_NIT];
#pragma unroll
  for (int it = 0; it < P3_NIT; ++it) {
    const int c = it * 256 + tid, pix = c >> 3, ch = c & 7;
    const int py = pix / P3_PW, px = pix - py * P3_PW;
    pyx[it] = c < P3_NCH ? (py | (px << 8)) : -1;
    poff[it] = ((py - 1) * p.W + (px - 1)) * 128 + ch * 16;
  }
  auto fetch = [&](int t, i32x4_t (&v)[P3_NIT]) {  // block t's patch -> registers (zero padding = out-of-range offsets)
    const int n = t / per_img, tt = t - n * per_img;
    const int y0 = (tt / tiles_x) * P3_TH, x0 = (tt % tiles_x) * P3_TW;
    const int base = ((n * p.H + y0) * p.W + x0) * 128;
#pragma unroll
    for (int it = 0; it < P3_NIT; ++it) {
      const int iy = y0 - 1 + (pyx[it] & 0xff), ix = x0 - 1 + ((pyx[it] >> 8) & 0xff);
      const bool ok = pyx[it] >= 0 && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      const unsigned off = ok ? (unsigned)(base + poff[it]) : 0xFFFFFFF0u;
      v[it] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
    }
  };
  int k = blockIdx.x;
  if (k >= total) return;
  i32x4_t pv[P3_NIT];
  fetch(xcd_remap(k, total), pv);
  // weights: [64 cout][ldw] with k = tap * 64 + ci -> LDS [tap][cout][128 B], once per workgroup
  {
    const char* wg = p.Wt;
    const long ldw_b = p.ldw * 2;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      i32x4_t v[9];
#pragma unroll
      for (int it = 0; it < 9; ++it) {
        const int c = (half * 9 + it) * 256 + tid;  // 0 .. 4607
        const int tap = c >> 9, co = (c >> 3) & 63, ch = c & 7;
        v[it] = *(const i32x4_t*)(wg + co * ldw_b + tap * 128 + ch * 16);
      }
#pragma unroll
      for (int it = 0; it < 9; ++it) {
        const int c = (half * 9 + it) * 256 + tid;
        const int tap = c >> 9, co = (c >> 3) & 63, ch = c & 7;
        *(i32x4_t*)(wts + tap * (64 * 128) + swz(co, ch)) = v[it];
      }
    }
  }
  if constexpr (PW) {  // the 1x1's weights: [256 cout][pw_ldw] (64 input channels = one 128-byte row) -> LDS [cout][128 B]
    const long ldw3_b = p.pw_ldw * 2;
    i32x4_t v[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int c = it * 256 + tid;  // 0 .. 2047
      v[it] = *(const i32x4_t*)(p.pw_w + (long)(c >> 3) * ldw3_b + (c & 7) * 16);
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int c = it * 256 + tid;
      *(i32x4_t*)(w3s + swz(c >> 3, c & 7)) = v[it];
    }
  }
  const int lx = lane & 31, lh = lane >> 5;
  [[maybe_unused]] float sc3[4][2], bi3[4][2];
  if constexpr (PW) {
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        sc3[cb][j] = p.pw_scale ? p.pw_scale[cb * 64 + j * 32 + lx] : 1.f;
        bi3[cb][j] = p.pw_bias ? p.pw_bias[cb * 64 + j * 32 + lx] : 0.f;
      }
  }
  // this lane's two output channels' affine, once per workgroup (inside the block loop each half of every epilogue paid
  // a global-load latency for them: one wave per SIMD hides nothing - 16 of 38 us on the stem layer at 800x1216)
  float sc2[2], bi2[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    sc2[j] = p.scale ? p.scale[j * 32 + lx] : 1.f;
    bi2[j] = p.bias ? p.bias[j * 32 + lx] : 0.f;
  }
  for (; k < total; k += gridDim.x) {
    const int t = xcd_remap(k, total);
    const int n = t / per_img, tt = t - n * per_img;
    const int y0 = (tt / tiles_x) * P3_TH, x0 = (tt % tiles_x) * P3_TW;
#pragma unroll
    for (int it = 0; it < P3_NIT; ++it) {
      const int c = it * 256 + tid;
      if (c < P3_NCH) *(i32x4_t*)(patch + swz(c >> 3, c & 7)) = pv[it];
    }
    LDS_BARRIER();
    if (k + (int)gridDim.x < total) fetch(xcd_remap(k + gridDim.x, total), pv);  // lands under the MFMA phase
    f32x16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // 36 k-steps (9 taps x 4), software-pipelined by hand: one wave per SIMD has nobody to hide its LDS latency behind,
    // so the fragments of step s + 1 are requested before the four MFMAs of step s are issued
    i32x4_t fa[2][2], fb[2][2];
    auto frags = [&](int s_, i32x4_t (&a)[2], i32x4_t (&b)[2]) {
      const int tap = s_ >> 2, ks = s_ & 3, dy = tap / 3, dx = tap - dy * 3, slot = ks * 2 + lh;
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = *(const i32x4_t*)(patch + swz((wave * 2 + i + dy) * P3_PW + lx + dx, slot));
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = *(const i32x4_t*)(wts + tap * (64 * 128) + swz(j * 32 + lx, slot));
    };
    frags(0, fa[0], fb[0]);
#pragma unroll
    for (int s_ = 0; s_ < 36; ++s_) {
      if (s_ + 1 < 36) frags(s_ + 1, fa[(s_ + 1) & 1], fb[(s_ + 1) & 1]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mma_step<DRN_BF16>(acc[i][j], fa[s_ & 1][i], fb[s_ & 1][j]);
      // one k-step's reads, then one k-step's MFMAs: keep the compiler from sinking the reads to their first use
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    // epilogue: affine -> fp32 [128 pixels][64 channels] in the (dead) patch area, one half of the block at a time -> 8
    // channels per lane: residual, ReLU, 16-byte stores
    // WAVE-PRIVATE and barrier-free (cycle counters on the first version - fp32 halves of the whole block staged by all
    // four waves, two barriers per half - put 38 % of a block's time in the epilogue, one wave per SIMD hiding nothing): a wave
    // stages one of its two 32-pixel output rows at a time as fp32 [32 pixels][64 channels] in its own 8.5 KB (row pitch 68
    // floats: the two half-waves, four pixels apart, land on different banks), reads it back as 32-byte runs - LDS operations
    // of one wave execute in order, so its own writes and reads need no barrier - adds the residual, ReLU, and stores 16-byte
    // pieces of its own pixels' 128-byte rows.  The four waves run their epilogues independently.
    constexpr int EP_PITCH = 68;
    float* wtile = (float*)(patch + wave * (32 * EP_PITCH * 4));
    auto epilogue = [&](f32x16_t (&ac)[2][2], const float (&sc_)[2], const float (&bi_)[2], int ch0, int relu_) {
    [[maybe_unused]] int keep[4][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int y = y0 + wave * 2 + i;
      i32x4_t rv[4];
      if constexpr (RES) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int idx = it * 64 + lane, ml = idx >> 3, cg = idx & 7;
          const int yc = min(y, p.Ho - 1), xc = min(x0 + ml, p.Wo - 1);
          rv[it] = *(const i32x4_t*)((const bf16_t*)p.residual + (((long)n * p.Ho + yc) * p.Wo + xc) * p.ldres + ch0 + cg * 8);
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          wtile[((r & 3) + 8 * (r >> 2) + 4 * lh) * EP_PITCH + j * 32 + lx] = ac[i][j][r] * sc_[j] + bi_[j];
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int idx = it * 64 + lane, ml = idx >> 3, cg = idx & 7;
        const int x = x0 + ml;
        const long m = ((long)n * p.Ho + y) * p.Wo + x;
        const f32x4_t lo = *(const f32x4_t*)(wtile + ml * EP_PITCH + cg * 8), hi = *(const f32x4_t*)(wtile + ml * EP_PITCH + cg * 8 + 4);
        float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        i32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if constexpr (RES) {
            const uint32_t w = (uint32_t)rv[it][e];
            v[2 * e] += __builtin_bit_cast(float, w << 16) * p.res_mult;
            v[2 * e + 1] += __builtin_bit_cast(float, w & 0xffff0000u) * p.res_mult;
          }
          if (relu_) { v[2 * e] = fmaxf(v[2 * e], 0.f); v[2 * e + 1] = fmaxf(v[2 * e + 1], 0.f); }
          o[e] = (int)((uint32_t)f32_to_bf16(v[2 * e]) | ((uint32_t)f32_to_bf16(v[2 * e + 1]) << 16));
        }
        if constexpr (!POOL) {
          if (y < p.Ho && x < p.Wo) *(i32x4_t*)((bf16_t*)p.Y + m * p.ldy + ch0 + cg * 8) = o;
        } else {
          // 2 x 2 / stride-2 maximum of the ReLU'd, bf16-rounded outputs (non-negative: their bit patterns order like
          // integers): the wave's two output rows are one pooled row - vertical partner = the same thread's piece of row
          // i = 0, horizontal partner (pixel ml ^ 1) = lane ^ 8
          if (i == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) keep[it][e] = o[e];
          } else {
            typedef short s16x2p_t __attribute__((ext_vector_type(2)));
            auto pkmax = [](int a, int b) {
              return __builtin_bit_cast(int, __builtin_elementwise_max(__builtin_bit_cast(s16x2p_t, a), __builtin_bit_cast(s16x2p_t, b)));
            };
            int pe[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int mx = pkmax(keep[it][e], o[e]);
              pe[e] = pkmax(mx, __shfl_xor(mx, 8, 64));
            }
            const i32x4_t po = {pe[0], pe[1], pe[2], pe[3]};
            const int Hp = (p.Ho - 2) / 2 + 1, Wp = (p.Wo - 2) / 2 + 1;
            const int yp = (y0 >> 1) + wave, xp = (x0 + ml) >> 1;
            if ((ml & 1) == 0 && yp < Hp && xp < Wp)
              *(i32x4_t*)((bf16_t*)p.Y + (((long)n * Hp + yp) * Wp + xp) * p.ldy + ch0 + cg * 8) = po;
          }
        }
      }
    }
    };
    if constexpr (!PW) {
      LDS_BARRIER();  // every wave is done reading the patch: the staging rows reuse its space
      epilogue(acc, sc2, bi2, 0, p.relu);
    } else {
      // the 3x3's output -> bf16 A fragments: rows = this wave's 64 pixels (wave * 64 + i * 32 + pixel), 128 B = 64 channels
      LDS_BARRIER();  // every wave is done reading the patch
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ml = wave * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh, nl = j * 32 + lx;
            float v = acc[i][j][r] * sc2[j] + bi2[j];
            if (p.relu) v = fmaxf(v, 0.f);
            *(bf16_t*)(patch + swz(ml, nl >> 3) + (nl & 7) * 2) = f32_to_bf16(v);
          }
      i32x4_t ya[2][4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) ya[i][ks] = *(const i32x4_t*)(patch + swz(wave * 64 + i * 32 + lx, ks * 2 + lh));
      LDS_BARRIER();  // every wave has its fragments: the staging rows below overlap the other waves' y2 rows
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {  // (unrolled: sc3 / bi3 are register arrays)
        f32x16_t a3[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) a3[i][j][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          i32x4_t b3[2];
#pragma unroll
          for (int j = 0; j < 2; ++j) b3[j] = *(const i32x4_t*)(w3s + swz(cb * 64 + j * 32 + lx, ks * 2 + lh));
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) mma_step<DRN_BF16>(a3[i][j], ya[i][ks], b3[j]);
        }
        epilogue(a3, sc3[cb], bi3[cb], cb * 64, p.pw_relu);
      }
    }
    LDS_BARRIER();  // tile reads done before the next block's patch overwrites the area
  }
}

#undef LDS_BARRIER
// Mid-size layers (the res3 / res4 convs of a real-size image: a few hundred 64x64 tiles, 8 .. 72 K-slabs): one 64x64 tile
// per CU on four waves is latency-bound (~0.5 us per slab), the 32x32 wave-K-split kernel moves 2x the operand bytes per
// flop and runs into the L2 bandwidth (res4 3x3 on 3800 pixels: 952 workgroups x 36 slabs x 8 KB = 274 MB in 16 us).
// Here TWO groups of four waves share one 64x64 tile: group g multiplies the K-slabs [g * n/2, (g + 1) * n/2) out of
// its own 16-KB LDS stage with its own register ring - twice the loads in flight and twice the MFMA issue per tile, the
// operand bytes of the 64x64 tiling - and group 1's partial tile is added to group 0's through LDS (fixed order) in
// front of the common epilogue.  Needs an even slab count; chosen on ONE image's geometry like the other variants.
template <int DT, bool K64 = true>
__global__ __launch_bounds__(512) void conv_nhwc_k2_kernel(ConvParams p) {  // (forcing 128 VGPRs for two workgroups per CU: 8 B of scratch, res4 layers 3 % slower, not kept)
  extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 x 16 KB
  constexpr int ES = EsOf<DT>::value;
  const int Mtot = p.Nb * p.Ho * p.Wo;
  const int tiles_m = (Mtot + 63) / 64, tiles_n = (p.Cout + 63) / 64;
  int tm, tn;
  tile_coords(xcd_remap(blockIdx.x, tiles_m * tiles_n), tiles_m, tiles_n, tm, tn);
  const int bm = tm * 64, bn = tn * 64;
  const int tid = threadIdx.x & 255, g = threadIdx.x >> 8;
  ConvLoader<DT, 64> la;
  la.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, (unsigned)((long)p.Nb * p.H * p.W * p.Cin * ES), 0x00020000);
  la.H = p.H; la.W = p.W; la.Cin = p.Cin; la.KW = p.KW; la.dil = p.dil; la.ntaps = p.KH * p.KW;
  const int r0 = tid >> 3;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int m = bm + r0 + 32 * q;
    if (m < Mtot) {
      const int n = m / (p.Ho * p.Wo), rem = m - n * p.Ho * p.Wo;
      const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
      la.hi0[q] = ho * p.stride - p.pad;
      la.wi0[q] = wo * p.stride - p.pad;
      la.nbase[q] = (unsigned)((long)n * p.H * p.W * p.Cin * ES);
    } else {
      la.hi0[q] = 0; la.wi0[q] = 0; la.nbase[q] = ConvLoader<DT, 64>::OOB;
    }
  }
  const RowLoader lb = make_row_loader(p.Wt, bn, p.Cout, 64, p.ldw * ES);
  f32x16_t acc[1][1];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
  const int half = ((p.Ktot * ES + 127) / 128) >> 1;  // launcher: the slab count is even
  mainloop<DT, 64, 64, decltype(la), decltype(lb), 1, K64>(acc, smem + g * (128 * 128), la, lb, g * half, (g + 1) * half,
                                                           tid);
  // group 1's partial tile -> LDS (its own stage: nobody reads it any more), added by group 0 lane for lane
  const int lane = tid & 63, wave = tid >> 6;
  float* part = (float*)(smem + 128 * 128) + wave * 1024 + lane;
  if (g == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) part[r * 64] = acc[0][0][r];
  }
  __syncthreads();
  if (g == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] += part[r * 64];
  }
  conv_epilogue<DT, 64, 64>(p, acc, smem, bm, bn, Mtot, tid, g == 0);
}

// Small-map convolution: 32 x 32 output tile per workgroup, the K range of every 128-byte slab split over the FOUR WAVES
// (wave w multiplies k-step w: one MFMA and two LDS fragment reads per wave and slab), their accumulators added in wave
// order through LDS at the end.  For the res3 / res4 layers of a 224 x 224 image (196 .. 784 pixels) the 64 x 64 kernel
// runs on 16 .. 26 workgroups and its per-slab chain - 8 fragment reads, 4 dependent MFMAs, two barriers - costs ~0.55 us
// whatever the prefetch depth (measured: ring depth 3 / 4 / 5 and division-free addressing all within 5 %), so a 36-slab
// 3 x 3 conv took 23 us on 196 pixels.  Here the chain per slab is a quarter of that and there are 4x the workgroups.
// (Splitting K over workgroups instead - partial tiles in HBM, last arriver reduces - was built and measured slower
// than no split: the cross-XCD coherence of the partials costs more than the split saves; HISTORY.md section 5.)
template <int DT, bool K64 = true>
__global__ __launch_bounds__(256) void conv_nhwc_ks_kernel(ConvParams p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * 32 * 32 * 4];  // one 8-KB operand stage, then 4 partial tiles
  constexpr int ES = EsOf<DT>::value;
  constexpr int DEPTH = 4;
  const int Mtot = p.Nb * p.Ho * p.Wo;
  const int tiles_m = (Mtot + 31) / 32, tiles_n = (p.Cout + 31) / 32;
  int tm, tn;
  tile_coords(xcd_remap(blockIdx.x, tiles_m * tiles_n), tiles_m, tiles_n, tm, tn);
  const int bm = tm * 32, bn = tn * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  ConvLoader<DT, 32> la;
  la.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, (unsigned)((long)p.Nb * p.H * p.W * p.Cin * ES), 0x00020000);
  la.H = p.H; la.W = p.W; la.Cin = p.Cin; la.KW = p.KW; la.dil = p.dil; la.ntaps = p.KH * p.KW;
  {
    const int m = bm + (tid >> 3);
    if (m < Mtot) {
      const int n = m / (p.Ho * p.Wo), rem = m - n * p.Ho * p.Wo;
      const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
      la.hi0[0] = ho * p.stride - p.pad;
      la.wi0[0] = wo * p.stride - p.pad;
      la.nbase[0] = (unsigned)((long)n * p.H * p.W * p.Cin * ES);
    } else {
      la.hi0[0] = 0; la.wi0[0] = 0; la.nbase[0] = ConvLoader<DT, 32>::OOB;
    }
  }
  const RowLoader lb = make_row_loader(p.Wt, bn, p.Cout, 32, p.ldw * ES);
  f32x16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int n = (p.Ktot * ES + 127) / 128;
  i32x4_t ra[DEPTH][1], rb[DEPTH][1];
#pragma unroll
  for (int d = 0; d < DEPTH; ++d)
    if (d < n) {
      la.template load<32>(ra[d], d, tid);
      lb.template load<32>(rb[d], d, tid);
    }
  lds_store_tile<32>(smem, ra[0], tid);
  lds_store_tile<32>(smem + 32 * 128, rb[0], tid);
  __syncthreads();
  const int slot = wave * 2 + (lane >> 5);
  auto slab = [&](auto dtag, int i, auto fulltag) {  // steady state / bounds-checked tail: see mainloop()
    constexpr int d = decltype(dtag)::value;
    constexpr bool FULL = decltype(fulltag)::value;
    if (FULL || i + DEPTH < n) {
      la.template load<32>(ra[d], i + DEPTH, tid);
      lb.template load<32>(rb[d], i + DEPTH, tid);
    }
    if constexpr (DT == DRN_FP8 && K64) {
      // K = 64 scaled MFMA: waves 0 / 1 multiply the two halves of the slab (k-steps 2w, 2w + 1), waves 2 / 3 add zeros
      if (wave < 2) {
        const int s2 = wave * 4 + (lane >> 5);
        const i32x4_t fa0 = *(const i32x4_t*)(smem + swz(lane & 31, s2)), fa1 = *(const i32x4_t*)(smem + swz(lane & 31, s2 + 2));
        const i32x4_t fb0 = *(const i32x4_t*)(smem + 32 * 128 + swz(lane & 31, s2));
        const i32x4_t fb1 = *(const i32x4_t*)(smem + 32 * 128 + swz(lane & 31, s2 + 2));
        mma_step64_fp8(acc, fa0, fa1, fb0, fb1);
      }
    } else {
      const i32x4_t fa = *(const i32x4_t*)(smem + swz(lane & 31, slot));
      const i32x4_t fb = *(const i32x4_t*)(smem + 32 * 128 + swz(lane & 31, slot));
      mma_step<DT>(acc, fa, fb);
    }
    __syncthreads();
    if (FULL || i + 1 < n) {
      lds_store_tile<32>(smem, ra[(d + 1) % DEPTH], tid);
      lds_store_tile<32>(smem + 32 * 128, rb[(d + 1) % DEPTH], tid);
    }
    __syncthreads();
  };
  int base = 0;
  for (; base + 2 * DEPTH <= n; base += DEPTH)
    static_for<DEPTH>([&](auto dtag) { slab(dtag, base + decltype(dtag)::value, std::true_type{}); });
  for (; base < n; base += DEPTH)
    static_for<DEPTH>([&](auto dtag) {
      const int i = base + decltype(dtag)::value;
      if (i < n) slab(dtag, i, std::false_type{});
    });
  // the four k-step partials, as [wave][row][col] fp32
  float* part = (float*)smem;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int ml = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    part[(wave * 32 + ml) * 32 + (lane & 31)] = acc[r];
  }
  __syncthreads();
  const bool vec_epi = (p.Cout & 7) == 0 && vec8_ok(p.out_dt, p.Y, p.ldy) &&
                       (!p.residual || vec8_ok(p.res_dt, p.residual, p.ldres));
  if (vec_epi) {  // 128 lanes: one pixel row x 8 channels each (see conv_nhwc_kernel)
    if (tid >= 128) return;
    const int ml = tid >> 2, cg = tid & 3, m = bm + ml, nn = bn + cg * 8;
    if (m >= Mtot || nn >= p.Cout) return;
    i32x4_t rv = {0, 0, 0, 0};
    if (p.residual) rv = load8(p.res_dt, p.residual, (long)m * p.ldres + nn);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int o = ml * 32 + cg * 8 + e;
      const float sum = ((part[o] + part[1024 + o]) + part[2048 + o]) + part[3072 + o];
      v[e] = sum * (p.scale ? p.scale[nn + e] : 1.f) + (p.bias ? p.bias[nn + e] : 0.f);
    }
    if (p.residual) add8(p.res_dt, rv, p.res_mult, v);
    if (p.relu) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
    }
    store8(p.out_dt, p.Y, (long)m * p.ldy + nn, v);
    return;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int o = tid + 256 * q, ml = o >> 5, nl = o & 31, m = bm + ml, nn = bn + nl;
    if (m >= Mtot || nn >= p.Cout) continue;
    const float sum = ((part[o] + part[1024 + o]) + part[2048 + o]) + part[3072 + o];
    float v = sum * (p.scale ? p.scale[nn] : 1.f) + (p.bias ? p.bias[nn] : 0.f);
    if (p.residual) {
      const long ri = (long)m * p.ldres + nn;
      const float rres = p.res_dt == DRN_BF16 ? bf16_to_f32(((const bf16_t*)p.residual)[ri])
                         : p.res_dt == DRN_FP8 ? fp8_to_f32(((const uint8_t*)p.residual)[ri])
                                               : ((const float*)p.residual)[ri];
      v += rres * p.res_mult;
    }
    if (p.relu) v = fmaxf(v, 0.f);
    const long yi = (long)m * p.ldy + nn;
    if (p.out_dt == DRN_BF16) ((bf16_t*)p.Y)[yi] = f32_to_bf16(v);
    else if (p.out_dt == DRN_FP8) ((uint8_t*)p.Y)[yi] = f32_to_fp8(v);
    else ((float*)p.Y)[yi] = v;
  }
}

template <int DT, bool K64 = true>
int launch_conv_ks(const ConvParams& p, hipStream_t st) {
  const int Mtot = p.Nb * p.Ho * p.Wo;
  const int tiles = ((Mtot + 31) / 32) * ((p.Cout + 31) / 32);
  hipLaunchKernelGGL((conv_nhwc_ks_kernel<DT, K64>), dim3(tiles), dim3(256), 0, st, p);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

static int launch_conv3x3_c64(const ConvParams& p, hipStream_t st) {
  const int tiles = p.Nb * ((p.Ho + P3_TH - 1) / P3_TH) * ((p.Wo + P3_TW - 1) / P3_TW);
  constexpr int smem = P3_PATCH + P3_WTS;  // 117 KB: one workgroup per CU
  const int nwg = tiles < cu_count() ? tiles : cu_count();  // persistent: one workgroup per CU walks the pixel blocks
  auto k = !p.residual ? conv3x3_c64_kernel<false> : conv3x3_c64_kernel<true>;
  if (!drn_launch::allow_lds((const void*)k, smem)) return DRN_ERR_LAUNCH;
  hipLaunchKernelGGL(k, dim3(nwg), dim3(256), smem, st, p);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

template <bool RES, bool PW, bool POOL>
static int launch_c64_variant(const ConvParams& p, int nwg, int smem, hipStream_t st) {
  if (!drn_launch::allow_lds((const void*)conv3x3_c64_kernel<RES, PW, POOL>, smem)) return DRN_ERR_LAUNCH;
  hipLaunchKernelGGL((conv3x3_c64_kernel<RES, PW, POOL>), dim3(nwg), dim3(256), smem, st, p);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}
// the fused forms (drn_conv3x3_pw_nhwc): [3x3] [+ 1x1 to 256 channels] [+ 2x2 max pool]
static int launch_conv3x3_c64_pw(const ConvParams& p, hipStream_t st) {
  const int tiles = p.Nb * ((p.Ho + P3_TH - 1) / P3_TH) * ((p.Wo + P3_TW - 1) / P3_TW);
  const bool pw = p.pw_w != nullptr, res = p.residual != nullptr, pool = p.pool != 0;
  const int smem = P3_PATCH + P3_WTS + (pw ? P3_PW_WTS : 0);  // 117 / 146.5 KB: one workgroup per CU
  const int nwg = tiles < cu_count() ? tiles : cu_count();
#define C64_CASE(R_, W_, P_) if (res == R_ && pw == W_ && pool == P_) return launch_c64_variant<R_, W_, P_>(p, nwg, smem, st)
  C64_CASE(false, true, false); C64_CASE(true, true, false); C64_CASE(false, true, true); C64_CASE(true, true, true);
  C64_CASE(false, false, true); C64_CASE(true, false, true);
#undef C64_CASE
  return DRN_ERR_UNSUPPORTED;  // (no 1x1 and no pool: drn_conv2d_nhwc's own class)
}

template <int DT, bool K64 = true>
int launch_conv_k2(const ConvParams& p, hipStream_t st) {
  const int Mtot = p.Nb * p.Ho * p.Wo;
  const int tiles = ((Mtot + 63) / 64) * ((p.Cout + 63) / 64);
  hipLaunchKernelGGL((conv_nhwc_k2_kernel<DT, K64>), dim3(tiles), dim3(512), 2 * 128 * 128, st, p);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

static int launch_conv1x1_pp(const ConvParams& p, hipStream_t st) {
  const long Mtot = (long)p.Nb * p.Ho * p.Wo;
  const int tiles = (int)((Mtot + 255) / 256) * ((p.Cout + 255) / 256);
  constexpr int smem = 2 * 512 * 128;
  if (!drn_launch::allow_lds((const void*)conv1x1_pp_kernel, smem)) return DRN_ERR_LAUNCH;
  hipLaunchKernelGGL(conv1x1_pp_kernel, dim3(tiles), dim3(512), smem, st, p);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

template <int DT, int BM, int BN, bool K64 = true>
int launch_conv(const ConvParams& p, hipStream_t st) {
  const int Mtot = p.Nb * p.Ho * p.Wo;
  const int tiles = ((Mtot + BM - 1) / BM) * ((p.Cout + BN - 1) / BN);
  constexpr int smem = ((BM == 64 && BN == 64) ? 1 : 2) * (BM + BN) * 128;
  auto k = conv_nhwc_kernel<DT, BM, BN, K64>;
  if (smem > 48 * 1024 && !drn_launch::allow_lds((const void*)k, smem)) return DRN_ERR_LAUNCH;
  hipLaunchKernelGGL(k, dim3(tiles), dim3(256), smem, st, p);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// ---- the forward's host side: which kernel a layer runs on (conv_fwd_plan) and its launch (conv_fwd_launch) ----------------

// (dtype, fp8_k64) -> the <DT, K64> template arguments of the tiled / k2 / ks kernels: f(integral_constant<int, DT>,
// bool_constant<K64>).  K64 only distinguishes the fp8 kernels.
template <class F>
int with_conv_dtype(int dtype, bool k64, F&& f) {
  if (dtype == DRN_BF16) return f(std::integral_constant<int, DRN_BF16>{}, std::true_type{});
  if (dtype == DRN_FP8)
    return k64 ? f(std::integral_constant<int, DRN_FP8>{}, std::true_type{})
               : f(std::integral_constant<int, DRN_FP8>{}, std::false_type{});
  return f(std::integral_constant<int, DRN_F32>{}, std::true_type{});
}

bool al16(const void* q) { return (((uintptr_t)q) & 15) == 0; }

// What conv3x3_c64_kernel asks of every caller (drn_conv2d_nhwc_q's plan and drn_conv3x3_pw_nhwc): the knob, a map of at least
// conv_patch_min pixels (117 KB of LDS, so only where the trunk is not meant to share CUs with the heads' GEMMs: maps of
// >= 32k pixels), 16-byte weight rows, aligned weights / output / shortcut.
bool patch_c64_ok(const DrnTune& t, long pixels, const void* w, long ldw, const void* y, const void* residual) {
  return t.conv_patch && pixels >= t.conv_patch_min && (ldw * 2) % 16 == 0 && al16(w) && al16(y) && (!residual || al16(residual));
}

struct ConvPlan {
  int kind;   // DRN_CONV_KIND_* (include/drn_wsod.h)
  int dtype;  // element type of x / w
  bool k64;   // fp8 operands: the K = 64 scaled MFMA (false: the K = 16 form, DRN_CONV_KIND_FP8_K16 in drn_conv2d_plan)
};

// Which kernel runs the layer `p` (operands of `dtype`) under the knobs `t` on a device of `cus` compute units.  Pure: no device
// call, no read of g_tune.  The ONE place that holds a class condition of the forward; the order of the rules is part of it.
// Every family gives the same bits except the two small-map kernels (k2, ks), which add their K partials in another order.
ConvPlan conv_fwd_plan(const ConvParams& p, int dtype, const DrnTune& t, int cus) {
  ConvPlan pl{DRN_CONV_KIND_TILED_128, dtype, dtype != DRN_FP8 || t.fp8_k64 != 0};
  auto is = [&](int kind) { pl.kind = kind; return pl; };
  const int es = drn_esize(dtype);
  const bool res = p.residual != nullptr;
  const bool bf16_io = dtype == DRN_BF16 && p.out_dt == DRN_BF16 && (!res || p.res_dt == DRN_BF16);
  const long HoWo = (long)p.Ho * p.Wo, Mtot = (long)p.Nb * HoWo;
  const int nslab = (p.Ktot * es + 127) / 128;
  // (decided on ONE image's geometry: the k2 / ks kernels add the K partials in another order than the tiled ones, and a layer
  // must round the same way whether its image runs alone or in a batch - graphed trunk pairs vs eager, 2 ranks vs 1)
  const long tiles64 = ((HoWo + 63) / 64) * ((p.Cout + 63) / 64);

  // LDS-resident patch + weights for the 64-channel 3x3 layers of large maps (conv3x3_c64_kernel)
  if (bf16_io && p.Cin == 64 && p.Cout == 64 && p.KH == 3 && p.KW == 3 && p.stride == 1 && p.dil == 1 && p.pad == 1 &&
      patch_c64_ok(t, HoWo, p.Wt, p.ldw, p.Y, p.residual) && (p.ldy & 7) == 0 && (!res || (p.ldres & 7) == 0))
    return is(DRN_CONV_KIND_PATCH_C64);

  // What the register-ring kernels (conv_ring.hip) and the eight-wave kernel (pp8.hip) both ask: bf16, whole 64-channel K slabs
  // (so nslab == KH * KW * (Cin >> 6)), 16-byte rows and pointers, 32-bit byte offsets into the weights
  const bool slab64 = bf16_io && (p.Cin & 63) == 0 && (p.Cout & 7) == 0 && p.KH * p.KW <= 32 && (p.ldy & 7) == 0 &&
                      (!res || (p.ldres & 7) == 0) && al16(p.X) && al16(p.Wt) && al16(p.Y) && (!res || al16(p.residual)) &&
                      (p.ldw * 2) % 16 == 0 && (long)p.Cout * p.ldw * 2 < 0xFFFFFFF0L;
  // (pp8 reads scale / bias as vectors; the input's 32-bit range is an argument check of the entry points)
  const bool pp8_ok = t.pp8 && slab64 && (!p.scale || al16(p.scale)) && (!p.bias || al16(p.bias));
  // the 256x128 form where one image's layer gives it at least ~5/8 of the CUs' worth of tiles (drn_pp8_wide_ok)
  auto pp8 = [&] { return is(drn_pp8_wide_ok(HoWo, p.Cout, t, cus) ? DRN_CONV_KIND_PP8_WIDE : DRN_CONV_KIND_PP8); };
  if (t.pp8 == 2 && pp8_ok) return pp8();  // (A/B pin: every layer in the eight-wave kernel's class takes it)

  // 1x1 / stride 1 convs to >= 256 channels of a large map: the GEMM ping-pong mainloop with the conv epilogue
  // (conv1x1_pp_kernel; the dilated-C5 trunk's 1x1s to 512 / 1024 / 2048 channels and the res2 1x1s to 256 channels at a real
  // image size).  Class measured (profiles/r5_17_conv1x1_pp_threshold_*.txt, r5_19_conv_800.txt): from ~3/4 of the CUs' worth
  // of 256x256 tiles per image on it wins at any K; at 100-191 tiles - half the chip holds a tile - only with a long K loop
  // (>= 16 slabs: 2048 -> 512 at 118 tiles 47 -> 44 us, but 128 -> 512 at 120 tiles 12 -> 15 us); at 59-60 tiles (res4 of the
  // C4 trunk, the DC5 trunk's 1x1s to 256 channels) the small tiles win; a 64-channel output wastes three quarters of the
  // tile.  Decided on ONE image's geometry; same bits as the tiled kernels either way.
  const bool pp_ok = t.conv_pp && bf16_io && p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad == 0 && (p.Cin & 63) == 0 &&
                     (p.Cout & 7) == 0 && (p.ldy & 3) == 0 && (!res || (p.ldres & 3) == 0) &&
                     (((uintptr_t)p.X | (uintptr_t)p.Wt | (uintptr_t)p.Y | (uintptr_t)p.residual) & 15) == 0 &&
                     (p.ldw * 2) % 16 == 0 && (long)p.Cout * p.ldw * 2 < 0xFFFFFFF0L;
  const long t256 = ((HoWo + 255) / 256) * ((p.Cout + 255) / 256);
  // (1) >= 3/4 of the CUs' worth of 256x256 tiles: the ping-pong GEMM mainloop, whatever K
  if (pp_ok && (t.conv_pp > 1 ? t256 >= t.conv_pp : (p.Cout >= 256 && t256 >= 192))) return is(DRN_CONV_KIND_PP256);
  // (2) the eight-wave 128x128 / 256x128 kernel (pp8.hip; round 6): layers with too few 256x256 tiles for (1) - the 3x3s of
  // res4 / res5, the 1x1s to 256 / 512 channels of the dilated-C5 trunk, the C4 trunk's 1x1s to 1024 channels.  Measured class
  // (tools/conv_bench.py / tools/pp8_probe.py at 800x1216, profiles/r6_*): one image's layer offers at least 5/8 of the CUs a
  // 128x128 tile and the K loop is long enough to amortise the ring's prologue.
  const long t128 = ((HoWo + 127) / 128) * ((p.Cout + 127) / 128);
  if (pp8_ok && (t.pp8 != 1 || (nslab >= 4 && t128 * 8 >= 5L * cus && p.Cout >= 128))) return pp8();
  // (3) 100-191 tiles of 256x256 with a long K loop (round 5's class; reached when (2) is switched off)
  if (pp_ok && t.conv_pp == 1 && p.Cout >= 256 && t256 >= 100 && (p.Cin >> 6) >= 16) return is(DRN_CONV_KIND_PP256);

  // everything beyond the latency-bound small maps: the register-ring kernels.  Where they win (tools/conv_bench.py at
  // 800x1216, profiles/r5_04_*, r5_12_*): layers of >= 4 K slabs on more than CUs / 4 and up to ~4 rounds of 64x64 tiles per
  // image - the res3 / res4 1x1 and 3x3 layers of a real-size image.  Single-slab 1x1s and the huge res2 maps are bound by
  // their output traffic (the 128-wide tiled kernels move fewer operand bytes there); maps of fewer than 1024 pixels (the
  // 224x224 benchmark image) stay in the small-map kernels' class.  Decided on ONE image's geometry, as above.
  if (t.conv_ring && slab64) {
    if (t.conv_ring == 128) return is(DRN_CONV_KIND_RING_128);
    if (t.conv_ring != 1 || (nslab >= 4 && tiles64 > cus / 4 && tiles64 <= 4L * cus && HoWo >= 1024))
      return is(DRN_CONV_KIND_RING_64);
  }

  // two K-groups per 64x64 tile (conv_nhwc_k2_kernel): mid-size layers - more 64x64 tiles than the wave-K-split kernel
  // takes, at most one per CU (the kernel keeps one 512-thread workgroup per CU) - with an even slab count >= 8
  const long k2_max = t.conv_k2_tiles >= 0 ? t.conv_k2_tiles : cus;
  if ((nslab & 1) == 0 && nslab >= 8 && tiles64 > cus / 4 && tiles64 <= k2_max && p.Nb <= 64) return is(DRN_CONV_KIND_K2);
  // few 64x64 tiles and a long K loop: latency-bound, see conv_nhwc_ks_kernel
  // (round 2, tools/conv_bench.py at 800x1216: up to one 64x64 tile per CU the 36-slab res4 3x3 still gains, 23.1 ->
  // 20.5 us, while layers with few slabs lose - the 9-slab stem 3x3 8.6 -> 9.7 us at 224x224: deep K only)
  const long ks_max = t.conv_ks_tiles > 0 ? t.conv_ks_tiles : (nslab >= 32 ? cus : cus / 4);
  if (t.conv_ksplit && tiles64 <= ks_max && nslab >= 8 && p.Nb <= 64) return is(DRN_CONV_KIND_KS);

  // the tiled kernels, on the BATCH's geometry (they give the same bits at every tile)
  if (((Mtot + 127) / 128) * ((p.Cout + 127) / 128) < 128) return is(DRN_CONV_KIND_TILED_64);
  // narrow outputs (the 64-channel stem / res2 layers at real image sizes): a 128x128 tile would run half empty
  return is(p.Cout <= 64 ? DRN_CONV_KIND_TILED_128X64 : DRN_CONV_KIND_TILED_128);
}

// Issues what the plan says.  A refused launch is DRN_ERR_LAUNCH: no other kernel is tried.
int conv_fwd_launch(const ConvPlan& pl, const ConvParams& p, hipStream_t st) {
  auto tiled = [&](auto bm, auto bn) {
    return with_conv_dtype(pl.dtype, pl.k64, [&](auto dt, auto k64) {
      return launch_conv<decltype(dt)::value, decltype(bm)::value, decltype(bn)::value, decltype(k64)::value>(p, st);
    });
  };
  using i64 = std::integral_constant<int, 64>;
  using i128 = std::integral_constant<int, 128>;
  switch (pl.kind) {
    case DRN_CONV_KIND_PATCH_C64: return launch_conv3x3_c64(p, st);
    case DRN_CONV_KIND_PP256: return launch_conv1x1_pp(p, st);
    case DRN_CONV_KIND_PP8: return drn_pp8_conv_launch(p, false, st);
    case DRN_CONV_KIND_PP8_WIDE: return drn_pp8_conv_launch(p, true, st);
    case DRN_CONV_KIND_RING_64: return drn_conv_ring_launch(p, 64, st);
    case DRN_CONV_KIND_RING_128: return drn_conv_ring_launch(p, 128, st);
    case DRN_CONV_KIND_K2:
      return with_conv_dtype(pl.dtype, pl.k64, [&](auto dt, auto k64) {
        return launch_conv_k2<decltype(dt)::value, decltype(k64)::value>(p, st);
      });
    case DRN_CONV_KIND_KS:
      return with_conv_dtype(pl.dtype, pl.k64, [&](auto dt, auto k64) {
        return launch_conv_ks<decltype(dt)::value, decltype(k64)::value>(p, st);
      });
    case DRN_CONV_KIND_TILED_64: return tiled(i64{}, i64{});
    case DRN_CONV_KIND_TILED_128X64: return tiled(i128{}, i64{});
    default: return tiled(i128{}, i128{});
  }
}

// The argument checks of drn_conv2d_nhwc_q and drn_conv2d_plan, and the parameter block.  Pointers are inspected, never
// dereferenced.
int conv_params(const void* x, const void* w, void* y, const float* scale, const float* bias, const void* residual, int Nb, int H,
                int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil, long ldw, long ldy, long ldres, int relu,
                int dtype, int out_dtype, int res_dtype, float res_mult, const DrnTune& t, ConvParams& p) {
  if (!x || !w || !y) return DRN_ERR_ARG;
  auto known = [](int d) { return d == DRN_F32 || d == DRN_BF16 || d == DRN_FP8; };
  if (!known(dtype) || !known(out_dtype) || (residual && !known(res_dtype))) return DRN_ERR_ARG;
  const int es = drn_esize(dtype);
  if ((Cin * es) % 16 != 0 || (ldw * es) % 16 != 0) return DRN_ERR_ARG;  // 16-B chunks never straddle taps
  const int Ho = (H + 2 * pad - dil * (KH - 1) - 1) / stride + 1;
  const int Wo = (W + 2 * pad - dil * (KW - 1) - 1) / stride + 1;
  if (Ho <= 0 || Wo <= 0 || Nb <= 0) return DRN_ERR_ARG;
  if ((long)Nb * H * W * Cin * es >= 0xFFFFFFF0L) return DRN_ERR_ARG;  // one buffer descriptor spans the input
  const int Ktot = KH * KW * Cin;
  if (ldw * es < ((Ktot * es + 127) / 128) * 128) return DRN_ERR_ARG;  // weight rows zero-padded to 128-B slabs
  p = ConvParams{(const char*)x, (const char*)w, (char*)y, scale, bias, (const char*)residual, Nb, H, W, Cin, Ho, Wo,
                 Cout, KH, KW, stride, pad, dil, relu, Ktot, ldw, ldy, ldres, out_dtype, res_dtype, res_mult, t.fp8_k64};
  return DRN_OK;
}

}  // namespace

extern "C" {

// The tail of a 64-channel bottleneck on a large map as ONE launch (conv3x3_c64_kernel<.., PW, POOL>): the 3x3's output never
// goes to memory; w3 == NULL: no 1x1 stage (y has 64 channels, the residual - if any - too); pool: MaxPool2d(2, 2) in the
// epilogue (needs the last ReLU).  Same shape class as the LDS-resident-patch kernel takes on its own; anything else:
// DRN_ERR_UNSUPPORTED (the caller runs the separate launches).
int drn_conv3x3_pw_nhwc(const void* x, const void* w2, const float* scale2, const float* bias2, int relu2, const void* w3,
                        const float* scale3, const float* bias3, const void* residual, void* y, int Nb, int H, int W,
                        long ldw2, long ldw3, float res_mult, int relu3, int pool, void* stream) {
  if (!x || !w2 || !y || Nb <= 0 || H <= 0 || W <= 0) return DRN_ERR_ARG;
  if (!patch_c64_ok(g_tune, (long)H * W, w2, ldw2, y, residual) || (long)Nb * H * W * 128 >= 0xFFFFFFF0L || ldw2 < 9 * 64 ||
      (w3 && ldw3 < 64) || (w3 && (ldw3 * 2) % 16 != 0) || !al16(x) || (w3 && !al16(w3)) || (!w3 && !pool) ||
      (pool && (!(w3 ? relu3 : relu2) || H < 2 || W < 2)))
    return DRN_ERR_UNSUPPORTED;
  const int cy = w3 ? 256 : 64;
  ConvParams p{(const char*)x, (const char*)w2, (char*)y, scale2, bias2, (const char*)residual, Nb, H, W, 64, H, W,
               64, 3, 3, 1, 1, 1, relu2, 9 * 64, ldw2, cy, cy, DRN_BF16, DRN_BF16, res_mult, 0,
               (const char*)w3, ldw3, scale3, bias3, relu3, pool};
  return launch_conv3x3_c64_pw(p, (hipStream_t)stream);
}

// NHWC conv + per-channel affine (folded FrozenBN or bias) + optional residual + optional ReLU; `dtype` is the element
// type of x / w (fp32, bf16 or fp8 e4m3fn), y and the residual may be stored in another one (see include/drn_wsod.h).
int drn_conv2d_nhwc_q(const void* x, const void* w, void* y, const float* scale, const float* bias,
                      const void* residual, int Nb, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                      int pad, int dil, long ldw, long ldy, long ldres, int relu, int dtype, int out_dtype,
                      int res_dtype, float res_mult, void* stream) {
  ConvParams p;
  const int rc = conv_params(x, w, y, scale, bias, residual, Nb, H, W, Cin, Cout, KH, KW, stride, pad, dil, ldw, ldy, ldres, relu,
                             dtype, out_dtype, res_dtype, res_mult, g_tune, p);
  if (rc != DRN_OK) return rc;
  return conv_fwd_launch(conv_fwd_plan(p, dtype, g_tune, cu_count()), p, (hipStream_t)stream);
}

// Host-only: the kernel drn_conv2d_nhwc_q would run these arguments on, under the knobs as they stand, on a device of `cus`
// compute units (<= 0: this device's).  No launch, no device memory touched.  See include/drn_wsod.h.
int drn_conv2d_plan(const void* x, const void* w, void* y, const float* scale, const float* bias, const void* residual, int Nb,
                    int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil, long ldw, long ldy, long ldres,
                    int relu, int dtype, int out_dtype, int res_dtype, float res_mult, int cus) {
  ConvParams p;
  const int rc = conv_params(x, w, y, scale, bias, residual, Nb, H, W, Cin, Cout, KH, KW, stride, pad, dil, ldw, ldy, ldres, relu,
                             dtype, out_dtype, res_dtype, res_mult, g_tune, p);
  if (rc != DRN_OK) return rc;
  const ConvPlan pl = conv_fwd_plan(p, dtype, g_tune, cus > 0 ? cus : cu_count());
  return pl.kind | (pl.k64 ? 0 : DRN_CONV_KIND_FP8_K16);
}

int drn_conv2d_nhwc(const void* x, const void* w, void* y, const float* scale, const float* bias,
                    const void* residual, int Nb, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                    int pad, int dil, long ldw, long ldy, long ldres, int relu, int dtype, void* stream) {
  if (dtype != DRN_F32 && dtype != DRN_BF16) return DRN_ERR_ARG;
  return drn_conv2d_nhwc_q(x, w, y, scale, bias, residual, Nb, H, W, Cin, Cout, KH, KW, stride, pad, dil, ldw, ldy, ldres,
                           relu, dtype, dtype, dtype, 1.0f, stream);
}

}  // extern "C"
