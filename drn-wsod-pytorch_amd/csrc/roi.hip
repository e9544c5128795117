// RoI pooling for gfx950: RoIPool / ROIAlign forward, fused with the OICR objectness scaling and written straight into the fc6
// GEMM operand layout ([roi][c*P*P + bin] rows, the reference's NCHW flatten order, box_head.py:85-86), and their backward, atomic
// and deterministic.  NHWC maps.  Built with -ffp-contract=off: the arithmetic is the oracle's, op for op.
// Top down: the kernels; roi_fwd_plan - the ONE place that says which forward kernel pools a shape, with which template
// arguments and geometry - and roi_fwd_launch, which issues what a plan says; the entry points.
// Replaces: torchvision RoIPool (detectron2/modeling/poolers.py:162-165), ROIAlign (detectron2/layers/csrc/ROIAlign/
// ROIAlign_cuda.cu:65-250) and the objectness scaling of roi_heads_oicr.py:342-343.
#include "drn_common.h"
#include "tune.h"
#include "../../include/drn_wsod.h"
#include <float.h>
#include <stdio.h>

namespace {

struct RoiParams {
  const char* feat;  // NHWC
  const float* rois;  // [M][5]
  const float* obj;   // [M] objectness logits or null; output is scaled by (obj + 1)
  char* out;          // [M][ld_out], k = c*P*P + ph*P + pw
  int32_t* argmax;    // [M][C*P*P] (h*W + w, or -1) or null  (ROIPool only)
  int N, H, W, C, P, M;
  float scale;
  long ld_out;
  int sampling_ratio, aligned;
  int lds_px;  // pixels of staging LDS available per block (0 = direct path only)
  char* out_t;   // optional transposed copy [C*P*P][ld_out_t] (column = roi), or null
  long ld_out_t;
  int gpw;       // whole-map kernel: consecutive 8-ROI groups handled by one block (per staged map slice)
  int cpb;       // 64-ROI kernel: consecutive 8-channel chunks handled by one block (bin bounds computed once per block)
  int pf;        // 64-ROI kernel: two map buffers, the next chunk's slice is fetched under this chunk's scan
  int t_c0;      // first channel whose rows of out_t are needed (drn_roi_pool_nhwc_t); kernels may write more
  int c_begin;   // 64-ROI kernel: first channel it handles (the lane-per-bin kernel writes A; this one then only the A^T tail)
  int lane_g;    // lane-per-bin kernel: ROIs per group (one ROI per lane of every wave: <= 64)
  int lane_reps;  // lane-per-bin kernel: groups a block walks with ONE staged slice (large maps: the staging is L2 traffic ~ groups x map)
  int walk;       // walking lane-per-bin kernel: consecutive channel chunks a block walks with ONE window table of its ROIs
  int walk_wp;    // its LDS row pitch in cells (odd)
  const char* cm;  // its chunk-major, order-mapped copy of the map ([N][C/8][H*W] cells of 16 bytes) or null
  unsigned walk_wmagic;  // ceil(2^32 / W): pixel -> row by one v_mul_hi
};

constexpr int RP_CH = 64;    // channels per block = one wave-wide line of NHWC
constexpr int RP_MAXBIN = 64;  // P*P <= 64 (P <= 8)

// torchvision RoIPool's box arithmetic - ONE copy: every RoIPool kernel, forward and backward, takes its
// windows from these two, so no two of them can disagree about a bin (the op has no torchvision here to be pinned against).
// The box on the map: its first column / row and its extent in cells (>= 1).
__device__ __forceinline__ void roi_box(const float* roi, float scale, int& x1, int& y1, int& rw, int& rh) {
  x1 = (int)roundf(roi[1] * scale), y1 = (int)roundf(roi[2] * scale);
  const int x2 = (int)roundf(roi[3] * scale), y2 = (int)roundf(roi[4] * scale);
  rw = max(x2 - x1 + 1, 1), rh = max(y2 - y1 + 1, 1);
}
// [s, e) of bin i along one axis: bins of `bin` cells counted from `origin`, clamped to the map's [0, limit]
__device__ __forceinline__ void roi_bin(int i, float bin, int origin, int limit, int& s, int& e) {
  s = min(max((int)floorf((float)i * bin) + origin, 0), limit);
  e = min(max((int)ceilf((float)(i + 1) * bin) + origin, 0), limit);
}

// ROIAlign's box and sampling grid (ROIAlign_cuda.cu:65-139): one copy for the forward and both backward kernels
struct RoiAlignGeom { float sh, sw, bin_h, bin_w, count; int gh, gw; };
__device__ __forceinline__ RoiAlignGeom roi_align_geom(const float* roi, float scale, int aligned, int P, int sampling_ratio) {
  RoiAlignGeom g;
  const float off = aligned ? 0.5f : 0.f;
  g.sw = roi[1] * scale - off; g.sh = roi[2] * scale - off;
  const float ew = roi[3] * scale - off, eh = roi[4] * scale - off;
  float rw = ew - g.sw, rh = eh - g.sh;
  if (!aligned) { rw = fmaxf(rw, 1.f); rh = fmaxf(rh, 1.f); }
  g.bin_h = rh / (float)P; g.bin_w = rw / (float)P;
  g.gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / P);
  g.gw = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rw / P);
  g.count = (float)(g.gh * g.gw);
  return g;
}

// MODE 0: RoIPool   MODE 1: ROIAlign (ROIAlign_cuda.cu:65-139 semantics)
template <int DT_IN, int DT_OUT, int MODE>
__global__ __launch_bounds__(256) void roi_kernel(RoiParams p) {
  using EI = ElemOf<DT_IN>;
  using TI = typename EI::type;
  using EO = ElemOf<DT_OUT>;
  using TO = typename EO::type;
  __shared__ float tile[RP_CH][RP_MAXBIN + 1];
  __shared__ int atile[RP_CH][RP_MAXBIN + 1];
  const int m = blockIdx.x;
  const int c0 = blockIdx.y * RP_CH;
  const int cl = threadIdx.x & 63, bg = threadIdx.x >> 6;  // lane = channel, 4 bin groups
  const int c = c0 + cl;
  const float* roi = p.rois + 5 * (long)m;
  const int b = (int)roi[0];
  const int PP = p.P * p.P;
  const float mul = p.obj ? p.obj[m] + 1.f : 1.f;
  const TI* fb = (const TI*)p.feat + (long)b * p.H * p.W * p.C;
  if (MODE == 0) {
    int x1, y1, rw, rh;
    roi_box(roi, p.scale, x1, y1, rw, rh);
    const float bin_h = (float)rh / (float)p.P, bin_w = (float)rw / (float)p.P;
    // LDS path: the union of all bins is the clipped box [y1, y1+rh) x [x1, x1+rw); stage those pixels of this
    // block's 64 channels with 16-B loads (all independent => all in flight), then scan bins out of LDS.
    const int ry0 = min(max(y1, 0), p.H), ry1 = min(max(y1 + rh, 0), p.H);
    const int rx0 = min(max(x1, 0), p.W), rx1 = min(max(x1 + rw, 0), p.W);
    const int rww = rx1 - rx0, npx = (ry1 - ry0) * rww;
    if (p.lds_px > 0 && npx <= p.lds_px && c0 + RP_CH <= p.C) {
      extern __shared__ __attribute__((aligned(16))) char stage[];
      constexpr int ESI = DT_IN == DRN_BF16 ? 2 : 4;
      constexpr int VPL = RP_CH * ESI / 16;  // lanes (16 B each) per pixel
      for (int i = threadIdx.x; i < npx * VPL; i += 256) {
        const int px = i / VPL, v = i - px * VPL;
        const int h = ry0 + px / rww, w = rx0 + px % rww;
        *(i32x4_t*)(stage + ((long)px * RP_CH) * ESI + v * 16) =
            *(const i32x4_t*)((const char*)(fb + ((long)h * p.W + w) * p.C + c0) + v * 16);
      }
      __syncthreads();
      const TI* st = (const TI*)stage;
      for (int bin = bg; bin < PP; bin += 4) {
        const int ph = bin / p.P, pw = bin - ph * p.P;
        int hs, he, ws, we;
        roi_bin(ph, bin_h, y1, p.H, hs, he);
        roi_bin(pw, bin_w, x1, p.W, ws, we);
        const bool empty = he <= hs || we <= ws;
        float best = empty ? 0.f : -FLT_MAX;
        int besti = -1;
        for (int h = hs; h < he; ++h)
          for (int w = ws; w < we; ++w) {
            const float v = EI::ld(st + ((h - ry0) * rww + (w - rx0)) * RP_CH + cl);
            if (v > best) { best = v; besti = h * p.W + w; }
          }
        tile[cl][bin] = best * mul;
        atile[cl][bin] = besti;
      }
    } else
    for (int bin = bg; bin < PP; bin += 4) {
      const int ph = bin / p.P, pw = bin - ph * p.P;
      int hs, he, ws, we;
      roi_bin(ph, bin_h, y1, p.H, hs, he);
      roi_bin(pw, bin_w, x1, p.W, ws, we);
      const bool empty = he <= hs || we <= ws;
      float best = empty ? 0.f : -FLT_MAX;
      int besti = -1;
      if (c < p.C)
        for (int h = hs; h < he; ++h)
          for (int w = ws; w < we; ++w) {
            const float v = EI::ld(fb + ((long)h * p.W + w) * p.C + c);
            if (v > best) { best = v; besti = h * p.W + w; }
          }
      tile[cl][bin] = best * mul;
      atile[cl][bin] = besti;
    }
  } else {
    const RoiAlignGeom g = roi_align_geom(roi, p.scale, p.aligned, p.P, p.sampling_ratio);
    const float sw = g.sw, sh = g.sh, bin_h = g.bin_h, bin_w = g.bin_w, count = (float)max(g.gh * g.gw, 1);
    const int gh = g.gh, gw = g.gw;
    for (int bin = bg; bin < PP; bin += 4) {
      const int ph = bin / p.P, pw = bin - ph * p.P;
      float acc = 0.f;
      for (int iy = 0; iy < gh; ++iy) {
        const float yy = sh + ph * bin_h + (float)(iy + .5f) * bin_h / (float)gh;
        for (int ix = 0; ix < gw; ++ix) {
          const float xx = sw + pw * bin_w + (float)(ix + .5f) * bin_w / (float)gw;
          float x = xx, y = yy;
          if (y < -1.0f || y > p.H || x < -1.0f || x > p.W) continue;
          if (y <= 0) y = 0;
          if (x <= 0) x = 0;
          int yl = (int)y, xl = (int)x, yh, xh;
          if (yl >= p.H - 1) { yh = yl = p.H - 1; y = (float)yl; } else yh = yl + 1;
          if (xl >= p.W - 1) { xh = xl = p.W - 1; x = (float)xl; } else xh = xl + 1;
          const float ly = y - yl, lx = x - xl, hy = 1.f - ly, hx = 1.f - lx;
          if (c < p.C) {
            const float v1 = EI::ld(fb + ((long)yl * p.W + xl) * p.C + c), v2 = EI::ld(fb + ((long)yl * p.W + xh) * p.C + c);
            const float v3 = EI::ld(fb + ((long)yh * p.W + xl) * p.C + c), v4 = EI::ld(fb + ((long)yh * p.W + xh) * p.C + c);
            acc += hy * hx * v1 + hy * lx * v2 + ly * hx * v3 + ly * lx * v4;
          }
        }
      }
      tile[cl][bin] = acc / count * mul;
    }
  }
  __syncthreads();
  // coalesced write-out: k = c*PP + bin is contiguous over this block's 64 channels
  const int nvalid = min(RP_CH, p.C - c0) * PP;
  TO* orow = (TO*)p.out + (long)m * p.ld_out + (long)c0 * PP;
  constexpr int ESO = DT_OUT == DRN_BF16 ? 2 : 4;
  constexpr int VE = 16 / ESO;  // elements per 16-B store
  if ((nvalid % VE) == 0 && ((((long)m * p.ld_out + (long)c0 * PP) * ESO) & 15) == 0 && (((uintptr_t)p.out) & 15) == 0) {
    for (int v = threadIdx.x; v < nvalid / VE; v += 256) {
      float f[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const int i = v * VE + e, lc = i / PP;
        f[e] = tile[lc][i - lc * PP];
      }
      i32x4_t o;
      if constexpr (DT_OUT == DRN_BF16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (int)((uint32_t)f32_to_bf16(f[2 * e]) | ((uint32_t)f32_to_bf16(f[2 * e + 1]) << 16));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __builtin_bit_cast(int, f[e]);
      }
      *(i32x4_t*)((char*)orow + (long)v * 16) = o;
    }
  } else {
    for (int i = threadIdx.x; i < nvalid; i += 256) {
      const int lc = i / PP;
      EO::st(orow + i, tile[lc][i - lc * PP]);
    }
  }
  if (MODE == 0 && p.argmax)
    for (int i = threadIdx.x; i < nvalid; i += 256) {
      const int lc = i / PP;
      p.argmax[(long)m * p.C * PP + (long)c0 * PP + i] = atile[lc][i - lc * PP];
    }
}

// Backward of RoIPool (MODE 0: scatter to the saved arg-max) / ROIAlign (MODE 1: bilinear scatter,
// ROIAlign_cuda.cu:141-250 semantics), fused with the objectness scaling of the forward.  One block = one ROI x 64
// channels like roi_kernel: the [64 x P*P] slice of grad_out is read coalesced into LDS, then lane = channel scatters
// with fp32 atomics into the NHWC gradient map - neighbouring lanes hit neighbouring addresses.  Like the
// reference's CUDA kernels the accumulation order is not fixed (only used when the backbone trains).
struct RoiBwdParams {
  const char* grad_out;  // [M][ld], k = c*P*P + bin
  const float* rois; const float* obj; const int32_t* argmax;
  float* dfeat;          // [N][H][W][C] fp32, zeroed by the launcher
  int N, H, W, C, P, M; float scale; long ld; int sampling_ratio, aligned;
};

template <int DT, int MODE>
__global__ __launch_bounds__(256) void roi_bwd_kernel(RoiBwdParams p) {
  using E = ElemOf<DT>;
  using T = typename E::type;
  __shared__ float tile[RP_CH][RP_MAXBIN + 1];
  __shared__ int atile[RP_CH][RP_MAXBIN + 1];
  const int m = blockIdx.x, c0 = blockIdx.y * RP_CH;
  const int cl = threadIdx.x & 63, bg = threadIdx.x >> 6;
  const int c = c0 + cl;
  const float* roi = p.rois + 5 * (long)m;
  const int b = (int)roi[0];
  const int PP = p.P * p.P;
  const float mul = p.obj ? p.obj[m] + 1.f : 1.f;
  const int nvalid = min(RP_CH, p.C - c0) * PP;
  const T* grow = (const T*)p.grad_out + (long)m * p.ld + (long)c0 * PP;
  for (int i = threadIdx.x; i < nvalid; i += 256) {
    const int lc = i / PP;
    tile[lc][i - lc * PP] = E::ld(grow + i) * mul;
    if (MODE == 0) atile[lc][i - lc * PP] = p.argmax[(long)m * p.C * PP + (long)c0 * PP + i];
  }
  __syncthreads();
  if (c >= p.C) return;
  float* gb = p.dfeat + (long)b * p.H * p.W * p.C + c;
  if (MODE == 0) {
    for (int bin = bg; bin < PP; bin += 4) {
      const int a = atile[cl][bin];
      if (a >= 0) atomicAdd(gb + (long)a * p.C, tile[cl][bin]);
    }
  } else {
    const RoiAlignGeom g = roi_align_geom(roi, p.scale, p.aligned, p.P, p.sampling_ratio);
    const float sw = g.sw, sh = g.sh, bin_h = g.bin_h, bin_w = g.bin_w, count = g.count;
    const int gh = g.gh, gw = g.gw;
    for (int bin = bg; bin < PP; bin += 4) {
      const int ph = bin / p.P, pw = bin - ph * p.P;
      const float g = tile[cl][bin];
      for (int iy = 0; iy < gh; ++iy) {
        const float yy = sh + ph * bin_h + (float)(iy + .5f) * bin_h / (float)gh;
        for (int ix = 0; ix < gw; ++ix) {
          const float xx = sw + pw * bin_w + (float)(ix + .5f) * bin_w / (float)gw;
          float x = xx, y = yy;
          if (y < -1.0f || y > p.H || x < -1.0f || x > p.W) continue;
          if (y <= 0) y = 0;
          if (x <= 0) x = 0;
          int yl = (int)y, xl = (int)x, yh, xh;
          if (yl >= p.H - 1) { yh = yl = p.H - 1; y = (float)yl; } else yh = yl + 1;
          if (xl >= p.W - 1) { xh = xl = p.W - 1; x = (float)xl; } else xh = xl + 1;
          const float ly = y - yl, lx = x - xl, hy = 1.f - ly, hx = 1.f - lx;
          atomicAdd(gb + ((long)yl * p.W + xl) * p.C, g * (hy * hx) / count);
          atomicAdd(gb + ((long)yl * p.W + xh) * p.C, g * (hy * lx) / count);
          atomicAdd(gb + ((long)yh * p.W + xl) * p.C, g * (ly * hx) / count);
          atomicAdd(gb + ((long)yh * p.W + xh) * p.C, g * (ly * lx) / count);
        }
      }
    }
  }
}

// ---- the same backward with a FIXED accumulation order and no atomics (drn_roi_pool_backward_det_nhwc) --------
// dfeat[b, y, x, c] = +0.0f plus the contributions that land on it, added one at a time in ascending (ROI m, bin =
// ph*P + pw) order - for ROIAlign then iy, ix and the taps (yl,xl), (yl,xh), (yh,xl), (yh,xh) - each contribution
// rounded to fp32 before it is added (the scaled gradient sits in LDS as fp32; this file is built without contraction).
// For RoIPool that is the order of the oracle's sequential scatter, so the result equals it bit for bit.
// Every accumulator has ONE owner: the map is cut into T x T pixel tiles, a workgroup (one wave, lane = channel) owns
// one tile of one image for 64 channels, keeps the [T*T][64] fp32 accumulator in LDS and STORES it at the end - every
// element of dfeat is written exactly once, zeros included, so there is no memset either.
//   pass 1 (roi_det_list_kernel): one wave per (image, tile) walks the ROIs in ascending order, 64 per round; a lane
//     keeps its ROI if it is of that image and some bin can reach the tile; one ballot + a prefix popcount per round
//     compact the survivors, so the list comes out ascending with no sort and no atomic.  An entry is (m, the bin rows
//     that can reach the tile as a bit mask | the bin columns << 8): RoIPool from the forward's own window bounds (the
//     arg-max of a bin lies in its window), ROIAlign from the bin's sample extent widened by two pixels (a superset -
//     only taps inside the tile are ever added).
//   pass 2 (roi_bwd_det_kernel): walks its tile's list in order; per entry the rows [first, last masked bin row] of the
//     64-channel slice of grad_out are staged into LDS with coalesced reads (a large ROI on a large map is not re-read
//     whole by every tile it covers), RoIPool's arg-max is turned into a tile-local pixel (or "not mine") on the way;
//     then lane = channel walks the masked bins in ascending order and adds into its own LDS column.
// Workspace: tiles(4) records of (M + 1) 8-byte entries, entry 0 = the count (drn_roi_backward_det_ws_bytes); the tile
// edge is 4 when 8 would leave fewer than 256 workgroups (a 14x14 map), else 8 - the result does not depend on it.
struct RoiDetParams {
  const char* grad_out; const float* rois; const float* obj; const int32_t* argmax; float* dfeat;
  int2* ws;
  int N, H, W, C, P, M; float scale; long ld; int sampling_ratio, aligned;
  int tiles_y, tiles_x;
  unsigned wmagic;  // ceil(2^32 / W) (W >= 2): offset inside a tile's rows -> row by one v_mul_hi
};

template <int MODE, int T>
__global__ __launch_bounds__(64) void roi_det_list_kernel(RoiDetParams p) {
  const int lane = threadIdx.x;
  const int id = blockIdx.x, per = p.tiles_y * p.tiles_x;
  const int b = id / per, t = id - b * per;
  const int ty0 = (t / p.tiles_x) * T, tx0 = (t % p.tiles_x) * T;
  const int ty1 = min(ty0 + T, p.H), tx1 = min(tx0 + T, p.W);
  int2* rec = p.ws + (long)id * (p.M + 1);
  int n = 0;
  for (int m0 = 0; m0 < p.M; m0 += 64) {
    const int m = m0 + lane;
    unsigned hmask = 0, wmask = 0;
    if (m < p.M) {
      const float* roi = p.rois + 5 * (long)m;
      if ((int)roi[0] == b) {
        if (MODE == 0) {
          int x1, y1, rw, rh;
          roi_box(roi, p.scale, x1, y1, rw, rh);
          const float bin_h = (float)rh / (float)p.P, bin_w = (float)rw / (float)p.P;
          for (int i = 0; i < p.P; ++i) {  // the forward's window bounds: the forward's own helpers
            int hs, he, ws, we;
            roi_bin(i, bin_h, y1, p.H, hs, he);
            roi_bin(i, bin_w, x1, p.W, ws, we);
            if (max(hs, ty0) < min(he, ty1)) hmask |= 1u << i;
            if (max(ws, tx0) < min(we, tx1)) wmask |= 1u << i;
          }
        } else {
          const RoiAlignGeom g = roi_align_geom(roi, p.scale, p.aligned, p.P, p.sampling_ratio);
          if (g.gh > 0 && g.gw > 0)
            for (int i = 0; i < p.P; ++i) {
              // every sample of bin row i lies between its two edges (up to rounding); its taps are floor(y), floor(y) + 1
              const float ya = g.sh + i * g.bin_h, yb = g.sh + (i + 1) * g.bin_h;
              const float xa = g.sw + i * g.bin_w, xb = g.sw + (i + 1) * g.bin_w;
              const float ylo = fminf(fmaxf(fminf(ya, yb), -2.f), (float)p.H + 2.f), yhi = fminf(fmaxf(fmaxf(ya, yb), -2.f), (float)p.H + 2.f);
              const float xlo = fminf(fmaxf(fminf(xa, xb), -2.f), (float)p.W + 2.f), xhi = fminf(fmaxf(fmaxf(xa, xb), -2.f), (float)p.W + 2.f);
              if ((int)floorf(ylo) - 1 < ty1 && (int)floorf(yhi) + 2 >= ty0) hmask |= 1u << i;
              if ((int)floorf(xlo) - 1 < tx1 && (int)floorf(xhi) + 2 >= tx0) wmask |= 1u << i;
            }
        }
      }
    }
    const bool keep = hmask != 0 && wmask != 0;
    const unsigned long long bal = __ballot(keep);
    if (keep) rec[1 + n + __popcll(bal & ((1ull << lane) - 1ull))] = make_int2(m, (int)(hmask | (wmask << 8)));
    n += __popcll(bal);
  }
  if (lane == 0) rec[0] = make_int2(n, 0);
}

template <int DT, int MODE, int T>
__global__ __launch_bounds__(64) void roi_bwd_det_kernel(RoiDetParams p) {
  using E = ElemOf<DT>;
  using TG = typename E::type;
  constexpr int NOT_MINE = 255;
  __shared__ float acc[T * T][RP_CH];               // lane = channel: conflict-free
  __shared__ float tile[RP_CH][RP_MAXBIN + 1];      // the scaled gradients, fp32
  __shared__ unsigned char apix[MODE == 0 ? RP_CH : 1][RP_MAXBIN + 4];  // RoIPool: tile-local arg-max pixel; 17-word pitch
  const int lane = threadIdx.x;
  const int id = blockIdx.x, per = p.tiles_y * p.tiles_x;
  const int b = id / per, t = id - b * per;
  const int ty0 = (t / p.tiles_x) * T, tx0 = (t % p.tiles_x) * T;
  const int th = min(T, p.H - ty0), tw = min(T, p.W - tx0);
  const int c0 = blockIdx.y * RP_CH, nch = min(RP_CH, p.C - c0);
  const int PP = p.P * p.P;
#pragma unroll
  for (int q = 0; q < T * T; ++q) acc[q][lane] = 0.f;
  const int2* rec = p.ws + (long)id * (p.M + 1);
  const int n = rec[0].x;
  const unsigned tbase = (unsigned)(ty0 * p.W + tx0), tspan = (unsigned)((th - 1) * p.W + tw);
  for (int e = 0; e < n; ++e) {
    const int2 ent = rec[1 + e];
    const int m = ent.x;
    const unsigned hmask = (unsigned)ent.y & 0xffu, wmask = ((unsigned)ent.y >> 8) & 0xffu;
    const int ph_lo = __builtin_ctz(hmask), ph_hi = 31 - __builtin_clz(hmask);
    const int off = ph_lo * p.P, L = (ph_hi - ph_lo + 1) * p.P;  // the staged run of every channel: bins [off, off + L)
    const float mul = p.obj ? p.obj[m] + 1.f : 1.f;
    const TG* grow = (const TG*)p.grad_out + (long)m * p.ld + (long)c0 * PP;
    const int32_t* arow = MODE == 0 ? p.argmax + (long)m * p.C * PP + (long)c0 * PP : nullptr;
    __syncthreads();  // the previous entry's walk no longer reads the staging tiles
    const float inv_l = 1.f / (float)L;
    for (int i = lane; i < nch * L; i += 64) {
      const int lc = (int)(((float)i + 0.5f) * inv_l);  // i / L: i < 4096, L <= 64 - the product is >= 1/128 away from an integer
      const int j = off + (i - lc * L);
      tile[lc][j] = E::ld(grow + lc * PP + j) * mul;
      if constexpr (MODE == 0) {
        // arg-max (h*W + w) -> pixel of this tile, or NOT_MINE (also for -1 and for anything outside the map)
        const unsigned u = (unsigned)arow[lc * PP + j] - tbase;
        int q = NOT_MINE;
        if (u < tspan) {
          const unsigned r = p.W > 1 ? __umulhi(u, p.wmagic) : u, x = u - r * (unsigned)p.W;
          if (x < (unsigned)tw) q = (int)(r * T + x);
        }
        apix[lc][j] = (unsigned char)q;
      }
    }
    __syncthreads();
    if (lane < nch) {
      if constexpr (MODE == 0) {
        for (int ph = ph_lo; ph <= ph_hi; ++ph)
          for (unsigned wm = wmask; wm; wm &= wm - 1) {
            const int bin = ph * p.P + __builtin_ctz(wm);
            const int q = apix[lane][bin];
            if (q != NOT_MINE) acc[q][lane] += tile[lane][bin];
          }
      } else {
        const RoiAlignGeom g = roi_align_geom(p.rois + 5 * (long)m, p.scale, p.aligned, p.P, p.sampling_ratio);
        for (int ph = ph_lo; ph <= ph_hi; ++ph) {
          if (!((hmask >> ph) & 1u)) continue;
          for (unsigned wm = wmask; wm; wm &= wm - 1) {
            const int pw = __builtin_ctz(wm);
            const float gv = tile[lane][ph * p.P + pw];
            for (int iy = 0; iy < g.gh; ++iy) {
              const float yy = g.sh + ph * g.bin_h + (float)(iy + .5f) * g.bin_h / (float)g.gh;
              for (int ix = 0; ix < g.gw; ++ix) {
                const float xx = g.sw + pw * g.bin_w + (float)(ix + .5f) * g.bin_w / (float)g.gw;
                float x = xx, y = yy;
                if (y < -1.0f || y > p.H || x < -1.0f || x > p.W) continue;
                if (y <= 0) y = 0;
                if (x <= 0) x = 0;
                int yl = (int)y, xl = (int)x, yh, xh;
                if (yl >= p.H - 1) { yh = yl = p.H - 1; y = (float)yl; } else yh = yl + 1;
                if (xl >= p.W - 1) { xh = xl = p.W - 1; x = (float)xl; } else xh = xl + 1;
                const float ly = y - yl, lx = x - xl, hy = 1.f - ly, hx = 1.f - lx;
                const unsigned ryl = (unsigned)(yl - ty0), ryh = (unsigned)(yh - ty0);
                const unsigned rxl = (unsigned)(xl - tx0), rxh = (unsigned)(xh - tx0);
                const bool iyl = ryl < (unsigned)th, iyh = ryh < (unsigned)th, ixl = rxl < (unsigned)tw, ixh = rxh < (unsigned)tw;
                if (iyl && ixl) acc[ryl * T + rxl][lane] += gv * (hy * hx) / g.count;
                if (iyl && ixh) acc[ryl * T + rxh][lane] += gv * (hy * lx) / g.count;
                if (iyh && ixl) acc[ryh * T + rxl][lane] += gv * (ly * hx) / g.count;
                if (iyh && ixh) acc[ryh * T + rxh][lane] += gv * (ly * lx) / g.count;
              }
            }
          }
        }
      }
    }
  }
  if (lane < nch) {
    float* ob = p.dfeat + (((long)b * p.H + ty0) * p.W + tx0) * p.C + c0 + lane;
    for (int r = 0; r < th; ++r)
      for (int x = 0; x < tw; ++x) ob[((long)r * p.W + x) * p.C] = acc[r * T + x][lane];
  }
}

// ROIPool specialised for the 7x7 pooler every DRN-WSOD config uses.  One block = one ROI x 256 channels (four
// 64-channel chunks, so the ROI geometry, the 49 bin rectangles and the window's pixel table are computed once);
// per chunk the window pixels are staged in LDS by 16-B loads, the bin maxima come out of LDS, and the
// [c*49 + bin] run (64*49 contiguous outputs) leaves in 16-B stores.  All divisions are by constants.
template <int DT_IN, int DT_OUT>
__global__ __launch_bounds__(256) void roi_pool7_kernel(RoiParams p) {
  using EI = ElemOf<DT_IN>;
  using TI = typename EI::type;
  using EO = ElemOf<DT_OUT>;
  using TO = typename EO::type;
  constexpr int PP = 49, CHUNKS = 4;
  constexpr int ESI = DT_IN == DRN_BF16 ? 2 : 4, ESO = DT_OUT == DRN_BF16 ? 2 : 4;
  constexpr int VPL = RP_CH * ESI / 16, VE = 16 / ESO;
  extern __shared__ __attribute__((aligned(16))) char stage[];  // [lds_px][64] TI
  __shared__ float tile[RP_CH][PP + 1];
  __shared__ int bins[PP][4];
  __shared__ int pxoff[256];
  const int m = blockIdx.x;
  const int cl = threadIdx.x & 63, bg = threadIdx.x >> 6;
  const float* roi = p.rois + 5 * (long)m;
  const int b = (int)roi[0];
  const float mul = p.obj ? p.obj[m] + 1.f : 1.f;
  const TI* fb = (const TI*)p.feat + (long)b * p.H * p.W * p.C;
  int x1, y1, rw, rh;
  roi_box(roi, p.scale, x1, y1, rw, rh);
  const float bin_h = (float)rh / 7.f, bin_w = (float)rw / 7.f;
  const int ry0 = min(max(y1, 0), p.H), ry1 = min(max(y1 + rh, 0), p.H);
  const int rx0 = min(max(x1, 0), p.W), rx1 = min(max(x1 + rw, 0), p.W);
  const int rww = rx1 - rx0, npx = (ry1 - ry0) * rww;  // npx <= lds_px <= 256 guaranteed by the launcher
  if (threadIdx.x < PP) {
    const int ph = threadIdx.x / 7, pw = threadIdx.x - ph * 7;
    roi_bin(ph, bin_h, y1, p.H, bins[threadIdx.x][0], bins[threadIdx.x][1]);
    roi_bin(pw, bin_w, x1, p.W, bins[threadIdx.x][2], bins[threadIdx.x][3]);
  }
  if (threadIdx.x < npx) {
    const int hh = threadIdx.x / rww;
    pxoff[threadIdx.x] = (ry0 + hh) * p.W + rx0 + (threadIdx.x - hh * rww);
  }
  __syncthreads();
  for (int ch = 0; ch < CHUNKS; ++ch) {
    const int c0 = (blockIdx.y * CHUNKS + ch) * RP_CH;
    if (c0 >= p.C) break;
    for (int i = threadIdx.x; i < npx * VPL; i += 256) {
      const int px = i / VPL, v = i - px * VPL;
      *(i32x4_t*)(stage + (long)px * (RP_CH * ESI) + v * 16) =
          *(const i32x4_t*)((const char*)(fb + (long)pxoff[px] * p.C + c0) + v * 16);
    }
    __syncthreads();
    const TI* st = (const TI*)stage;
    for (int bin = bg; bin < PP; bin += 4) {
      const int hs = bins[bin][0], he = bins[bin][1], ws = bins[bin][2], we = bins[bin][3];
      float best = (he <= hs || we <= ws) ? 0.f : -FLT_MAX;
      for (int h = hs; h < he; ++h)
        for (int w = ws; w < we; ++w) best = fmaxf(best, EI::ld(st + ((h - ry0) * rww + (w - rx0)) * RP_CH + cl));
      tile[cl][bin] = best * mul;
    }
    __syncthreads();
    char* orow = (char*)((TO*)p.out + (long)m * p.ld_out + (long)c0 * PP);
    for (int v = threadIdx.x; v < RP_CH * PP / VE; v += 256) {
      float f[VE];
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const int i = v * VE + e, lc = i / PP;
        f[e] = tile[lc][i - lc * PP];
      }
      i32x4_t o;
      if constexpr (DT_OUT == DRN_BF16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (int)((uint32_t)f32_to_bf16(f[2 * e]) | ((uint32_t)f32_to_bf16(f[2 * e + 1]) << 16));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __builtin_bit_cast(int, f[e]);
      }
      *(i32x4_t*)(orow + (long)v * 16) = o;
    }
    __syncthreads();
  }
}

// 7x7 ROIPool, whole-map variant: when a CH-channel slice of one image's feature map fits in LDS (C4/DC5 maps of
// VOC-sized images: 14x14 .. 28x28 pixels) a block stages that slice ONCE and pools ROI_GROUP = 8 consecutive ROIs
// out of it - no per-ROI trip to L2, two barriers per block instead of three per (ROI, chunk).  The [8][CH*49] result
// tile leaves LDS twice: as the 8 row runs of A (16-B stores, k = c*49 + bin) and, when out_t is given, as CH*49
// 16-B column runs of A^T (8 ROIs wide), which replaces the separate 2 x 205 MB transpose pass of the fc6 operand.
// Block ids are XCD-remapped chunk-major, so the 8 blocks that complete one 128-B line of A^T share an XCD's L2.
// two packed bf16 -> two packed int16 with the same ordering (and back: the map is an involution); lets window
// maxima run as v_pk_max_i16 on whole 32-bit words.  -0 orders below +0, NaNs order as large magnitudes.
typedef short s16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int bf16x2_order(int x) {
  const s16x2_t v = __builtin_bit_cast(s16x2_t, x);
  const s16x2_t m = (v >> (short)15) & (short)0x7fff;
  return __builtin_bit_cast(int, (s16x2_t)(v ^ m));
}
__device__ __forceinline__ int pk_max_i16(int a, int b) {
  return __builtin_bit_cast(int, __builtin_elementwise_max(__builtin_bit_cast(s16x2_t, a), __builtin_bit_cast(s16x2_t, b)));
}

constexpr int ROI_GROUP = 8;
template <int DT, int CH>
__global__ __launch_bounds__(256) void roi_pool7_map_kernel(RoiParams p) {
  using E = ElemOf<DT>;
  using T = typename E::type;
  constexpr int PP = 49, ES = DT == DRN_BF16 ? 2 : 4;
  constexpr int RUN = CH * PP;       // outputs per ROI in this chunk
  constexpr int VPL = CH * ES / 16;  // 16-B vectors per pixel
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int HW = p.H * p.W;
  char* map = smem;                                          // [HW][CH]
  T* tile = (T*)(smem + (((long)HW * CH * ES + 15) & ~15L));  // [ROI_GROUP][RUN]
  __shared__ int hb[ROI_GROUP][7][2], wb[ROI_GROUP][7][2], bidx[ROI_GROUP];
  __shared__ float mulv[ROI_GROUP];
  const int ngroups = (p.M + ROI_GROUP - 1) / ROI_GROUP;
  const int nblk = (ngroups + p.gpw - 1) / p.gpw;  // blocks per channel chunk
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int chunk = logical / nblk, gblk = logical - chunk * nblk;
  const int c0 = chunk * CH;
  const int tid = threadIdx.x;
  const int r = tid >> 5, lane = tid & 31;
  int staged = -1;  // image whose map slice currently sits in LDS
  // several ROI groups per block share one staged map slice: for the large maps of test-time scales the slice is far
  // bigger than a group's output, and re-staging it per group was the whole cost
  for (int gi = 0; gi < p.gpw; ++gi) {
  const int group = gblk * p.gpw + gi;
  if (group >= ngroups) break;
  const int m0 = group * ROI_GROUP;
  const int nr = min(ROI_GROUP, p.M - m0);
  __syncthreads();  // the previous group's tile / bounds are no longer read
  if (tid < ROI_GROUP * 7) {
    const int r = tid / 7, i = tid - r * 7;
    if (r < nr) {
      const float* roi = p.rois + 5 * (long)(m0 + r);
      int x1, y1, rw, rh;
      roi_box(roi, p.scale, x1, y1, rw, rh);
      roi_bin(i, (float)rh / 7.f, y1, p.H, hb[r][i][0], hb[r][i][1]);
      roi_bin(i, (float)rw / 7.f, x1, p.W, wb[r][i][0], wb[r][i][1]);
      if (i == 0) {
        bidx[r] = (int)roi[0];
        mulv[r] = p.obj ? p.obj[m0 + r] + 1.f : 1.f;
      }
    }
  }
  __syncthreads();
  const int r = tid >> 5, lane = tid & 31;
  for (int r0 = 0; r0 < nr;) {  // one pass per run of ROIs on the same image (one pass unless a group straddles images)
    const int b = bidx[r0];
    int r1 = r0 + 1;
    while (r1 < nr && bidx[r1] == b) ++r1;
    if (b != staged) {  // uniform over the block
      const char* fb = p.feat + ((long)b * HW * p.C + c0) * ES;
      for (int i = tid; i < HW * VPL; i += 256) {
        const int px = i / VPL, v = i - px * VPL;
        i32x4_t x = *(const i32x4_t*)(fb + (long)px * p.C * ES + v * 16);
        if constexpr (DT == DRN_BF16) {
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] = bf16x2_order(x[e]);
        }
        *(i32x4_t*)(map + (long)i * 16) = x;
      }
      staged = b;
      __syncthreads();
    }
    if (r >= r0 && r < r1) {
      const float mul = mulv[r];
      T* trow = tile + (long)r * RUN;
      if constexpr (DT == DRN_BF16) {
        // lane = (channel octet, bin subset): one 16-B LDS read feeds four packed int16 maxima (8 channels)
        constexpr int NOCT = CH / 8, NSUB = 32 / NOCT;
        const int oct = lane % NOCT, bs = lane / NOCT;
        for (int bin = bs; bin < PP; bin += NSUB) {
          const int ph = bin / 7, pw = bin - ph * 7;
          const int hs = hb[r][ph][0], he = hb[r][ph][1], ws = wb[r][pw][0], we = wb[r][pw][1];
          const int lo = (int)0x80008000u;
          i32x4_t acc = {lo, lo, lo, lo};
          for (int h = hs; h < he; ++h) {
            const char* row = map + ((long)(h * p.W) * CH + oct * 8) * 2;
            for (int w = ws; w < we; ++w) {
              const i32x4_t x = *(const i32x4_t*)(row + (long)w * CH * 2);
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[e] = pk_max_i16(acc[e], x[e]);
            }
          }
          const bool empty = he <= hs || we <= ws;
          bf16_t* dst = trow + (oct * 8) * PP + bin;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t y = (uint32_t)bf16x2_order(acc[e]);
            const float f0 = empty ? 0.f : __builtin_bit_cast(float, y << 16);
            const float f1 = empty ? 0.f : __builtin_bit_cast(float, y & 0xffff0000u);
            dst[(2 * e) * PP] = f32_to_bf16(f0 * mul);
            dst[(2 * e + 1) * PP] = f32_to_bf16(f1 * mul);
          }
        }
      } else {
        for (int u = lane; u < CH * PP; u += 32) {
          const int bin = u / CH, cu = u - bin * CH;
          const int ph = bin / 7, pw = bin - ph * 7;
          const int hs = hb[r][ph][0], he = hb[r][ph][1], ws = wb[r][pw][0], we = wb[r][pw][1];
          float b0 = (he <= hs || we <= ws) ? 0.f : -FLT_MAX;
          for (int h = hs; h < he; ++h)
            for (int w = ws; w < we; ++w) b0 = fmaxf(b0, *(const float*)(map + ((long)(h * p.W + w) * CH + cu) * 4));
          trow[cu * PP + bin] = b0 * mul;
        }
      }
    }
    __syncthreads();
    r0 = r1;
  }
  // A rows: nr contiguous runs of RUN elements
  constexpr int VROW = RUN * ES / 16;
  for (int v = tid; v < nr * VROW; v += 256) {
    const int rr = v / VROW, q = v - rr * VROW;
    *(i32x4_t*)(p.out + ((long)(m0 + rr) * p.ld_out + (long)c0 * PP) * ES + (long)q * 16) =
        *(const i32x4_t*)((const char*)tile + ((long)rr * RUN * ES + (long)q * 16));
  }
  if (p.out_t) {
    T* ot = (T*)p.out_t + (long)c0 * PP * p.ld_out_t + m0;
    if (nr == ROI_GROUP) {  // launcher guarantees 16-B alignment of every 8-ROI run
      for (int idx = tid; idx < RUN; idx += 256) {
        T vals[ROI_GROUP];
#pragma unroll
        for (int rr = 0; rr < ROI_GROUP; ++rr) vals[rr] = tile[(long)rr * RUN + idx];
        i32x4_t* dst = (i32x4_t*)(ot + (long)idx * p.ld_out_t);
#pragma unroll
        for (int q = 0; q < ROI_GROUP * ES / 16; ++q) dst[q] = ((const i32x4_t*)vals)[q];
      }
    } else {
      for (int idx = tid; idx < RUN; idx += 256)
        for (int rr = 0; rr < nr; ++rr) ot[(long)idx * p.ld_out_t + rr] = tile[(long)rr * RUN + idx];
    }
  }
  }  // ROI groups of this block
}

// 7x7 ROIPool, whole-map variant for the training operand pair (A, A^T) in bf16: a block pools 64 consecutive ROIs out
// of an 8-channel slice of the map, so that every row of its A^T tile - 64 ROIs x 2 B - is one FULL 128-byte line
// (the 8-ROI kernel above writes A^T as 16-byte column runs and relies on eight blocks of one XCD meeting in L2 to
// complete a line: 0.39 of the HBM write roofline).  Work items are (ROI, bin) pairs, one 16-byte LDS read per window
// pixel feeds the packed int16 maxima of all 8 channels; 3136 items over 256 threads - no idle lanes, which is what
// made round 1's 64-ROI attempt slower.  The [64][8*49] tile (pitch 792 B: 8-byte aligned rows for the A runs, bank
// spread for the transposed reads) leaves LDS as 64 runs of 784 B of A and 392 full lines of A^T.  Block ids run
// chunk-fastest inside an XCD's contiguous range: the two partial lines at the ends of a 784-byte A run are shared with
// the neighbouring channel chunks, which the same XCD's L2 sees right next in time.
constexpr int ROI_G64 = 64;
constexpr int G64_CH = 8, G64_RUN = G64_CH * 49, G64_PITCH = G64_RUN * 2 + 8, G64_THREADS = 512;
template <int JMAX>  // (ROI, bin) items per thread: ceil(64 * 49 / threads) = 13 / 7 / 4 for 256 / 512 / 1024 threads
__global__ __launch_bounds__(JMAX >= 13 ? 256 : JMAX >= 7 ? 512 : 1024, JMAX >= 13 ? 2 : 4) void roi_pool7_map64_kernel(RoiParams p) {
  constexpr int PP = 49;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int HW = p.H * p.W;
  // the map slice is staged in BANDS of whole rows (p.lds_px pixels at most; one band = the whole map for everything up
  // to ~6700 pixels): larger maps - 75 x 122 for a 1200 x 1951 image - used to fall to the 8-ROI kernel that re-stages
  // the slice per 8 ROIs (1.4 ms per call there).  A (ROI, bin) item keeps its running maximum in registers across the bands.
  const int band_rows = p.lds_px >= HW ? p.H : p.lds_px / p.W;
  const long map_bytes = ((long)(band_rows < p.H ? band_rows * p.W : HW) * 16 + 15) & ~15L;
  // [band pixels][8 channels, order-mapped bf16]; p.pf: two such buffers, chunk cc scans buffer cc & 1
  char* tile = smem + (p.pf ? 2 : 1) * map_bytes;            // [64][G64_PITCH]
  __shared__ unsigned char hb[ROI_G64][7][2], wb[ROI_G64][7][2];
  __shared__ int bidx[ROI_G64];
  __shared__ float mulv[ROI_G64];
  const int nchunks = (p.C - p.c_begin) / G64_CH, nblk = nchunks / p.cpb;   // blocks per ROI group
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int group = logical / nblk, cb = logical - group * nblk;
  const int m0 = group * ROI_G64;
  const int nr = min(ROI_G64, p.M - m0);
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int i = tid; i < ROI_G64 * 7; i += nthr) {
    const int r = i / 7, k = i - r * 7;
    if (r < nr) {
      const float* roi = p.rois + 5 * (long)(m0 + r);
      int x1, y1, rw, rh, hs, he, ws, we;
      roi_box(roi, p.scale, x1, y1, rw, rh);
      roi_bin(k, (float)rh / 7.f, y1, p.H, hs, he);
      roi_bin(k, (float)rw / 7.f, x1, p.W, ws, we);
      hb[r][k][0] = (unsigned char)hs; hb[r][k][1] = (unsigned char)he;
      wb[r][k][0] = (unsigned char)ws; wb[r][k][1] = (unsigned char)we;
      if (k == 0) {
        bidx[r] = (int)roi[0];
        mulv[r] = p.obj ? p.obj[m0 + r] + 1.f : 1.f;
      }
    }
  }
  __syncthreads();
  // runs of ROIs on the same image, as a bit mask of run ends (bit r: ROI r is the last of its run).  The walk that
  // used to find each run's end - `while (bidx[r1] == b) ++r1`: 64 dependent LDS reads in every thread, per chunk -
  // was 40-50 us of the 141-us launch (knock-outs, profiles/r2_24_*)
  __shared__ unsigned long long runmask;
  if (tid < 64) {
    const bool last = tid + 1 >= nr || bidx[tid + 1] != bidx[tid];
    const unsigned long long m = __ballot(last && tid < nr);
    if (tid == 0) runmask = m;
  }
  __syncthreads();
  const unsigned long long runs = runmask;
  // Per-thread item table, computed ONCE per block: item j of this thread is (ROI, bin) number tid + j * nthr of the
  // group, whatever the chunk - its window, its tile / A offsets, its scale and its "empty bin" flag do not depend on
  // the channels.  (They used to be re-derived - two divisions, four byte loads, the 64-bit output address - in the scan,
  // again in the epilogue and again in the A store loop of every chunk: the launch is VALU-issue bound, ~1400
  // instructions per thread and chunk at 4 cycles each.)
  int win[JMAX];    // hs | he << 8 | ws << 16 | we << 24 (map coordinates)
  int meta[JMAX];   // r | bin << 8 | empty << 16 | valid << 17
#pragma unroll
  for (int j = 0; j < JMAX; ++j) {
    const int it = tid + j * nthr;
    const bool valid = it < nr * PP;
    const int r = valid ? it / PP : 0, bin = valid ? it - r * PP : 0;
    const int ph = bin / 7, pw = bin - ph * 7;
    const int hs = hb[r][ph][0], he = hb[r][ph][1], ws = wb[r][pw][0], we = wb[r][pw][1];
    win[j] = hs | he << 8 | ws << 16 | we << 24;
    meta[j] = r | bin << 8 | ((he <= hs || we <= ws) ? 1 << 16 : 0) | (valid ? 1 << 17 : 0);
  }
  // p.pf (whole map in one band, <= 2 pixels per thread): the slice of the NEXT chunk (first run's image) is fetched
  // into registers at the top of a chunk and moved into the other map buffer behind the scan: no chunk but the first
  // waits for a global load, and the wait sits in front of this chunk's stores in program order (vmcnt counts loads
  // and stores in order), so the stores drain under the next chunk's scan.
  i32x4_t pfr[2];
  const int b_first = bidx[0];
  auto fetch = [&](int c0_) {
    const char* src = p.feat + ((long)b_first * HW * p.C + c0_) * 2;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int px = tid + q * nthr;
      if (px < HW) pfr[q] = *(const i32x4_t*)(src + (long)px * p.C * 2);
    }
  };
  auto stash = [&](char* dst) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int px = tid + q * nthr;
      if (px < HW) {
        i32x4_t x = pfr[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = bf16x2_order(x[e]);
        *(i32x4_t*)(dst + (long)px * 16) = x;
      }
    }
  };
  if (p.pf) {
    fetch(p.c_begin + cb * p.cpb * G64_CH);
    stash(smem);
    __syncthreads();
  }
  typedef int i32x2_t __attribute__((ext_vector_type(2)));
  for (int cc = 0; cc < p.cpb; ++cc) {  // the block's channel chunks: same ROIs, same bin bounds
    const int c0 = p.c_begin + (cb * p.cpb + cc) * G64_CH;
    // the packed table stays packed: without this the compiler hoists every unpacked field (and every product with a
    // pitch) out of the chunk loop - ~60 more live registers, i.e. spills at the 128 that two blocks per CU allow
#pragma unroll
    for (int j = 0; j < JMAX; ++j) asm volatile("" : "+v"(win[j]), "+v"(meta[j]));
    char* map = p.pf ? smem + (cc & 1) * map_bytes : smem;
    if (p.pf && cc + 1 < p.cpb) fetch(c0 + G64_CH);
    for (int r0 = 0; r0 < nr;) {  // one pass per run of ROIs on the same image
      const int b = bidx[r0];
      const int r1 = r0 + __builtin_ctzll(runs >> r0) + 1;
      const char* fb = p.feat + ((long)b * HW * p.C + c0) * 2;
      const int lo = (int)0x80008000u;
      i32x4_t acc[JMAX];
#pragma unroll
      for (int j = 0; j < JMAX; ++j) acc[j] = i32x4_t{lo, lo, lo, lo};
      for (int y0 = 0; y0 < p.H; y0 += band_rows) {
        const int y1 = min(p.H, y0 + band_rows), npx = (y1 - y0) * p.W;
        const char* fbb = fb + (long)y0 * p.W * p.C * 2;
        if (!(p.pf && r0 == 0)) {  // (prefetch mode: the first run's slice is in LDS already, behind a barrier)
          // four pixels per thread and trip, all four loads issued before the first conversion: at real map sizes (50x76:
          // 3800 pixels of 16 bytes, 2 KB apart) the one-pixel loop waited out a full memory latency per pixel -
          // 47 of the launch's 256 us there (knock-outs, profiles/r3_23_roi_large_maps.txt)
          // (JMAX <= 4 = the 1024-thread variant these maps take; in the 512-thread variant of the 14x14 .. 38x38 maps the
          // extra live registers would spill at its 128-register cap, and its slice comes from the prefetch path anyway)
          if (JMAX > 4) {
            for (int px = tid; px < npx; px += nthr) {
              i32x4_t x = *(const i32x4_t*)(fbb + (long)px * p.C * 2);
#pragma unroll
              for (int e = 0; e < 4; ++e) x[e] = bf16x2_order(x[e]);
              *(i32x4_t*)(map + (long)px * 16) = x;
            }
          } else
          for (int px0 = tid; px0 < npx; px0 += 4 * nthr) {
            i32x4_t x[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int px = px0 + q * nthr;
              if (px < npx) x[q] = *(const i32x4_t*)(fbb + (long)px * p.C * 2);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int px = px0 + q * nthr;
              if (px < npx) {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[q][e] = bf16x2_order(x[q][e]);
                *(i32x4_t*)(map + (long)px * 16) = x[q];
              }
            }
          }
          __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
          const int r = meta[j] & 0xff;
          if ((meta[j] >> 17 & 1) && r >= r0 && r < r1) {
            const int hs = max(win[j] & 0xff, y0), he = min(win[j] >> 8 & 0xff, y1);
            const int ws = win[j] >> 16 & 0xff, we = win[j] >> 24 & 0xff;
            for (int h = hs; h < he; ++h) {
              const char* row = map + (long)((h - y0) * p.W) * 16;
              int w = ws;
              if (JMAX <= 4)
              for (; w + 1 < we; w += 2) {  // two pixels per trip, both reads in flight before the first max
                const i32x4_t x0 = *(const i32x4_t*)(row + w * 16), x1 = *(const i32x4_t*)(row + w * 16 + 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] = pk_max_i16(pk_max_i16(acc[j][e], x0[e]), x1[e]);
              }
              for (; w < we; ++w) {
                const i32x4_t x = *(const i32x4_t*)(row + w * 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] = pk_max_i16(acc[j][e], x[e]);
              }
            }
          }
        }
        if (!(p.pf && r1 == nr)) __syncthreads();  // the band may be replaced (prefetch mode, last run: this buffer rests for two chunks)
      }
#pragma unroll
      for (int j = 0; j < JMAX; ++j) {
        const int r = meta[j] & 0xff, bin = meta[j] >> 8 & 0xff;
        if ((meta[j] >> 17 & 1) && r >= r0 && r < r1) {
          const bool empty = meta[j] >> 16 & 1;
          const float mul = mulv[r];
          bf16_t* dst = (bf16_t*)(tile + r * G64_PITCH) + bin;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t y = (uint32_t)bf16x2_order(acc[j][e]);
            const float f0 = empty ? 0.f : __builtin_bit_cast(float, y << 16);
            const float f1 = empty ? 0.f : __builtin_bit_cast(float, y & 0xffff0000u);
            dst[(2 * e) * PP] = f32_to_bf16(f0 * mul);
            dst[(2 * e + 1) * PP] = f32_to_bf16(f1 * mul);
          }
        }
      }
      r0 = r1;
    }
    if (p.pf && cc + 1 < p.cpb) stash(smem + ((cc + 1) & 1) * map_bytes);  // (that buffer's readers: chunk cc - 1, two barriers ago)
    __syncthreads();  // the tile is complete (and the next chunk's slice visible)
    // A: nr runs of 784 bytes (49 x 16 B), rows of the tile are 8-byte aligned; piece j of this thread = its item j
    char* oa = p.out + ((long)m0 * p.ld_out + (long)c0 * PP) * 2;
    const int ld2 = (int)(p.ld_out * 2);  // (64 rows x ld_out x 2 B fits 31 bits: ld_out < 16 M elements)
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
      if (meta[j] >> 17 & 1) {
        const int r = meta[j] & 0xff, bin = meta[j] >> 8 & 0xff;
        const char* src = tile + r * G64_PITCH + bin * 16;
        const i32x2_t a = *(const i32x2_t*)src, b2 = *(const i32x2_t*)(src + 8);
        *(i32x4_t*)(oa + (r * ld2 + bin * 16)) = i32x4_t{a[0], a[1], b2[0], b2[1]};
      }
    }
    if (p.out_t && c0 + G64_CH > p.t_c0) {  // (round 3: the fc6 dW reads A itself; only the peeled tail columns keep an A^T)
      char* ot = p.out_t + ((long)c0 * PP * p.ld_out_t + m0) * 2;
      if (nr == ROI_G64) {
        // (k row, 8-ROI octet): 8 lanes write one full 128-byte line; piece i of this thread is row (tid >> 3) + i * nthr / 8
        const int q = tid & 7;
        const char* src = tile + (8 * q) * G64_PITCH + (tid >> 3) * 2;
        char* dst = ot + (long)(tid >> 3) * p.ld_out_t * 2 + q * 16;
        const long dstep = (long)(nthr >> 3) * p.ld_out_t * 2;
#pragma unroll
        for (int i = 0; i < JMAX; ++i) {
          if (tid + i * nthr < G64_RUN * 8) {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
              w[k] = (uint32_t)(*(const bf16_t*)(src + (2 * k) * G64_PITCH)) |
                     ((uint32_t)(*(const bf16_t*)(src + (2 * k + 1) * G64_PITCH)) << 16);
            *(i32x4_t*)dst = i32x4_t{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
          }
          src += (nthr >> 3) * 2;
          dst += dstep;
        }
      } else {
        for (int idx = tid; idx < G64_RUN; idx += nthr)
          for (int rr = 0; rr < nr; ++rr)
            ((bf16_t*)(ot + (long)idx * p.ld_out_t * 2))[rr] = *(const bf16_t*)(tile + (long)rr * G64_PITCH + idx * 2);
      }
    }
    if (cc + 1 < p.cpb) {
      // the tile is free for the next chunk: every wave's LDS reads have returned (their data went into the stores).  A raw
      // barrier - __syncthreads() would also wait (vmcnt) for the A / A^T stores just issued, which are meant to drain
      // under the next chunk's scan
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }  // channel chunks of this block
}

// 7x7 ROIPool, LANE-PER-BIN variant (round 4): the training operand A in bf16.
// What bounded the 64-ROI kernel above (88 us for the 201 MB of A at the bench shape = 0.29 of the HBM roofline, its
// traffic 1.03x algorithmic): ~240 VALU instructions per (ROI, bin, 8 channels) item - a per-pixel window loop whose
// trip counts differ lane by lane and that waits out the LDS latency at every pixel (ISA: ds_read_b128, s_waitcnt
// lgkmcnt(0), four v_pk_max_i16, six loop-control instructions), an epilogue that scatters every item's 8 channels into a
// [ROI][channel][bin] LDS tile as eight 2-byte writes, and a second pass that reads the tile back for the stores.
// Here a WAVE owns one ROI and lane l < 49 owns bin l:
//   * channel c's 49 bins sit in 49 consecutive lanes, and A[r][c * 49 + bin] is exactly that order: every channel
//     leaves as ONE 98-byte run per store instruction (global_store_short / _short_d16_hi on the packed pair) - no LDS
//     tile, no transposition, no second pass, no barrier per chunk;
//   * the bin windows are computed once per ROI and serve all NCK 8-channel chunks of the block's slice: per window
//     pixel one address and NCK independent 16-byte LDS reads (all in flight together) feed NCK x 4 v_pk_max_i16;
//   * window loops run to the wave's LARGEST window with clamped coordinates (a pixel read twice does not change a
//     maximum): uniform trip counts, no divergence, nothing waits per pixel.
// LDS: [NCK][H*W][16 B] (8 channels of a pixel, order-mapped bf16), staged once per run of same-image ROIs of the block.
// Bit-identical to the kernels above (same maxima, same fp32 scaling, same RNE conversion).  15 of 64 lanes idle.
// VD (round 5): dwords of one LDS cell - 4 = 8 channels of a pixel in 16 bytes (every map whose 8-channel slice fits the LDS),
// 2 = 4 channels in 8 bytes: maps of up to ~19 700 cells, i.e. the shipped dilated-C5 recipe's stride-8 feature map of a
// real-size image (99 x 151 at 800 x 1216: an 8-channel slice is 240 KB).  Those maps used to fall to the 64-ROI kernel in
// row bands: 1.95 ms per pooling launch at R = 2000, 46 % of a DC5 inference pass (profiles/r5_25_infer800_r50dc5_kernel_stats.txt).
template <int NCK, int NWV = 8, int VD = 4>
__global__ __launch_bounds__(NWV * 64) void roi_pool7_lane_kernel(RoiParams p) {
  typedef int cellv __attribute__((ext_vector_type(VD)));
  constexpr int CB = VD * 4, CH = VD * 2;  // bytes / channels of a cell
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int HW = p.H * p.W;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = NWV;
  // window pixels per trip of the scan: with one or two chunks per block (large maps: windows of 4-15 pixels a side) four
  // clamped pixels of a row go out together - four independent LDS reads in flight instead of one per trip
  constexpr int UNR = NCK <= 2 ? 4 : 1;
  const int nslice = p.C / (CH * NCK);
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int group = logical / nslice, sl = logical - group * nslice;
  const int c0 = sl * CH * NCK;
  const int ph = lane / 7, pw = lane - ph * 7;
  const bool is_bin = lane < 49;
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const unsigned cstride = (unsigned)HW * (unsigned)CB;
  int cur_img = -1;
  for (int rep = 0; rep < p.lane_reps; ++rep) {  // (the staged slice carries over from group to group while the image stays)
  const int m0 = (group * p.lane_reps + rep) * p.lane_g;
  if (m0 >= p.M) break;
  const int nr = min(p.lane_g, p.M - m0);
  // every wave keeps the group's ROIs in its lanes (lane l: ROI m0 + l; <= 64 per group): box corners on the map, image
  // index, scale - one round of loads per group instead of a dependent scalar load chain per ROI; a ROI's values reach all
  // lanes through v_readlane (the ROI index is wave-uniform)
  int vx1 = 0, vy1 = 0, vrw = 0, vrh = 0, vimg = -1;
  float vmul = 1.f;
  if (lane < nr) {
    const float* roi = p.rois + 5 * (long)(m0 + lane);
    vimg = (int)roi[0];
    roi_box(roi, p.scale, vx1, vy1, vrw, vrh);
    vmul = p.obj ? p.obj[m0 + lane] + 1.f : 1.f;
  }
  // runs of ROIs on the same image as a bit mask of run ends (one run in all but ragged batches)
  const int nxt = __shfl_down(vimg, 1, 64);
  const unsigned long long runs = __ballot(lane < nr && (lane + 1 >= nr || nxt != vimg));
  for (int r0 = 0; r0 < nr;) {
    const int b = __builtin_amdgcn_readlane(vimg, r0);
    const int r1 = r0 + __builtin_ctzll(runs >> r0) + 1;
    if (b != cur_img) {
      if (cur_img >= 0) __syncthreads();  // every wave is done with the previous image's slice
      // (built and measured: staging from a chunk-major copy of the map, [N][C / 8][H * W][8] - every slice one contiguous run
      // instead of 16 bytes of each 2-KB pixel - moved the launch by 2-5 % at 43x58 .. 63x92: the scan bounds it, not the
      // staging's sector over-fetch; the extra entry points were removed again)
      const char* fb = p.feat + ((long)b * HW * p.C + c0) * 2;
      for (int idx = tid; idx < HW * NCK; idx += NW * 64) {
        const int px = idx / NCK, c = idx - px * NCK;
        cellv x = *(const cellv*)(fb + (long)px * p.C * 2 + c * CB);
#pragma unroll
        for (int e = 0; e < VD; ++e) x[e] = bf16x2_order(x[e]);
        *(cellv*)(smem + ((long)c * HW + px) * CB) = x;
      }
      __syncthreads();
      cur_img = b;
    }
    for (int r = r0 + wave; r < r1; r += NW) {
      const int x1 = __builtin_amdgcn_readlane(vx1, r), y1 = __builtin_amdgcn_readlane(vy1, r);
      const int rw = __builtin_amdgcn_readlane(vrw, r), rh = __builtin_amdgcn_readlane(vrh, r);
      const float mul = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vmul), r));
      int hs, he, ws, we;
      roi_bin(ph, (float)rh / 7.f, y1, p.H, hs, he);
      roi_bin(pw, (float)rw / 7.f, x1, p.W, ws, we);
      const bool empty = he <= hs || we <= ws;
      const int nh = (is_bin && !empty) ? he - hs : 0, nw = (is_bin && !empty) ? we - ws : 0;
      int max_nh = 0, max_nw = 0;  // the wave's largest window (uniform)
      while (__ballot(max_nh < nh) != 0) ++max_nh;
      while (__ballot(max_nw < nw) != 0) ++max_nw;
      const int lo = (int)0x80008000u;
      cellv acc[NCK];
#pragma unroll
      for (int c = 0; c < NCK; ++c)
#pragma unroll
        for (int e = 0; e < VD; ++e) acc[c][e] = lo;
      // (built and measured: the same loops with every read PREDICATED on the lane's own window instead of clamped - a third
      // of the LDS bytes - are slower at every map size, 61 -> 67 us at 14x14 and 350 -> 404 us at 63x92: the exec-mask
      // bookkeeping and the re-initialised operands cost more issue slots than the reads cost LDS cycles)
      // UNRH window rows per trip (4-channel cells - the largest maps, windows of 5-20 pixels a side: two rows x four clamped
      // pixels = eight independent LDS reads in flight instead of four; the scan of those maps is bound by the reads' latency,
      // not by LDS bandwidth: 1432 us against ~270 us of LDS cycles at 99x151, profiles/r5_26_*)
      constexpr int UNRH = VD == 2 ? 2 : 1;
      const int wlast = min(max(we - 1, 0), p.W - 1), wfirst = min(max(ws, 0), p.W - 1);
      for (int hi = 0; hi < max_nh; hi += UNRH) {
        unsigned arow[UNRH];
#pragma unroll
        for (int v = 0; v < UNRH; ++v) {
          const int hr = min(max(min(hs + hi + v, he - 1), 0), p.H - 1);
          arow[v] = lds0 + (unsigned)(hr * p.W) * (unsigned)CB;
        }
        for (int wi = 0; wi < max_nw; wi += UNR) {
          cellv x[UNRH][UNR][NCK];
#pragma unroll
          for (int u = 0; u < UNR; ++u) {
            const int wc = min(wfirst + wi + u, wlast);  // clamped: a pixel read twice does not change a maximum
#pragma unroll
            for (int v = 0; v < UNRH; ++v) {
              const unsigned a = arow[v] + (unsigned)wc * (unsigned)CB;
#pragma unroll
              for (int c = 0; c < NCK; ++c)
                x[v][u][c] = *(__attribute__((address_space(3))) const cellv*)(uintptr_t)(a + (unsigned)c * cstride);
            }
          }
#pragma unroll
          for (int v = 0; v < UNRH; ++v)
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
              for (int c = 0; c < NCK; ++c)
#pragma unroll
                for (int e = 0; e < VD; ++e) acc[c][e] = pk_max_i16(acc[c][e], x[v][u][c][e]);
        }
      }
      if (is_bin) {
        bf16_t* dst = (bf16_t*)p.out + (long)(m0 + r) * p.ld_out + (long)c0 * 49 + lane;

#pragma unroll
        for (int c = 0; c < NCK; ++c)
#pragma unroll
          for (int e = 0; e < VD; ++e) {
            // (an empty bin is +0 in both halves; one packed conversion - v_cvt_pk_bf16_f32, RNE like f32_to_bf16 - and the
            // two halves of its result leave through global_store_short / global_store_short_d16_hi)
            const uint32_t y = empty ? 0u : (uint32_t)bf16x2_order(acc[c][e]);
            typedef float f32x2_t __attribute__((ext_vector_type(2)));
            typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
            const f32x2_t f = f32x2_t{__builtin_bit_cast(float, y << 16), __builtin_bit_cast(float, y & 0xffff0000u)} * mul;
            const uint32_t o = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2_t));
            dst[(c * CH + 2 * e) * 49] = (bf16_t)(o & 0xffffu);
            dst[(c * CH + 2 * e + 1) * 49] = (bf16_t)(o >> 16);
          }
      }
    }
    r0 = r1;
  }
  }  // groups of this block
}

// 7x7 ROIAlign, LANE-PER-BIN (round 6): bf16 in / bf16 out, the forward of detectron2/layers/roi_align.py:22-59 ->
// ROIAlign_forward (detectron2/layers/csrc/ROIAlign/ROIAlign_cuda.cu:65-139; pre_calc + accumulate of ROIAlign_cpu.cpp), fused with
// the objectness scaling like the RoIPool kernels.  The generic kernel (roi_kernel MODE 1: block = ROI x 64 channels, lane =
// channel) computes every sample's four bilinear weights - ~40 VALU instructions of float clamping - once per LANE, i.e. 64
// times per 64 channels, and fetches its four taps from global memory per sample: 455-500 us for 2000 ROIs on the 14x14x1024
// map, 0.05 of the HBM roof (profiles/r6_11_roi_align.txt).  Here, as in roi_pool7_lane_kernel: a block stages NCK 8-channel
// slices of the whole map in LDS once per group of ROIs, a WAVE owns one ROI and lane l < 49 owns bin l; the sampling grid
// (gh x gw, adaptive or fixed) is uniform over the ROI, a sample's weights and its four cell addresses are computed ONCE per
// bin and serve all NCK x 8 channels of the block's slices (4 x NCK 16-byte LDS reads, 7 fp32 operations per channel), and a
// channel's 49 bins leave as one 98-byte run per store instruction.
// Same operations on the same values in the same order as roi_kernel<.., 1> (w = hy * hx ..; ((w1 v1 + w2 v2) + w3 v3) + w4 v4;
// samples outside [-1, H] x [-1, W] skipped; acc / count * (objectness + 1); one RNE conversion): bit-identical outputs.
template <int NCK>
__global__ __launch_bounds__(512) void roi_align7_lane_kernel(RoiParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int HW = p.H * p.W;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = 8;
  const int nslice = p.C / (8 * NCK);
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int group = logical / nslice, sl = logical - group * nslice;
  const int c0 = sl * 8 * NCK;
  const int ph = lane / 7, pw = lane - ph * 7;
  const bool is_bin = lane < 49;
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const unsigned cstride = (unsigned)HW * 16u;
  const int m0 = group * p.lane_g;
  if (m0 >= p.M) return;
  const int nr = min(p.lane_g, p.M - m0);
  // the group's ROIs in the lanes of every wave (lane l: ROI m0 + l)
  float fx1 = 0.f, fy1 = 0.f, fx2 = 0.f, fy2 = 0.f, vmul = 1.f;
  int vimg = -1;
  if (lane < nr) {
    const float* roi = p.rois + 5 * (long)(m0 + lane);
    vimg = (int)roi[0];
    fx1 = roi[1]; fy1 = roi[2]; fx2 = roi[3]; fy2 = roi[4];
    vmul = p.obj ? p.obj[m0 + lane] + 1.f : 1.f;
  }
  const int nxt = __shfl_down(vimg, 1, 64);
  const unsigned long long runs = __ballot(lane < nr && (lane + 1 >= nr || nxt != vimg));
  auto bcast = [&](float v, int r) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), r)); };
  int cur_img = -1;
  for (int r0 = 0; r0 < nr;) {
    const int b = __builtin_amdgcn_readlane(vimg, r0);
    const int r1 = r0 + __builtin_ctzll(runs >> r0) + 1;
    if (b != cur_img) {
      if (cur_img >= 0) __syncthreads();
      const char* fb = p.feat + ((long)b * HW * p.C + c0) * 2;
      for (int idx = tid; idx < HW * NCK; idx += NW * 64) {
        const int px = idx / NCK, c = idx - px * NCK;
        *(i32x4_t*)(smem + ((long)c * HW + px) * 16) = *(const i32x4_t*)(fb + (long)px * p.C * 2 + c * 16);
      }
      __syncthreads();
      cur_img = b;
    }
    for (int r = r0 + wave; r < r1; r += NW) {
      const float off = p.aligned ? 0.5f : 0.f;
      const float sw = bcast(fx1, r) * p.scale - off, sh = bcast(fy1, r) * p.scale - off;
      const float ew = bcast(fx2, r) * p.scale - off, eh = bcast(fy2, r) * p.scale - off;
      const float mul = bcast(vmul, r);
      float rw = ew - sw, rh = eh - sh;
      if (!p.aligned) { rw = fmaxf(rw, 1.f); rh = fmaxf(rh, 1.f); }
      const float bin_h = rh / 7.f, bin_w = rw / 7.f;
      const int gh = p.sampling_ratio > 0 ? p.sampling_ratio : (int)ceilf(rh / 7);
      const int gw = p.sampling_ratio > 0 ? p.sampling_ratio : (int)ceilf(rw / 7);
      const float count = (float)max(gh * gw, 1);
      float acc[NCK][8];
#pragma unroll
      for (int c = 0; c < NCK; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[c][e] = 0.f;
      for (int iy = 0; iy < gh; ++iy) {
        const float yy = sh + ph * bin_h + (float)(iy + .5f) * bin_h / (float)gh;
        for (int ix = 0; ix < gw; ++ix) {
          const float xx = sw + pw * bin_w + (float)(ix + .5f) * bin_w / (float)gw;
          float x = xx, y = yy;
          if (!is_bin || y < -1.0f || y > p.H || x < -1.0f || x > p.W) continue;
          if (y <= 0) y = 0;
          if (x <= 0) x = 0;
          int yl = (int)y, xl = (int)x, yh, xh;
          if (yl >= p.H - 1) { yh = yl = p.H - 1; y = (float)yl; } else yh = yl + 1;
          if (xl >= p.W - 1) { xh = xl = p.W - 1; x = (float)xl; } else xh = xl + 1;
          const float ly = y - yl, lx = x - xl, hy = 1.f - ly, hx = 1.f - lx;
          const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
          const unsigned a1 = lds0 + (unsigned)(yl * p.W + xl) * 16u, a2 = lds0 + (unsigned)(yl * p.W + xh) * 16u;
          const unsigned a3 = lds0 + (unsigned)(yh * p.W + xl) * 16u, a4 = lds0 + (unsigned)(yh * p.W + xh) * 16u;
          typedef __attribute__((address_space(3))) const i32x4_t* lds_v4;
#pragma unroll
          for (int c = 0; c < NCK; ++c) {
            const i32x4_t q1 = *(lds_v4)(uintptr_t)(a1 + (unsigned)c * cstride), q2 = *(lds_v4)(uintptr_t)(a2 + (unsigned)c * cstride);
            const i32x4_t q3 = *(lds_v4)(uintptr_t)(a3 + (unsigned)c * cstride), q4 = *(lds_v4)(uintptr_t)(a4 + (unsigned)c * cstride);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              auto f = [&](const i32x4_t& q) {
                const uint32_t wd = (uint32_t)q[e >> 1];
                return __builtin_bit_cast(float, (e & 1) ? (wd & 0xffff0000u) : (wd << 16));
              };
              acc[c][e] += w1 * f(q1) + w2 * f(q2) + w3 * f(q3) + w4 * f(q4);
            }
          }
        }
      }
      if (is_bin) {
        bf16_t* dst = (bf16_t*)p.out + (long)(m0 + r) * p.ld_out + (long)c0 * 49 + lane;
#pragma unroll
        for (int c = 0; c < NCK; ++c)
#pragma unroll
          for (int e = 0; e < 8; ++e) dst[(c * 8 + e) * 49] = f32_to_bf16(acc[c][e] / count * mul);
      }
    }
    r0 = r1;
  }
}

// Chunk-major copy of a bf16 NHWC map for the walking kernel below: [N][H*W][C] -> [N][C/8][H*W] cells of 16 bytes (8 channels of a
// pixel), values already order-mapped (bf16x2_order).  A staged slice is then ONE contiguous run instead of 16 bytes of every
// pixel's 2-KB line (64 lines per wave instruction: ~28 us of a 156-us pooling launch at 50x76 - profiles/r5_32_roi_walk_knockouts.txt).
// 32 pixels x 32 chunks per block through LDS: 512-byte runs on both sides.
__global__ __launch_bounds__(256) void roi_chunk_major_kernel(const char* __restrict__ feat, char* __restrict__ cm, int HW, int C) {
  __shared__ i32x4_t tile[32][33];
  const int nchunks = C >> 3;
  const int px0 = blockIdx.x * 32, ch0 = blockIdx.y * 32, img = blockIdx.z;
  const char* src = feat + (long)img * HW * C * 2;
  char* dst = cm + (long)img * nchunks * HW * 16;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = threadIdx.x + 256 * i, pl = idx >> 5, cl = idx & 31;
    i32x4_t x = {0, 0, 0, 0};
    if (px0 + pl < HW && ch0 + cl < nchunks) x = *(const i32x4_t*)(src + ((long)(px0 + pl) * C + (ch0 + cl) * 8) * 2);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = bf16x2_order(x[e]);
    tile[pl][cl] = x;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = threadIdx.x + 256 * i, cl = idx >> 5, pl = idx & 31;
    if (px0 + pl < HW && ch0 + cl < nchunks) *(i32x4_t*)(dst + ((long)(ch0 + cl) * HW + px0 + pl) * 16) = tile[pl][cl];
  }
}

// 7x7 ROIPool, lane-per-bin, WALKING variant (round 5) for maps whose 8-channel slice leaves at most two blocks per CU
// (43x58 and larger: test-time scales, real-size training images).  Knock-outs of the kernel above at 50x76 / R = 2000
// (profiles/r5_32_roi_walk_knockouts.txt): 71 us of its 215 are the staging (one 16-byte piece of every pixel's 2-KB line per
// load - and one load, one wait, one LDS write per trip), ~90 us the scan, ~27 us the stores; the scan is instruction-issue
// bound (conflict-free or broadcast LDS addresses: -10 %; six more VALU instructions per read: +18 %), and with ROIs sorted by
// size the launch takes 1.6x as long - whatever unit waits for its largest ROIs sets the time.  Here
//   * a block keeps its group of ROIs and walks `p.walk` CONSECUTIVE channel chunks, re-staging the slice between them: the
//     walked chunks are the 16-byte pieces of ONE 128-byte line per pixel (walk = 8), so the first chunk's staging brings the
//     lines into the XCD's L2 and the other seven hit there; eight loads are in flight per thread;
//   * the bin bounds are computed once per block into an LDS table: per ROI 7 row entries (first row's LDS offset, rows - 1)
//     and 7 column entries (first column's offset, columns - 1) - a lane fetches the two entries of its bin, 72 bytes per ROI
//     instead of ~100 VALU instructions per (ROI, chunk);
//   * the waves of a block take ROIs from a shared counter (one LDS atomic per ROI and chunk, fetched one ROI ahead) instead
//     of a fixed share: the barrier at the end of a chunk waits for one ROI, not for the wave with the largest eight;
//   * the slice's rows have an ODD pitch in cells: W is even for every map here, so rows alone moved a lane by even cell
//     counts (4-byte banks: 16-byte cells map to 16 bank groups).
// Same maxima over the same pixels, same scaling / conversion as the kernels above: bit-identical outputs.
// NSG: sub-groups of 64 ROIs per block (image indices of a sub-group sit in the lanes of every wave).
constexpr int WALK_TAB = 18;  // table dwords per ROI: [0..7] rows by ph, [8..15] columns by pw, [16] largest window, [17] scale
template <int NWV, int NSG, int VD, int SB, int OCC = 1>  // SB: slice cells per thread (>= ceil(H * W / threads)); OCC: blocks per CU the registers must allow
__global__ __launch_bounds__(NWV * 64, OCC) void roi_pool7_walk_kernel(RoiParams p) {
  typedef int cellv __attribute__((ext_vector_type(VD)));
  constexpr int CB = VD * 4, CH = VD * 2, NT = NWV * 64, G = 64 * NSG;
  // (two window rows per trip - eight reads in flight - measured slower for 8-channel cells: 187 vs 174 us at 50x76, the rows are
  // rounded up to pairs)
  constexpr int UNR = 4, UNRH = VD == 2 ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int HW = p.H * p.W;
  const int tid = threadIdx.x, lane = tid & 63;
  const int Wp = p.walk_wp;  // LDS row pitch in cells
  const int ncg = p.C / (CH * p.walk);  // chunk groups
  const int ngroups = gridDim.x / ncg;
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  // chunk-group major: the blocks of one XCD share few slices
  const int cg = logical / ngroups, group = logical - cg * ngroups;
  const int ph = lane / 7, pw = lane - ph * 7;  // (lanes 49..63: ph = 7 / 8 / 9 -> the table's entry 7, an empty row)
  const bool is_bin = lane < 49;
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const unsigned WCB = (unsigned)Wp * CB;
  unsigned* tab = (unsigned*)(smem + (size_t)p.H * Wp * CB);
  unsigned* ctr = tab + G * WALK_TAB;
  const int m0 = group * G;
  // ---- once per block: the window table ---------------------------------------------------------------------------------
  for (int t = tid; t < G * 8; t += NT) {
    const int rl = t >> 3, e = t & 7;
    const int m = m0 + rl;
    unsigned rowe = 0x80000000u, cole = 0x80000000u;
    int nh = 0, nw = 0;
    float mul = 1.f;
    if (m < p.M && e < 7) {
      const float* roi = p.rois + 5 * (long)m;
      int x1, y1, rw, rh, hs, he, ws, we;
      roi_box(roi, p.scale, x1, y1, rw, rh);
      mul = p.obj ? p.obj[m] + 1.f : 1.f;
      roi_bin(e, (float)rh / 7.f, y1, p.H, hs, he);
      roi_bin(e, (float)rw / 7.f, x1, p.W, ws, we);
      nh = max(he - hs, 0);
      nw = max(we - ws, 0);
      // (an empty row / column of bins reads some valid pixel and drops it)
      rowe = (unsigned)min(hs, p.H - 1) * WCB | (unsigned)max(nh - 1, 0) << 20 | (nh == 0 ? 0x80000000u : 0u);
      cole = (unsigned)min(ws, p.W - 1) * CB | (unsigned)max(nw - 1, 0) << 20 | (nw == 0 ? 0x80000000u : 0u);
    }
    // the ROI's largest window: over its 8 entries = 8 consecutive lanes
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
      nh = max(nh, __shfl_xor(nh, d, 64));
      nw = max(nw, __shfl_xor(nw, d, 64));
    }
    tab[rl * WALK_TAB + e] = rowe;
    tab[rl * WALK_TAB + 8 + e] = cole;
    if (e == 0) {
      tab[rl * WALK_TAB + 16] = (unsigned)nh | (unsigned)nw << 16;
      tab[rl * WALK_TAB + 17] = __builtin_bit_cast(unsigned, mul);
    }
  }
  // image runs of every sub-group, as a bit mask of run ends (one run in all but ragged batches)
  int vimg[NSG], nrs[NSG];
  unsigned long long runs[NSG];
#pragma unroll
  for (int sg = 0; sg < NSG; ++sg) {
    const int ms = m0 + sg * 64;
    const int nr = max(min(64, p.M - ms), 0);
    nrs[sg] = nr;
    vimg[sg] = lane < nr ? (int)p.rois[5 * (long)(ms + lane)] : -1;
    const int nxt = __shfl_down(vimg[sg], 1, 64);
    runs[sg] = __ballot(lane < nr && (lane + 1 >= nr || nxt != vimg[sg]));
  }
  // ---- the walk -----------------------------------------------------------------------------------------------------------
  // one image in the whole group (every batch but ragged ones): the NEXT chunk's slice is fetched into registers under this
  // chunk's scan - two blocks of a CU start together and run the same phases, so without it both stage (the memory pipe busy,
  // VALU idle) and both scan (the reverse) at the same time
  bool single = true;
#pragma unroll
  for (int sg = 0; sg < NSG; ++sg)
    single = single && __ballot(lane < nrs[sg] && vimg[sg] != __builtin_amdgcn_readlane(vimg[0], 0)) == 0;
  cellv pf[SB];
  // source of a slice: the chunk-major, order-mapped copy when the caller gave a workspace (one contiguous run), else the NHWC
  // map itself (16 bytes of every pixel's line)
  const bool from_cm = p.cm != nullptr;
  const long src_pitch = from_cm ? CB : (long)p.C * 2;
  auto load_slice = [&](int b, int chunk) {
    const char* fb = from_cm ? p.cm + ((long)b * (p.C / CH) + chunk) * HW * CB : p.feat + ((long)b * HW * p.C + (long)chunk * CH) * 2;
    // (no branch around a load or a write, not even a uniform one: the wait-count pass then puts s_waitcnt vmcnt(0) in front of
    // every load; a thread past the end re-reads / re-writes the last cell)
#pragma unroll
    for (int k = 0; k < SB; ++k) pf[k] = *(const cellv*)(fb + (long)min(tid + k * NT, HW - 1) * src_pitch);
  };
  auto write_slice = [&]() {
#pragma unroll
    for (int k = 0; k < SB; ++k) {
      cellv x = pf[k];
#pragma unroll
      for (int e = 0; e < VD; ++e) x[e] = from_cm ? x[e] : bf16x2_order(x[e]);
      const unsigned px = (unsigned)min(tid + k * NT, HW - 1), py = __umulhi(px, p.walk_wmagic);  // px / W
      *(cellv*)(smem + (size_t)(py * Wp + (px - py * p.W)) * CB) = x;
    }
  };
  if (single && nrs[0] > 0) load_slice(__builtin_amdgcn_readlane(vimg[0], 0), cg * p.walk);
  bool staged = false;
  for (int cc = 0; cc < p.walk; ++cc) {
    const int chunk = cg * p.walk + cc;
    int cur_img = -1;
#pragma unroll
    for (int sg = 0; sg < NSG; ++sg) {
      const int nr = nrs[sg];
      for (int r0 = 0; r0 < nr;) {
        const int b = __builtin_amdgcn_readlane(vimg[sg], r0);
        const int r1 = r0 + __builtin_ctzll(runs[sg] >> r0) + 1;
        // every wave is done with the previous run (slice and counter): its LDS reads have returned (their data went into the
        // stores).  Raw barriers - __syncthreads() would also drain the A stores just issued (vmcnt)
        if (staged) {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
        }
        if (tid == 0) *ctr = (unsigned)r0;
        bool fresh = false;
        if (b != cur_img) {
          if (!single) load_slice(b, chunk);
          write_slice();
          cur_img = b;
          fresh = true;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        staged = true;
        if (single && fresh && cc + 1 < p.walk) load_slice(b, chunk + 1);
        // ROIs r0 .. r1-1 of this sub-group, taken from the counter one ahead of the one being scanned
        unsigned nxt = 0;
        if (lane == 0) nxt = atomicAdd(ctr, 1u);
        for (;;) {
          const int r = __builtin_amdgcn_readfirstlane(nxt);
          if (r >= r1) break;
          if (lane == 0) nxt = atomicAdd(ctr, 1u);
          const unsigned* te = tab + (sg * 64 + r) * WALK_TAB;
          const unsigned rowe = te[ph > 7 ? 7 : ph], cole = te[8 + pw];
          const unsigned uni = __builtin_amdgcn_readfirstlane(te[16]);
          const float mul = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(te[17]));
          const int max_nh = uni & 0xffff, max_nw = uni >> 16;
          const unsigned nhm1 = rowe >> 20 & 0x7ff, nwm1 = cole >> 20 & 0x7ff;
          const unsigned org = lds0 + (rowe & 0xfffff) + (cole & 0xfffff);
          const bool empty = (int)(rowe | cole) < 0;
          const int lo = (int)0x80008000u;
          cellv acc;
#pragma unroll
          for (int e = 0; e < VD; ++e) acc[e] = lo;
          for (int hi = 0; hi < max_nh; hi += UNRH) {
            unsigned arow[UNRH];
#pragma unroll
            for (int v = 0; v < UNRH; ++v) arow[v] = org + min((unsigned)(hi + v), nhm1) * WCB;
            for (int wi = 0; wi < max_nw; wi += UNR) {
              cellv x[UNRH][UNR];
#pragma unroll
              for (int u = 0; u < UNR; ++u) {
                const unsigned co = min((unsigned)(wi + u), nwm1) * CB;
#pragma unroll
                for (int v = 0; v < UNRH; ++v)
                  x[v][u] = *(__attribute__((address_space(3))) const cellv*)(uintptr_t)(arow[v] + co);
              }
#pragma unroll
              for (int v = 0; v < UNRH; ++v)
#pragma unroll
                for (int u = 0; u < UNR; ++u)
#pragma unroll
                  for (int e = 0; e < VD; ++e) acc[e] = pk_max_i16(acc[e], x[v][u][e]);
            }
          }
          // (built and measured: the item's 8 x 49 values - one 784-byte run of A - through a per-wave LDS scratch as ONE 16-byte store
          // per lane instead of eight 2-byte stores: 176.0 vs 173.8 us at 50x76, 137 vs 125 at 43x58 (the scratch costs the third
          // block per CU) - eight ds_write_b16 + a ds_read_b128 take the issue slots the eight stores took)
          if (is_bin) {
            bf16_t* dst = (bf16_t*)p.out + (long)(m0 + sg * 64 + r) * p.ld_out + (long)chunk * CH * 49 + lane;
#pragma unroll
            for (int e = 0; e < VD; ++e) {
              // (an empty bin is +0 in both halves; one packed conversion - v_cvt_pk_bf16_f32, RNE like f32_to_bf16)
              const uint32_t y = empty ? 0u : (uint32_t)bf16x2_order(acc[e]);
              typedef float f32x2_t __attribute__((ext_vector_type(2)));
              typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
              const f32x2_t f = f32x2_t{__builtin_bit_cast(float, y << 16), __builtin_bit_cast(float, y & 0xffff0000u)} * mul;
              const uint32_t o = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2_t));
              dst[(2 * e) * 49] = (bf16_t)(o & 0xffffu);
              dst[(2 * e + 1) * 49] = (bf16_t)(o >> 16);
            }
          }
        }
        r0 = r1;
      }
    }
  }
}

// 7x7 ROIPool from a SPARSE TABLE of block maxima (round 6) - the maps whose slice leaves room for 4 channels per cell only (the
// shipped dilated-C5 recipe's stride-8 map of a real-size image: 99 x 151 x 2048, ~3750 cells per ROI).  The window kernels above
// read every cell of every ROI: 15.4 G bf16 elements through LDS and a packed maximum per two of them, 920 us for 2000 ROIs
// (roi_pool7_lane_kernel<1, 16, 2>, profiles/r6_11_roi_align.txt) - a compute bound that no schedule removes.  A maximum is
// idempotent, so the windows can share work instead: with T[k][l][y][x] = max over rows y .. y + 2^k - 1 and columns x .. x + 2^l - 1,
// a bin [hs, he) x [ws, we) whose sides are within [2^k, 2^(k+1)] x [2^l, 2^(l+1)] is the maximum of FOUR table cells
// (rows hs and he - 2^k, columns ws and we - 2^l: the blocks overlap, which a maximum does not mind) instead of ~77.  A ROI's 49
// bins differ by at most one row / column, so ONE level pair (k, l) = floor(log2) of its smallest non-empty bin serves all of
// them (2^k <= nh <= 2^k + 1 <= 2^(k+1)); ROIs clipped by the map edge or beyond level 4 (bins of 32+ cells) take
// ceil(nh / 2^k) x ceil(nw / 2^l) cells in a loop.  Work per block = (4-channel slice, image, l):
//   * the ROIs of its class are listed (by k) in LDS from the one-byte class codes roi_st_prep_kernel left; no ROI: exit;
//   * the slice - one contiguous run of the chunk-major, order-mapped copy of the map - lands in LDS and l doubling steps
//     along the rows make T[0][l] in place (a thread keeps its cells in registers: per step one LDS read of the partner
//     cell, one barrier, one write, one barrier);
//   * for k = 0 .. 4: doubling steps down the columns up to level k, then the waves pool the listed ROIs of level k: wave = ROI,
//     lane = bin as in roi_pool7_lane_kernel (every channel leaves as one 98-byte run), the bin's four cell coordinates come
//     packed in ONE dword per lane from the record the prep kernel wrote (fetched eight ROIs at a time).
// 30 doubling steps per slice serve ALL ROIs (~2.5 LDS passes over the slice each) against ~77 reads per (ROI, bin) before.
// Same maxima over the same cells, same scaling and conversion: bit-identical to the other RoIPool kernels.
constexpr int ST_LEVELS = 5;  // levels 0 .. 4: blocks of 1 .. 16 rows / columns
constexpr int ST_BATCH = 8;   // ROI records a wave fetches per round

// One wave per ROI: the record [64 dwords] - lanes 0 .. 48: y0 | y1 << 8 | x0 << 16 | x1 << 24 (first / last block row, first / last
// block column of the bin at the ROI's level; an empty bin: y0 = 1 > y1 = 0), lane 60: most blocks per bin (rows | columns << 8),
// lane 62: the objectness scale, lane 63: k | l << 4 - and the class byte (image * 5 + l) * 5 + k (255: image index out of range).
__global__ __launch_bounds__(256) void roi_st_prep_kernel(RoiParams p, unsigned* __restrict__ rec, unsigned char* __restrict__ cls) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= p.M) return;
  const float* roi = p.rois + 5 * (long)m;
  const int b = (int)roi[0];
  int x1, y1, rw, rh, hs, he, ws, we;
  roi_box(roi, p.scale, x1, y1, rw, rh);
  const float mul = p.obj ? p.obj[m] + 1.f : 1.f;
  const int ph = lane / 7, pw = lane - ph * 7;
  const bool is_bin = lane < 49;
  roi_bin(ph, (float)rh / 7.f, y1, p.H, hs, he);
  roi_bin(pw, (float)rw / 7.f, x1, p.W, ws, we);
  const int nh = he - hs, nw = we - ws;
  const bool empty = !is_bin || nh <= 0 || nw <= 0;
  int hmin = is_bin && nh > 0 ? nh : 0x7fff, wmin = is_bin && nw > 0 ? nw : 0x7fff;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hmin = min(hmin, __shfl_xor(hmin, o, 64));
    wmin = min(wmin, __shfl_xor(wmin, o, 64));
  }
  if (hmin == 0x7fff) hmin = 1;
  if (wmin == 0x7fff) wmin = 1;
  const int k = min(31 - __builtin_clz(hmin), ST_LEVELS - 1), l = min(31 - __builtin_clz(wmin), ST_LEVELS - 1);
  int nr = empty ? 0 : (nh + (1 << k) - 1) >> k, nc = empty ? 0 : (nw + (1 << l) - 1) >> l;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nr = max(nr, __shfl_xor(nr, o, 64));
    nc = max(nc, __shfl_xor(nc, o, 64));
  }
  unsigned r = 1u;  // empty: y0 = 1, y1 = 0, x0 = x1 = 0
  if (!empty) r = (unsigned)hs | (unsigned)(he - (1 << k)) << 8 | (unsigned)ws << 16 | (unsigned)(we - (1 << l)) << 24;
  if (lane == 60) r = (unsigned)nr | (unsigned)nc << 8;
  if (lane == 61) r = (unsigned)b;
  if (lane == 62) r = __builtin_bit_cast(unsigned, mul);
  if (lane == 63) r = (unsigned)k | (unsigned)l << 4;
  rec[(long)m * 64 + lane] = r;
  if (lane == 0) cls[m] = (b >= 0 && b < p.N) ? (unsigned char)((b * ST_LEVELS + l) * ST_LEVELS + k) : (unsigned char)255;
}

// chunk-major copy with cells of VD dwords (roi_chunk_major_kernel is the VD = 4 form; kept separate: its 16-byte tile is the
// walking kernel's measured path)
template <int VD>
__global__ __launch_bounds__(256) void roi_chunk_major_vd_kernel(const char* __restrict__ feat, char* __restrict__ cm, int HW, int C) {
  typedef int cellv __attribute__((ext_vector_type(VD)));
  constexpr int CB = VD * 4, CH = VD * 2;
  __shared__ cellv tile[32][33];
  const int nchunks = C / CH;
  const int px0 = blockIdx.x * 32, ch0 = blockIdx.y * 32, img = blockIdx.z;
  const char* src = feat + (long)img * HW * C * 2;
  char* dst = cm + (long)img * nchunks * HW * CB;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = threadIdx.x + 256 * i, pl = idx >> 5, cl = idx & 31;
    cellv x;
#pragma unroll
    for (int e = 0; e < VD; ++e) x[e] = 0;
    if (px0 + pl < HW && ch0 + cl < nchunks) x = *(const cellv*)(src + ((long)(px0 + pl) * C + (ch0 + cl) * CH) * 2);
#pragma unroll
    for (int e = 0; e < VD; ++e) x[e] = bf16x2_order(x[e]);
    tile[pl][cl] = x;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = threadIdx.x + 256 * i, cl = idx >> 5, pl = idx & 31;
    if (px0 + pl < HW && ch0 + cl < nchunks) *(cellv*)(dst + ((long)(ch0 + cl) * HW + px0 + pl) * CB) = tile[pl][cl];
  }
}

__device__ unsigned long long g_st_prof[8];  // PROF builds (tools/roi_st_probe.py): shader-clock cycles of block phases as thread 0 sees them
template <int VD, int SB, bool PROF = false>  // SB: slice cells per thread (>= ceil(H * W / 1024))
__global__ __launch_bounds__(1024) void roi_pool7_st_kernel(RoiParams p, const unsigned* __restrict__ rec, const unsigned char* __restrict__ cls) {
  typedef int cellv __attribute__((ext_vector_type(VD)));
  typedef __attribute__((address_space(3))) const cellv* lds_cell_t;
  constexpr int CB = VD * 4, CH = VD * 2, NT = 1024, NW = 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int HW = p.H * p.W, W = p.W;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned short* list = (unsigned short*)(smem + (size_t)HW * CB);
  int* cnt = (int*)(list + ((p.M + 7) & ~7));  // [0..4] ROIs per level, [8..12] fill cursors
  constexpr int SCR = (CH * 98 + 15) & ~15;    // a wave's output run of one ROI: CH channels x 49 bins
  char* scr = (char*)(cnt + 16) + wave * SCR;
  const int last = (HW - 1) * CB;              // byte offset of the slice's last cell
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int nbl = p.N * ST_LEVELS;
  const int logical = xcd_remap(blockIdx.x, gridDim.x);  // the blocks of one slice (its images and levels) share an XCD's L2
  const int sl = logical / nbl, bl = logical - sl * nbl;
  const int b = bl / ST_LEVELS, l = bl - b * ST_LEVELS;
  const int c0 = sl * CH;
  unsigned long long tp[5] = {0, 0, 0, 0, 0}, t0 = 0, t1;
  if constexpr (PROF) t0 = __builtin_amdgcn_s_memtime();
#define ST_CLK(K) do { if constexpr (PROF) { t1 = __builtin_amdgcn_s_memtime(); tp[K] += t1 - t0; t0 = t1; } } while (0)
  // ---- the ROIs of this (image, l), by k ------------------------------------------------------------------------------------
  if (tid < 16) cnt[tid] = 0;
  __syncthreads();
  for (int m = tid; m < p.M; m += NT) {
    const unsigned d = (unsigned)cls[m] - (unsigned)(bl * ST_LEVELS);
    if (d < (unsigned)ST_LEVELS) atomicAdd(&cnt[d], 1);
  }
  __syncthreads();
  int start[ST_LEVELS + 1];
  start[0] = 0;
#pragma unroll
  for (int k = 0; k < ST_LEVELS; ++k) start[k + 1] = start[k] + __builtin_amdgcn_readfirstlane(cnt[k]);
  if (start[ST_LEVELS] == 0) return;
  ST_CLK(0);
  // ---- the slice: one contiguous run of the chunk-major copy -> registers -> LDS --------------------------------------------
  cellv own[SB];
  const char* src = p.cm + ((long)b * (p.C / CH) + sl) * HW * CB;
#pragma unroll
  for (int j = 0; j < SB; ++j) own[j] = *(const cellv*)(src + (long)min(tid + j * NT, HW - 1) * CB);
  for (int m = tid; m < p.M; m += NT) {
    const unsigned d = (unsigned)cls[m] - (unsigned)(bl * ST_LEVELS);
    if (d < (unsigned)ST_LEVELS) {
      int st0 = start[0];
#pragma unroll
      for (int k = 1; k < ST_LEVELS; ++k) st0 = d == (unsigned)k ? start[k] : st0;
      list[st0 + atomicAdd(&cnt[8 + d], 1)] = (unsigned short)m;
    }
  }
#pragma unroll
  for (int j = 0; j < SB; ++j) *(cellv*)(smem + (size_t)min(tid + j * NT, HW - 1) * CB) = own[j];
  __syncthreads();
  ST_CLK(1);
  // ---- doubling steps: cell i takes the maximum with cell i + stride (stride = s cells along a row, s * W cells down a column).
  // No edge cases: a partner beyond the row's end is the next row's cell, one beyond the map the last cell - real values in cells
  // that cover no valid block (x + 2s > W or y + 2s > H: never looked up, never the partner of a valid cell at a later level)
  int off[SB];
#pragma unroll
  for (int j = 0; j < SB; ++j) off[j] = min(tid + j * NT, HW - 1) * CB;
  auto step = [&](int stride_bytes) {
    cellv o[SB];
#pragma unroll
    for (int j = 0; j < SB; ++j) o[j] = *(lds_cell_t)(uintptr_t)(lds0 + (unsigned)min(off[j] + stride_bytes, last));
#pragma unroll
    for (int j = 0; j < SB; ++j)
#pragma unroll
      for (int e = 0; e < VD; ++e) own[j][e] = pk_max_i16(own[j][e], o[j][e]);
    __syncthreads();  // every partner has been read (and: every wave is done pooling the previous level out of the table)
#pragma unroll
    for (int j = 0; j < SB; ++j) *(cellv*)(smem + off[j]) = own[j];
    __syncthreads();
  };
  for (int s = 1; s < (1 << l); s <<= 1) step(s * CB);
  ST_CLK(2);
  // ---- level by level down the columns; the ROIs of each level ------------------------------------------------------------------
  const int T = 1 << l;
  int curk = 0;
#pragma unroll 1
  for (int k = 0; k < ST_LEVELS; ++k) {
    int seg0 = start[0], seg1 = start[1];
#pragma unroll
    for (int q = 1; q < ST_LEVELS; ++q) {
      seg0 = k == q ? start[q] : seg0;
      seg1 = k == q ? start[q + 1] : seg1;
    }
    if (seg0 == seg1) continue;
    for (; curk < k; ++curk) step((W << curk) * CB);
    ST_CLK(3);
    const int S = 1 << k;
    for (int base = seg0 + wave; base < seg1; base += NW * ST_BATCH) {
      int my = 0;
      if (lane < ST_BATCH) my = list[min(base + lane * NW, seg1 - 1)];
      unsigned rq[ST_BATCH];
#pragma unroll
      for (int q = 0; q < ST_BATCH; ++q) rq[q] = rec[(long)__builtin_amdgcn_readlane(my, q) * 64 + lane];
#pragma unroll
      for (int q = 0; q < ST_BATCH; ++q) {
        if (base + q * NW >= seg1) break;
        const int m = __builtin_amdgcn_readlane(my, q);
        const unsigned r = rq[q];
        const unsigned meta = (unsigned)__builtin_amdgcn_readlane((int)r, 60);
        const float mul = __builtin_bit_cast(float, __builtin_amdgcn_readlane((int)r, 62));
        const int max_nr = meta & 0xff, max_nc = meta >> 8 & 0xff;
        const int y0 = r & 0xff, y1 = r >> 8 & 0xff, x0 = r >> 16 & 0xff, x1 = r >> 24;
        const int keep = y1 < y0 ? 0 : -1;  // an empty bin is +0
        cellv acc;
        if (max_nr <= 2 && max_nc <= 2) {
          const unsigned r0 = __umul24((unsigned)y0, (unsigned)W), r1 = __umul24((unsigned)y1, (unsigned)W);
          const cellv a = *(lds_cell_t)(uintptr_t)(lds0 + (r0 + (unsigned)x0) * CB);
          const cellv bq = *(lds_cell_t)(uintptr_t)(lds0 + (r0 + (unsigned)x1) * CB);
          const cellv c = *(lds_cell_t)(uintptr_t)(lds0 + (r1 + (unsigned)x0) * CB);
          const cellv d = *(lds_cell_t)(uintptr_t)(lds0 + (r1 + (unsigned)x1) * CB);
#pragma unroll
          for (int e = 0; e < VD; ++e) acc[e] = pk_max_i16(pk_max_i16(a[e], bq[e]), pk_max_i16(c[e], d[e]));
        } else {
#pragma unroll
          for (int e = 0; e < VD; ++e) acc[e] = (int)0x80008000u;
          for (int i = 0; i < max_nr; ++i) {
            const unsigned row = __umul24((unsigned)min(y0 + i * S, y1), (unsigned)W);
            for (int j = 0; j < max_nc; ++j) {
              const cellv x = *(lds_cell_t)(uintptr_t)(lds0 + (row + (unsigned)min(x0 + j * T, x1)) * CB);
#pragma unroll
              for (int e = 0; e < VD; ++e) acc[e] = pk_max_i16(acc[e], x[e]);
            }
          }
        }
        // the ROI's CH x 49 values are ONE run of A: through the wave's LDS scratch (2-byte writes at [channel][bin]) they leave as
        // one 8- / 16-byte store per lane instead of CH 2-byte stores (a wave's LDS operations execute in order: the scratch is
        // reused from ROI to ROI without a wait)
        if (lane < 49) {
          unsigned short* sp = (unsigned short*)scr + lane;
#pragma unroll
          for (int e = 0; e < VD; ++e) {
            const uint32_t y = (uint32_t)(bf16x2_order(acc[e]) & keep);
            typedef float f32x2_t __attribute__((ext_vector_type(2)));
            typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
            const f32x2_t f = f32x2_t{__builtin_bit_cast(float, y << 16), __builtin_bit_cast(float, y & 0xffff0000u)} * mul;
            const uint32_t o = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2_t));
            sp[(2 * e) * 49] = (unsigned short)(o & 0xffffu);
            sp[(2 * e + 1) * 49] = (unsigned short)(o >> 16);
          }
          const cellv v = *(const volatile cellv*)(scr + lane * CB);
          *(cellv*)(p.out + ((long)m * p.ld_out + (long)c0 * 49) * 2 + lane * CB) = v;
        }
      }
    }
    if constexpr (PROF) {
      __syncthreads();  // (a profile build waits for the level's slowest wave here; the product waits in the next step)
      ST_CLK(4);
    }
  }
  if constexpr (PROF) {
    if (tid == 0) {
      for (int q = 0; q < 5; ++q) atomicAdd(&g_st_prof[q], tp[q]);
      atomicAdd(&g_st_prof[5], 1ull);
      atomicAdd(&g_st_prof[6], (unsigned long long)start[ST_LEVELS]);
    }
  }
#undef ST_CLK
}

// ---- the forward's host side: which kernel pools a shape (roi_fwd_plan) and its launch (roi_fwd_launch) ---------------------
enum RoiKind { RK_NONE, RK_SPARSE_TABLE, RK_WALK, RK_LANE, RK_MAP64, RK_MAP8, RK_POOL7, RK_GENERIC, RK_ALIGN_LANE };

struct RoiFwdQuery {
  int N, H, W, C, P, M, mode, in_dtype, out_dtype;
  bool argmax, out_t;  // the arg-max / the transposed copy is wanted
  int t_c0;            // first channel whose rows of out_t are needed
  // 16-byte alignment of the map's base; of out's base and row pitch; of out_t's (the whole-map kernels need all that apply, the
  // ROIAlign lane kernel the first, roi_pool7_kernel the second)
  bool feat16, out16, out_t16;
  unsigned skip;  // bit k: leave RoiKind k out (its launch was refused)
  int map8_from;  // first entry of the 8-ROI kernel's cascade (roi_map8_bf16 / _f32) still to consider
};
static bool roi_skipped(const RoiFwdQuery& q, RoiKind k) { return (q.skip >> k & 1u) != 0; }

// the 64-ROI kernel's launch: a plan of its own, because it also follows the lane-per-bin kernels for the A^T tail chunks
struct RoiMap64Plan { const void* fn; unsigned grid; int threads; size_t smem; int lds_px, cpb, pf, c_begin; };

struct RoiFwdPlan {
  RoiKind kind = RK_NONE;
  const void* fn = nullptr;  // the kernel: the kind's template with ...
  int vd = 4, nck = 1, nwv = 8, nsg = 1, sb = 0, occ = 1, ch = 0, prof = 0;  // ... these arguments (those the kind has)
  unsigned grid_x = 0, grid_y = 1, block = 256;
  size_t smem = 0;
  int lds_cap = 0;  // dynamic LDS the kernel has to be allowed first (0: it stays below the default)
  int lds_px = 0, gpw = 0, lane_g = 0, lane_reps = 0, walk = 0, walk_wp = 0;  // the RoiParams fields the kernel reads
  unsigned walk_wmagic = 0;
  RoiMap64Plan m64{};       // kind RK_MAP64; or, with m64_tail, the launch that follows the kind's own for the A^T tail chunks
  bool m64_tail = false, transpose = false;  // transpose: general shapes with out_t - the kernel pools into `out` only, then drn_transpose2d
  int cascade = 0;          // RK_MAP8: its entry of the cascade
  size_t ws_bytes = 0;      // workspace the kind pools from (0: none) ...
  bool ws_required = false;  // ... and whether it is refused without (else: it pools without, slower)
  void launch(RoiKind k, unsigned gx, unsigned gy, unsigned blk, size_t lds, int cap) {
    kind = k; grid_x = gx; grid_y = gy; block = blk; smem = lds; lds_cap = cap;
  }
};
#define ROI_PICK(COND, ...) if (COND) pl.fn = (const void*)__VA_ARGS__

static size_t roi_st_align(size_t x) { return (x + 255) & ~(size_t)255; }
// cells of VD dwords for this map under the sparse-table kernel (0: not its shape)
static int roi_st_vd(const DrnTune& t, int N, int H, int W, int C, int M) {
  if (!t.roi_st || H < 2 || H > 255 || W < 2 || W > 255 || N < 1 || N > 10 || M < 64 || M > 16384) return 0;
  const size_t hw = (size_t)H * W;
  if (hw > 30 * 1024) return 0;
  const size_t list = (size_t)((M + 7) & ~7) * 2 + 64;  // ROI list + counters; then a 208- / 400- / 784-byte scratch per wave
  const bool fits8 = C % 8 == 0 && hw * 16 + list + 16 * 784 <= 160 * 1024, fits4 = C % 4 == 0 && hw * 8 + list + 16 * 400 <= 160 * 1024;
  // 2 channels per cell: the stride-8 maps of the largest test-time scales (1200 x 1600: 150 x 200 cells), twice the blocks
  const bool fits2 = C % 2 == 0 && hw * 4 + list + 16 * 208 <= 160 * 1024;
  if (!fits8 && !fits4) return fits2 && (t.roi_st == 2 || M >= 400) ? 1 : 0;
  if (t.roi_st == 2) return fits8 ? 4 : fits4 ? 2 : 0;
  // default: where the table's fixed cost (staging + <= 8 doubling steps per block, ~HW) is below what the window kernels spend
  // reading every ROI's cells (~M x ROI area): profiles/r6_17_roi_st.txt, r6_18 (R = 250 / 1000 / 4000)
  if (fits8) return (M >= 600 && hw >= 3000) || (M >= 1500 && hw >= 1800) ? 4 : 0;
  return fits4 && M >= 400 ? 2 : 0;
}

// chunks per block of the lane-per-bin kernels: as many as fit 38 KB (four 8-wave blocks per CU), else 76 KB (two), else one chunk
// in <= 154 KB; 0: the map slice of even ONE chunk does not fit
static int roi_lane_chunks(int H, int W, int C) {
  if (C % 8) return 0;
  const size_t per_chunk = (size_t)H * W * 16;
  size_t budget = 38 * 1024;
  for (int pass = 0; pass < 3; ++pass, budget = pass == 1 ? 76 * 1024 : 154 * 1024)
    for (int k = 8; k >= 1; k >>= 1)
      if ((C / 8) % k == 0 && per_chunk * k <= budget) return k;
  return 0;
}

static unsigned roi_wmagic(int W) { return (unsigned)((0x100000000ull + (unsigned)W - 1) / (unsigned)W); }

// The 64-ROI kernel from channel c_begin on; false: not its shape.
// Chunks per block (t.roi_cpb): stand-alone the launch gets faster with 4-8 (141 -> 117-125 us at 14x14 / R = 2000: bin bounds and item
// table once per block, next slice prefetched), but INSIDE the training step it runs beside the optimizer pass and the
// trunk's conv chain, and 512 long-lived blocks - a static partition of the work - lose to 4096 short ones that the
// dispatcher balances over whichever CUs are free: same-box A/B of the whole step 646 img/s (1), 643 (2), 634 (8) against
// 646 with the previous kernel (profiles/r2_26_roi_ab.txt).  Default 1; the knob stays for stand-alone pooling (inference).
static bool roi_map64_plan(const RoiFwdQuery& q, const DrnTune& t, int cus, int c_begin, RoiMap64Plan& o) {
  if (!t.roi_map64 || q.C % G64_CH || q.H > 255 || q.W > 255) return false;
  // LDS a block may take for its map slice + result tile (+ ~1.5 KB static): 154 KB = one block per CU with the whole
  // slice of maps up to ~80x80; DRN_TUNE_ROI_LDS_KB = 76 stages larger maps in bands so that TWO blocks share a CU
  const size_t tile_b = (size_t)ROI_G64 * G64_PITCH, budget = (size_t)t.roi_lds_kb * 1024 - tile_b;
  size_t map_b = ((size_t)q.H * q.W * 16 + 15) & ~(size_t)15;
  o.lds_px = q.H * q.W;
  if (map_b > budget) {  // bands of whole rows
    const int rows = (int)(budget / ((size_t)q.W * 16));
    if (rows < 8) return false;
    o.lds_px = rows * q.W;
    map_b = ((size_t)o.lds_px * 16 + 15) & ~(size_t)15;
  }
  size_t smem = map_b + tile_b;
  // <= 76 KB: two blocks per CU (the 14x14 .. 38x38 maps), the tuned 512 threads.  Up to 156 KB - the 40x60 .. 63x100 maps of
  // real-size training images - ONE block per CU still stages its 8-channel map slice once per 64 ROIs; the 8-ROI whole-map
  // kernel that these maps used to fall to re-stages it per 8 ROIs (2.9 GB through L2 per call at 63x92: 1.5 ms, half of the
  // eager step at 1000x1464, `profiles/r2_15_*`); 1024 threads there - the window scans are latency-bound and eight waves per
  // CU hide little of it (63x92 map, 2000 proposals: 467 -> 394 us)
  o.threads = smem > 76 * 1024 && t.roi_map64 == 512 ? 1024 : t.roi_map64;
  o.fn = o.threads >= 1024 ? (const void*)roi_pool7_map64_kernel<4> : o.threads >= 512 ? (const void*)roi_pool7_map64_kernel<7>
                                                                                       : (const void*)roi_pool7_map64_kernel<13>;
  // prefetch mode: whole map in one band, two buffers within the same blocks-per-CU class, <= 2 pixels per thread
  const size_t cls = smem <= 76 * 1024 ? 76 * 1024 : 156 * 1024;
  o.pf = t.roi_prefetch && o.lds_px == q.H * q.W && smem + map_b <= cls && q.H * q.W <= 2 * o.threads;
  if (o.pf) smem += map_b;
  if (smem > 156 * 1024) return false;
  const int ngroups = (q.M + ROI_G64 - 1) / ROI_G64;
  // channel chunks per block (tune knob, default 1): the bin bounds of a 64-ROI group and the per-thread item table are
  // paid once per `cpb` chunks instead of once per chunk; largest power of two <= the knob that still leaves two blocks
  // for every CU
  int cpb = t.roi_cpb;
  const int nchunks = (q.C - c_begin) / G64_CH;
  while (cpb > 1 && (nchunks % cpb || (long)(nchunks / cpb) * ngroups < 2L * cus)) cpb >>= 1;
  o.cpb = cpb;
  o.c_begin = c_begin;
  o.grid = (unsigned)((nchunks / cpb) * ngroups);
  o.smem = smem;
  return true;
}

// A (all channels) through the lane-per-bin family - sparse table, walking or plain lane kernel, in this order; false: none
// of them takes the shape
static bool roi_lane_family_plan(const RoiFwdQuery& q, const DrnTune& t, int cus, RoiFwdPlan& pl) {
  const int H = q.H, W = q.W, C = q.C, M = q.M;
  if (!t.roi_lane || C % 8) return false;
  size_t per_chunk = (size_t)H * W * 16;
  int nck = roi_lane_chunks(H, W, C);
  int vd = 4;
  if (!nck && C % 4 == 0 && (size_t)H * W * 8 <= 154 * 1024)  // 4-channel cells: one 8-byte-per-pixel chunk per block
    nck = 1, vd = 2, per_chunk = (size_t)H * W * 8;
  const int svd = roi_st_vd(t, q.N, H, W, C, M);
  if (svd && !roi_skipped(q, RK_SPARSE_TABLE)) {  // large maps: four table cells per bin instead of the window's ~77
    const int HW = H * W, cells = (HW + 1023) / 1024;  // slice cells per thread, and the instance that holds them
    const int sb = svd == 1 ? (cells <= 20 ? 20 : 30) : svd == 2 ? (cells <= 10 ? 10 : cells <= 15 ? 15 : 20) : (cells <= 5 ? 5 : 10);
    pl.vd = svd; pl.sb = sb;
    pl.prof = t.roi_st_prof && ((svd == 2 && sb == 15) || (svd == 4 && sb == 10));  // (the two profile builds there are)
    ROI_PICK(svd == 1 && sb == 20, roi_pool7_st_kernel<1, 20>); ROI_PICK(svd == 1 && sb == 30, roi_pool7_st_kernel<1, 30>);
    ROI_PICK(svd == 2 && sb == 10, roi_pool7_st_kernel<2, 10>); ROI_PICK(svd == 2 && sb == 15, roi_pool7_st_kernel<2, 15>);
    ROI_PICK(svd == 2 && sb == 20, roi_pool7_st_kernel<2, 20>);
    ROI_PICK(svd == 4 && sb == 5, roi_pool7_st_kernel<4, 5>); ROI_PICK(svd == 4 && sb == 10, roi_pool7_st_kernel<4, 10>);
    ROI_PICK(pl.prof && svd == 2, roi_pool7_st_kernel<2, 15, true>); ROI_PICK(pl.prof && svd == 4, roi_pool7_st_kernel<4, 10, true>);
    pl.launch(RK_SPARSE_TABLE, (unsigned)(C / (svd * 2)) * q.N * ST_LEVELS, 1, 1024,
              (size_t)HW * svd * 4 + (size_t)((M + 7) & ~7) * 2 + 64 + 16 * (svd == 1 ? 208 : svd == 2 ? 400 : 784), 160 * 1024);
    // the chunk-major copy of the map, a 256-byte record and a class byte per ROI
    pl.ws_bytes = roi_st_align((size_t)q.N * H * W * C * 2) + roi_st_align((size_t)M * 256) + roi_st_align((size_t)M);
    pl.ws_required = true;
    return true;
  }
  if (!nck) return false;
  // maps the walking kernel takes: one 8-channel chunk per block (beyond the 38-KB class) that fits with its table
  if (nck == 1 && vd == 4 && t.roi_lane != 2 && W >= 2 && (size_t)H * W * 16 + 64 * WALK_TAB * 4 + 16 <= 160 * 1024 &&
      (H * W + 1023) / 1024 <= 10) {
    // (refused: the whole family is - the plain lane kernel is not its fallback)
    if (roi_skipped(q, RK_WALK)) return false;
    const size_t lds_max = 160 * 1024;
    // slice + window table + counter
    auto need = [&](int nsg_, int wp_) { return (size_t)H * wp_ * 16 + (size_t)64 * nsg_ * WALK_TAB * 4 + 16; };
    const bool big1 = need(1, W | 1) > 80 * 1024;  // one block per CU: 16 waves
    // the largest maps: first the odd pitch goes, then the second sub-group of ROIs
    // 128 ROIs per block (64 with DRN_TUNE_ROI_LANE = 3, for tests) where the table fits: half the stagings and barriers per item
    int wp = W | 1, nsg = t.roi_walk_nsg == 2 && (big1 || need(2, wp) <= 80 * 1024) ? 2 : 1;
    if (need(nsg, wp) > lds_max) wp = W;
    if (need(nsg, wp) > lds_max) nsg = 1;
    const int ngr = (M + 64 * nsg - 1) / (64 * nsg);
    const int nchunks = C / 8;
    // chunks per block: 8 (the pieces of one 128-byte line per pixel) unless fewer fill the rounds of blocks better - a VALU-bound
    // block per CU (two of the 8-wave blocks), so a grid of 1.5 rounds takes the time of 2 (75x122 / R = 1500: 12 groups x 16
    // chunk groups = 192 blocks: 244 us; 2 chunks per block = 768 blocks = 3 rounds: 204 us, profiles/r5_40_roi_walk_big.txt)
    const long slots = (long)cus * (big1 ? 1 : 2);
    int walk = 1;
    double best = -1.0;
    for (int w = 8, lg = 0; w >= 1; w >>= 1, ++lg) {
      if (nchunks % w != 0) continue;
      if (t.roi_lane_reps > 0 && w > t.roi_lane_reps) continue;
      const long grid = (long)ngr * (nchunks / w);
      const double score = (double)grid / (double)((grid + slots - 1) / slots * slots) * (1.0 - 0.015 * lg);
      if (t.roi_lane_reps > 0) { walk = w; break; }  // (knob: the largest admissible walk <= its value)
      if (score > best) best = score, walk = w;
    }
    // block shape: one block per CU -> 16 waves; two blocks per CU -> 16-wave blocks (eight waves per SIMD, <= 64 VGPRs) for slices
    // of up to 3072 cells, else 8-wave blocks (43x58: 111.9 vs 122.5 us; 50x76: 170.6 vs 161.9 us - profiles/r5_47_roi_walk_nsg2.txt)
    const bool w16 = !big1 && H * W <= 3072;
    const int nt = big1 || w16 ? 1024 : 512, sb = (H * W + nt - 1) / nt;
    pl.nwv = nt / 64; pl.nsg = nsg; pl.occ = w16 ? 2 : 1;
    pl.sb = w16 ? 3 : !big1 ? (sb <= 8 ? 8 : 10) : (sb <= 6 ? 6 : 10);
    pl.walk = walk; pl.walk_wp = wp; pl.walk_wmagic = roi_wmagic(W);
#define WALK_PICK(NWV_, NSG_, SB_, OCC_) \
  ROI_PICK(pl.nwv == NWV_ && nsg == NSG_ && pl.sb == SB_ && pl.occ == OCC_, roi_pool7_walk_kernel<NWV_, NSG_, 4, SB_, OCC_>)
    WALK_PICK(16, 2, 3, 2); WALK_PICK(16, 1, 3, 2);
    WALK_PICK(8, 2, 8, 1); WALK_PICK(8, 2, 10, 1); WALK_PICK(8, 1, 8, 1); WALK_PICK(8, 1, 10, 1);
    WALK_PICK(16, 2, 6, 1); WALK_PICK(16, 2, 10, 1); WALK_PICK(16, 1, 6, 1); WALK_PICK(16, 1, 10, 1);
#undef WALK_PICK
    pl.launch(RK_WALK, (unsigned)ngr * (nchunks / walk), 1, nt, need(nsg, wp), 160 * 1024);
    pl.ws_bytes = (size_t)q.N * H * W * C * 2;  // the chunk-major copy: the slices are staged as contiguous runs
    return true;
  }
  if (roi_skipped(q, RK_LANE)) return false;
  const size_t smem = per_chunk * nck;
  const bool big = smem > 76 * 1024;  // one block per CU: 16 waves
  // ROIs per block: 32 (four per wave) - the staging of the slice is then ~1/8 of the block's output bytes at 14x14; large
  // maps (one chunk of 60+ KB per block) take 64 so that the slice is staged half as often
  pl.lane_g = smem > 38 * 1024 ? 64 : 32;
  int ngroups = (M + pl.lane_g - 1) / pl.lane_g;
  // one block per CU (slices beyond 76 KB): every group of 64 ROIs re-stages the slice from L2 - 32 groups x 64 slices x
  // 120 KB = 250 MB at 50x76.  A block walks `lane_reps` groups with one staged slice as long as >= 2 rounds of blocks remain
  pl.lane_reps = 1;
  if (big) {
    const long blocks1 = (long)ngroups * (C / (2 * vd * nck));
    // (4-channel cells - the DC5 stride-8 map: a slice is staged 8 bytes per 4-KB pixel, i.e. a whole 128-byte line per cell from
    // the Infinity Cache: 7.9 GB per launch with 4 groups per staged slice; with all of a slice's groups on one block - still
    // two rounds of blocks - the launch went from 1242 to 948 us, profiles/r5_28_*)
    int reps = t.roi_lane_reps > 0 ? t.roi_lane_reps : (vd == 2 ? 32 : 4);
    while (reps > 1 && blocks1 / reps < 2L * cus) reps >>= 1;
    pl.lane_reps = reps;
    ngroups = (ngroups + reps - 1) / reps;
  }
  // (one block per CU - maps beyond ~4700 pixels: with a block per group of 64 ROIs this kernel measured 372 vs 325 us for the
  // 64-ROI kernel at 63x92 and went there only for maps that kernel stages in two row bands; with four groups per staged
  // slice it is 293 vs 330 us at 63x92 and 260 vs 368 us at 75x122 and takes every map whose chunk fits)
  pl.vd = vd; pl.nck = nck; pl.nwv = big ? 16 : 8;
  ROI_PICK(vd == 4 && nck == 8, roi_pool7_lane_kernel<8>); ROI_PICK(vd == 4 && nck == 4, roi_pool7_lane_kernel<4>);
  ROI_PICK(vd == 4 && nck == 2, roi_pool7_lane_kernel<2>);
  ROI_PICK(vd == 4 && nck == 1 && !big, roi_pool7_lane_kernel<1>); ROI_PICK(vd == 4 && nck == 1 && big, roi_pool7_lane_kernel<1, 16>);
  ROI_PICK(vd == 2 && big, roi_pool7_lane_kernel<1, 16, 2>); ROI_PICK(vd == 2 && !big, roi_pool7_lane_kernel<1, 8, 2>);
  pl.launch(RK_LANE, (unsigned)ngroups * (C / (2 * vd * nck)), 1, pl.nwv * 64, smem, 156 * 1024);
  return true;
}

// The 8-ROI whole-map kernel's cascade - channel slice per block and the LDS it may take: 32 channels wide when two blocks fit a CU
// (the 14x14 .. 28x28 training maps), else the widest slice whose map fits at all - the 43x58 .. 75x100 maps of test-time scales
// need 16 or 8 channels and most of a CU's LDS (one block per CU), which still beats the per-ROI window kernels by 3-4x there.
// (ch 0, bf16: maps too large for two 8-ROI blocks per CU - inference at real image sizes, no A^T - take the 64-ROI kernel first:
// the 8-ROI one would re-stage its map slice per 8 proposals)
struct RoiMap8Entry { int ch; size_t budget; };
constexpr size_t MAP8_TWO = 80 * 1024, MAP8_ONE = 156 * 1024;
constexpr RoiMap8Entry roi_map8_bf16[] = {{32, MAP8_TWO}, {64, MAP8_TWO}, {16, MAP8_TWO}, {8, MAP8_TWO}, {0, 0},
                                          {32, MAP8_ONE}, {16, MAP8_ONE}, {8, MAP8_ONE}};
constexpr RoiMap8Entry roi_map8_f32[] = {{32, MAP8_TWO}, {16, MAP8_TWO}, {8, MAP8_TWO}, {4, MAP8_TWO},
                                         {16, MAP8_ONE}, {8, MAP8_ONE}, {4, MAP8_ONE}};

// Which kernel pools the shape, and its launch.  Pure: no HIP call, no global, no pointer - drn_roi_pool_workspace_bytes asks it
// without a device.  The order of the candidates is the order of preference; `q.skip` / `q.map8_from` take out what a launch refused.
static RoiFwdPlan roi_fwd_plan(const RoiFwdQuery& q0, const DrnTune& t, int cus) {
  RoiFwdQuery q = q0;
  RoiFwdPlan pl;
  const int H = q.H, W = q.W, C = q.C, M = q.M;
  const bool bf16 = q.in_dtype == DRN_BF16 && q.out_dtype == DRN_BF16, f32 = q.in_dtype == DRN_F32 && q.out_dtype == DRN_F32;
  for (;;) {
    // whole-map kernels: 7x7 ROIPool, same in/out dtype, no argmax, 16-B aligned runs
    if (q.mode == 0 && q.P == 7 && !q.argmax && (bf16 || f32) && q.feat16 && q.out16 && (!q.out_t || q.out_t16)) {
      if (bf16 && M >= ROI_G64) {  // the training operand (pair), and A alone at inference (46 vs 83 us at
        // 14x14, 194 vs 433 us at 50x76 against the 8-ROI whole-map kernels: tools/roi_a_alone_bench.py)
        // round 4: A from the lane-per-bin kernels; the 64-ROI kernel - full 128-byte A^T lines - then only for the channel
        // chunks whose A^T rows the fc6 dW still reads (the tail its peel takes; it writes their A runs again, same values)
        // (built and measured: the tail's A^T rows as 2-byte stores from the lane kernel itself - 49 partial lines per
        // instruction - cost 40 us for 4.7 MB at the bench shape; the 64-ROI kernel's full lines cost ~8 us as a launch)
        const int cb = q.out_t ? q.t_c0 / G64_CH * G64_CH : C;
        const bool few_t = !q.out_t || (long)(C - cb) * 8 <= C;
        const bool tail = q.out_t && cb < C;
        if (few_t && C % G64_CH == 0 && (!tail || (!roi_skipped(q, RK_MAP64) && roi_map64_plan(q, t, cus, cb, pl.m64))) &&
            roi_lane_family_plan(q, t, cus, pl)) {
          pl.m64_tail = tail;
          return pl;
        }
        if ((q.out_t || t.roi_map64_a) && !roi_skipped(q, RK_MAP64) && roi_map64_plan(q, t, cus, 0, pl.m64)) {
          pl.kind = RK_MAP64;
          return pl;
        }
      }
      const RoiMap8Entry* casc = bf16 ? roi_map8_bf16 : roi_map8_f32;
      const int ncasc = bf16 ? (int)(sizeof(roi_map8_bf16) / sizeof(RoiMap8Entry)) : (int)(sizeof(roi_map8_f32) / sizeof(RoiMap8Entry));
      const int es = bf16 ? 2 : 4;
      for (int i = q.map8_from; i < ncasc; ++i) {
        const int ch = casc[i].ch;
        if (ch == 0) {
          if (M < ROI_G64 || roi_skipped(q, RK_MAP64) || !roi_map64_plan(q, t, cus, 0, pl.m64)) continue;
          pl.kind = RK_MAP64;
          return pl;
        }
        const size_t smem = (((size_t)H * W * ch * es + 15) & ~(size_t)15) + (size_t)ROI_GROUP * ch * 49 * es;
        if (C % ch || smem > casc[i].budget) continue;
        const int ngroups = (M + ROI_GROUP - 1) / ROI_GROUP;
        // groups per block: keep the bytes staged per block (H*W pixels) below the bytes it writes (8 ROIs x 49 bins x 2
        // copies per group) - 1 for the 14x14 training map, up to 10 for a 75x100 map
        pl.gpw = min(max((H * W + 783) / 784, 1), 16);
        pl.cascade = i; pl.ch = ch;
        ROI_PICK(bf16 && ch == 32, roi_pool7_map_kernel<DRN_BF16, 32>); ROI_PICK(bf16 && ch == 64, roi_pool7_map_kernel<DRN_BF16, 64>);
        ROI_PICK(bf16 && ch == 16, roi_pool7_map_kernel<DRN_BF16, 16>); ROI_PICK(bf16 && ch == 8, roi_pool7_map_kernel<DRN_BF16, 8>);
        ROI_PICK(f32 && ch == 32, roi_pool7_map_kernel<DRN_F32, 32>); ROI_PICK(f32 && ch == 16, roi_pool7_map_kernel<DRN_F32, 16>);
        ROI_PICK(f32 && ch == 8, roi_pool7_map_kernel<DRN_F32, 8>); ROI_PICK(f32 && ch == 4, roi_pool7_map_kernel<DRN_F32, 4>);
        pl.launch(RK_MAP8, (unsigned)((C / ch) * ((ngroups + pl.gpw - 1) / pl.gpw)), 1, 256, smem, smem > 48 * 1024 ? 156 * 1024 : 0);
        return pl;
      }
    }
    // ROIAlign, bf16 -> bf16, P = 7, channels in chunks of 8, a slice of the map in LDS: the lane-per-bin form
    if (q.mode == 1 && q.P == 7 && !q.out_t && bf16 && t.roi_lane && q.feat16 && M >= 32 && !roi_skipped(q, RK_ALIGN_LANE) && C % 8 == 0) {
      int nck = roi_lane_chunks(H, W, C);
      if (nck) {
        // (64 fp32 accumulators per lane at 8 chunks: 4 chunks per block keep the wave under 128 registers - two blocks per CU)
        if (nck > 4) nck = 4;
        const size_t smem = (size_t)H * W * 16 * nck;
        pl.nck = nck; pl.lane_g = smem > 38 * 1024 ? 64 : 32;
        ROI_PICK(nck == 4, roi_align7_lane_kernel<4>); ROI_PICK(nck == 2, roi_align7_lane_kernel<2>); ROI_PICK(nck == 1, roi_align7_lane_kernel<1>);
        pl.launch(RK_ALIGN_LANE, (unsigned)((M + pl.lane_g - 1) / pl.lane_g) * (C / (8 * nck)), 1, 512, smem, 156 * 1024);
        return pl;
      }
    }
    if (!q.out_t) break;
    // general shapes: pool into `out` alone - whichever kernel then takes the shape, without a workspace -, then the transpose pass
    q.out_t = false;
    pl.transpose = true;
  }
  // ROIPool on a full 64-channel chunk stages the box window in LDS: up to 256 pixels (25 KB bf16 / 64 KB f32... capped)
  if (q.mode == 0 && C % RP_CH == 0) {
    const int es = drn_esize(q.in_dtype);
    int px = H * W < 256 ? H * W : 256;
    if ((size_t)px * RP_CH * es > 32 * 1024) px = 32 * 1024 / (RP_CH * es);
    pl.lds_px = px;
    pl.smem = (size_t)px * RP_CH * es;
  }
  // 7x7 ROIPool, no argmax wanted, whole map fits the staging tile, channels in full 64-wide chunks, 16-B aligned output rows
  if (q.mode == 0 && q.P == 7 && !q.argmax && C % RP_CH == 0 && H * W <= pl.lds_px && pl.lds_px > 0 && H * W <= 256 && q.out16 &&
      (bf16 || f32)) {
    ROI_PICK(bf16, roi_pool7_kernel<DRN_BF16, DRN_BF16>); ROI_PICK(f32, roi_pool7_kernel<DRN_F32, DRN_F32>);
    pl.launch(RK_POOL7, M, (C / RP_CH + 3) / 4, 256, pl.smem, 0);
    return pl;
  }
#define GEN_PICK(DI, DO) \
  ROI_PICK(q.in_dtype == DI && q.out_dtype == DO, (q.mode == 0 ? roi_kernel<DI, DO, 0> : roi_kernel<DI, DO, 1>))
  GEN_PICK(DRN_BF16, DRN_BF16); GEN_PICK(DRN_F32, DRN_F32); GEN_PICK(DRN_F32, DRN_BF16); GEN_PICK(DRN_BF16, DRN_F32);
#undef GEN_PICK
  if (pl.fn) pl.launch(RK_GENERIC, M, (C + RP_CH - 1) / RP_CH, 256, pl.smem, 0);  // (other dtypes: RK_NONE - no kernel)
  return pl;
}

#undef ROI_PICK
static bool roi_map64_launch(const RoiMap64Plan& m, RoiParams p, hipStream_t st) {
  p.lds_px = m.lds_px; p.cpb = m.cpb; p.pf = m.pf; p.c_begin = m.c_begin;
  if (!drn_launch::allow_lds(m.fn, 156 * 1024)) return false;
  void* args[] = {(void*)&p};
  (void)hipLaunchKernel(m.fn, dim3(m.grid), dim3(m.threads), args, m.smem, st);
  return true;
}

// Issues what the plan says.  false: refused - the kernel may not take its LDS, or the workspace it requires is missing,
// misaligned or too small - and nothing was launched; the caller plans again without that kind.
static bool roi_fwd_launch(const RoiFwdPlan& pl, const RoiParams& p0, void* ws, size_t ws_bytes, hipStream_t st) {
  if (pl.kind == RK_MAP64) return roi_map64_launch(pl.m64, p0, st);
  RoiParams p = p0;
  p.lds_px = pl.lds_px; p.gpw = pl.gpw; p.lane_g = pl.lane_g; p.lane_reps = pl.lane_reps;
  p.walk = pl.walk; p.walk_wp = pl.walk_wp; p.walk_wmagic = pl.walk_wmagic;
  if (pl.kind != RK_MAP8) p.out_t = nullptr;  // (A only; the 64-ROI kernel follows for the A^T tail chunks)
  const bool ws_ok = ws && (((uintptr_t)ws) & 15) == 0 && ws_bytes >= pl.ws_bytes;
  if (pl.ws_required && !ws_ok) return false;
  if (pl.m64_tail && !drn_launch::allow_lds(pl.m64.fn, 156 * 1024)) return false;
  if (pl.lds_cap && !drn_launch::allow_lds(pl.fn, pl.lds_cap)) return false;
  const int HW = p.H * p.W;
  char* cm = (char*)ws;
  const unsigned* rec = (const unsigned*)(cm + roi_st_align((size_t)p.N * HW * p.C * 2));
  const unsigned char* cls = (const unsigned char*)rec + roi_st_align((size_t)p.M * 256);
  const void* cm_fn = nullptr;
  switch (pl.kind) {
    case RK_SPARSE_TABLE:  // its launches in order: prep, then the chunk-major copy, then the pooling
      hipLaunchKernelGGL(roi_st_prep_kernel, dim3((p.M + 3) / 4), dim3(256), 0, st, p, (unsigned*)rec, (unsigned char*)cls);
      cm_fn = pl.vd == 1 ? (const void*)roi_chunk_major_vd_kernel<1> : pl.vd == 2 ? (const void*)roi_chunk_major_vd_kernel<2>
                                                                                  : (const void*)roi_chunk_major_vd_kernel<4>;
      break;
    case RK_WALK:  // from the chunk-major copy where the caller gave the room for it
      if (ws_ok) cm_fn = (const void*)roi_chunk_major_kernel;
      break;
    default: break;
  }
  if (cm_fn) {
    void* cm_args[] = {(void*)&p.feat, (void*)&cm, (void*)&HW, (void*)&p.C};
    (void)hipLaunchKernel(cm_fn, dim3((HW + 31) / 32, (p.C / (pl.vd * 2) + 31) / 32, p.N), dim3(256), cm_args, 0, st);
    p.cm = cm;
  }
  void* args[] = {(void*)&p, (void*)&rec, (void*)&cls};  // (the sparse table's kernel takes all three, the others the first)
  (void)hipLaunchKernel(pl.fn, dim3(pl.grid_x, pl.grid_y), dim3(pl.block), args, pl.smem, st);
  return !pl.m64_tail || roi_map64_launch(pl.m64, p0, st);
}

}  // namespace

// DRN_TUNE_ROI_ST with value 12: print and clear the shader-clock sums the profile builds of roi_pool7_st_kernel accumulated
__attribute__((visibility("hidden"))) int drn_tune_roi_st_profile_dump() {
  unsigned long long h[8];
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(h, HIP_SYMBOL(g_st_prof), sizeof(h)) != hipSuccess) return -1;
  const double n = h[5] ? (double)h[5] : 1.0;
  fprintf(stderr, "roi_st profile: %llu blocks, %.1f ROIs each | shader-clock cycles per block: scan %.0f  slice %.0f  row steps %.0f  column steps %.0f  pooling %.0f\n",
          h[5], (double)h[6] / n, h[0] / n, h[1] / n, h[2] / n, h[3] / n, h[4] / n);
  for (auto& x : h) x = 0;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_st_prof), h, sizeof(h)) != hipSuccess) return -1;
  return 0;
}

extern "C" {

// mode 0 = RoIPool, 1 = ROIAlign. in_dtype = feature dtype, out_dtype = pooled dtype.
int drn_roi_pool_nhwc(const void* feat, const float* rois, const float* objectness, void* out, void* out_t,
                      int32_t* argmax, int N, int H, int W, int C, int P, int M, float spatial_scale, long ld_out,
                      long ld_out_t, int mode, int sampling_ratio, int aligned, int in_dtype, int out_dtype,
                      void* stream) {
  return drn_roi_pool_nhwc_t(feat, rois, objectness, out, out_t, argmax, N, H, W, C, P, M, spatial_scale, ld_out, ld_out_t,
                             mode, sampling_ratio, aligned, in_dtype, out_dtype, 0, stream);
}

// The same with a hint: rows of out_t below channel t_first_channel need not be written (the 64-ROI training kernel then
// skips its A^T store loop for those channel chunks; every other path writes all of out_t).
int drn_roi_pool_nhwc_t(const void* feat, const float* rois, const float* objectness, void* out, void* out_t,
                        int32_t* argmax, int N, int H, int W, int C, int P, int M, float spatial_scale, long ld_out,
                        long ld_out_t, int mode, int sampling_ratio, int aligned, int in_dtype, int out_dtype,
                        int t_first_channel, void* stream) {
  return drn_roi_pool_nhwc_ws(feat, rois, objectness, out, out_t, argmax, N, H, W, C, P, M, spatial_scale, ld_out, ld_out_t, mode,
                              sampling_ratio, aligned, in_dtype, out_dtype, t_first_channel, nullptr, 0, stream);
}

// Bytes of workspace with which drn_roi_pool_nhwc_ws pools this shape faster (0: the shape takes a kernel that needs none): what
// the plan of the best case - no out_t, everything aligned - pools from.
long drn_roi_pool_workspace_bytes(int N, int H, int W, int C, int P, int M, int mode, int has_argmax, int in_dtype, int out_dtype) {
  if (N < 1 || H < 1 || W < 1 || C < 1) return 0;
  const RoiFwdQuery q{N, H, W, C, P, M, mode, in_dtype, out_dtype, has_argmax != 0, false, 0, true, true, true, 0u, 0};
  return (long)roi_fwd_plan(q, g_tune, 256).ws_bytes;  // (ws_bytes does not depend on the CU count: no device call here)
}

// The same with a caller-owned workspace (drn_roi_pool_workspace_bytes; null / too small: as without): maps whose 8-channel slice
// leaves one chunk per block are first copied chunk-major into it, so that the walking kernel stages contiguous runs; the
// sparse-table kernel pools from nothing else.
int drn_roi_pool_nhwc_ws(const void* feat, const float* rois, const float* objectness, void* out, void* out_t,
                         int32_t* argmax, int N, int H, int W, int C, int P, int M, float spatial_scale, long ld_out,
                         long ld_out_t, int mode, int sampling_ratio, int aligned, int in_dtype, int out_dtype,
                         int t_first_channel, void* workspace, long workspace_bytes, void* stream) {
  if (!feat || !rois || !out || P < 1 || P * P > RP_MAXBIN || M < 0 || (mode != 0 && mode != 1)) return DRN_ERR_ARG;
  if (workspace_bytes < 0 || t_first_channel < 0) return DRN_ERR_ARG;
  if (ld_out < (long)C * P * P || (out_t && ld_out_t < M)) return DRN_ERR_ARG;
  if (M == 0) return DRN_OK;
  hipStream_t st = (hipStream_t)stream;
  const int es = drn_esize(out_dtype);
  RoiFwdQuery q{N, H, W, C, P, M, mode, in_dtype, out_dtype, argmax != nullptr, out_t != nullptr, out_t ? t_first_channel : 0,
                (((uintptr_t)feat) & 15) == 0, ((ld_out * es) % 16) == 0 && (((uintptr_t)out) & 15) == 0,
                ((ld_out_t * es) % 16) == 0 && (((uintptr_t)out_t) & 15) == 0, 0u, 0};
  for (;;) {
    const RoiFwdPlan pl = roi_fwd_plan(q, g_tune, drn_launch::cu_count());
    if (pl.kind == RK_NONE) return DRN_ERR_ARG;
    RoiParams p{(const char*)feat, rois, objectness, (char*)out, argmax, N, H, W, C, P, M, spatial_scale, ld_out,
                sampling_ratio, aligned, 0, pl.transpose ? nullptr : (char*)out_t, ld_out_t};
    p.t_c0 = q.t_c0;
    // (a plan that ends in the transpose pass pools without the workspace)
    if (roi_fwd_launch(pl, p, pl.transpose ? nullptr : workspace, (size_t)workspace_bytes, st)) {
      DRN_CHECK_LAUNCH();
      return pl.transpose ? drn_transpose2d(out, out_t, M, C * P * P, ld_out, ld_out_t, out_dtype, out_dtype, stream) : DRN_OK;
    }
    // refused: the next candidate in the plan's order (the 8-ROI kernel: the next entry of its cascade)
    if (pl.kind == RK_MAP8) q.map8_from = pl.cascade + 1;
    else q.skip |= 1u << pl.kind;
  }
}

// d(feat) of drn_roi_pool_nhwc: grad_out [M][ld_g] (k = c*P*P + bin, fp32 or bf16) -> dfeat [N][H][W][C] fp32 (zeroed
// here).  mode 0 needs the arg-max the forward returned; `objectness` as in the forward (fused scaling).
int drn_roi_pool_backward_nhwc(const void* grad_out, const float* rois, const float* objectness, const int32_t* argmax,
                               float* dfeat, int N, int H, int W, int C, int P, int M, float spatial_scale, long ld_g,
                               int mode, int sampling_ratio, int aligned, int grad_dtype, void* stream) {
  if (!grad_out || !rois || !dfeat || P < 1 || P * P > RP_MAXBIN || M < 0 || (mode != 0 && mode != 1)) return DRN_ERR_ARG;
  if ((mode == 0 && !argmax) || ld_g < (long)C * P * P || N < 1 || H < 1 || W < 1 || C < 1) return DRN_ERR_ARG;
  if (grad_dtype != DRN_F32 && grad_dtype != DRN_BF16) return DRN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(dfeat, 0, sizeof(float) * (size_t)N * H * W * C, st) != hipSuccess) return DRN_ERR_LAUNCH;
  if (M == 0) return DRN_OK;
  RoiBwdParams p{(const char*)grad_out, rois, objectness, argmax, dfeat, N, H, W, C, P, M, spatial_scale, ld_g,
                 sampling_ratio, aligned};
  dim3 grid(M, (C + RP_CH - 1) / RP_CH), block(256);
#define RB_LAUNCH(DT, MD) hipLaunchKernelGGL((roi_bwd_kernel<DT, MD>), grid, block, 0, st, p)
  if (grad_dtype == DRN_BF16) { if (mode == 0) RB_LAUNCH(DRN_BF16, 0); else RB_LAUNCH(DRN_BF16, 1); }
  else { if (mode == 0) RB_LAUNCH(DRN_F32, 0); else RB_LAUNCH(DRN_F32, 1); }
#undef RB_LAUNCH
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// The deterministic form of drn_roi_pool_backward_nhwc (see roi_bwd_det_kernel): same arguments plus a caller-owned
// workspace of drn_roi_backward_det_ws_bytes(N, H, W, M) bytes.  No memset, no atomics; two launches.
static inline long roi_det_tiles(int N, int H, int W, int T) { return (long)N * ((H + T - 1) / T) * ((W + T - 1) / T); }

long drn_roi_backward_det_ws_bytes(int N, int H, int W, int M) {
  if (N < 1 || H < 1 || W < 1 || M < 0) return 0;
  return 8L * ((long)M + 1) * roi_det_tiles(N, H, W, 4);
}

int drn_roi_pool_backward_det_nhwc(const void* grad_out, const float* rois, const float* objectness, const int32_t* argmax,
                                   float* dfeat, int N, int H, int W, int C, int P, int M, float spatial_scale, long ld_g,
                                   int mode, int sampling_ratio, int aligned, int grad_dtype, void* ws, long ws_bytes,
                                   void* stream) {
  if (!dfeat || P < 1 || P * P > RP_MAXBIN || M < 0 || (mode != 0 && mode != 1)) return DRN_ERR_ARG;
  if (N < 1 || H < 1 || W < 1 || C < 1 || (M > 0 && (!grad_out || !rois || (mode == 0 && !argmax) || ld_g < (long)C * P * P)))
    return DRN_ERR_ARG;
  if (grad_dtype != DRN_F32 && grad_dtype != DRN_BF16) return DRN_ERR_ARG;
  if (!ws || (((uintptr_t)ws) & 7) != 0 || ws_bytes < drn_roi_backward_det_ws_bytes(N, H, W, M)) return DRN_ERR_ARG;
  const int chunks = (C + RP_CH - 1) / RP_CH;
  // W bounds the exact range of the row-by-multiply in the kernel (8 * W * W < 2^32); the grid's y extent bounds C
  if (W > 16384 || chunks > 65535 || roi_det_tiles(N, H, W, 4) > 0x7fffffffL) return DRN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int T = roi_det_tiles(N, H, W, 8) * chunks < 256 ? 4 : 8;
  RoiDetParams p{(const char*)grad_out, rois, objectness, argmax, dfeat, (int2*)ws, N, H, W, C, P, M, spatial_scale, ld_g,
                 sampling_ratio, aligned, (H + T - 1) / T, (W + T - 1) / T,
                 W > 1 ? roi_wmagic(W) : 0u};
  const dim3 lgrid((unsigned)roi_det_tiles(N, H, W, T)), grid((unsigned)roi_det_tiles(N, H, W, T), chunks), block(64);
#define RD_LIST(MD, TT) hipLaunchKernelGGL((roi_det_list_kernel<MD, TT>), lgrid, block, 0, st, p)
#define RD_ACC(DT, MD, TT) hipLaunchKernelGGL((roi_bwd_det_kernel<DT, MD, TT>), grid, block, 0, st, p)
#define RD_BOTH(MD, TT)                                                  \
  do {                                                                   \
    RD_LIST(MD, TT);                                                     \
    DRN_CHECK_LAUNCH();                                                  \
    if (grad_dtype == DRN_BF16) RD_ACC(DRN_BF16, MD, TT); else RD_ACC(DRN_F32, MD, TT); \
  } while (0)
  if (mode == 0) { if (T == 4) RD_BOTH(0, 4); else RD_BOTH(0, 8); }
  else { if (T == 4) RD_BOTH(1, 4); else RD_BOTH(1, 8); }
#undef RD_BOTH
#undef RD_ACC
#undef RD_LIST
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // extern "C"
