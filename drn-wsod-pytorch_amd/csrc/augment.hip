// The training DatasetMapper's image chain in one launch for gfx950: crop -> Pillow BILINEAR resize -> horizontal flip ->
// brightness blend -> saturation blend, from the decoded 8-bit source image to the fp32 [C][Ho][Wo] planes (the integers 0 .. 255)
// that preprocess_kernel reads.  Built with -ffp-contract=off: the blends are the reference's float32 / float64 operations, op
// for op, and the result is the reference's bytes.
//
// Replaces (host numpy / PIL in the reference): DatasetMapper.__call__ (detectron2/data/dataset_mapper.py:112-185) applying
// CropTransform / HFlipTransform / BlendTransform (fvcore.transforms.transform; published semantics restated),
// ResizeTransform.apply_image (detectron2/data/transforms/transform.py:101-122: PIL.Image.resize(size, BILINEAR)) and the blends of
// RandomBrightness / RandomSaturation (detectron2/data/transforms/augmentation_impl.py:403-455).
//
// Anatomy.  A workgroup of 256 threads owns a tile of TX x TY = 64 x 16 output pixels (before the flip).
//   window  wave 0 reduces the tile's source columns [xlo, xhi), wave 1 its source rows [ylo, yhi) from the tap tables (every
//           table entry is clamped to the crop first, so no table can send an address outside it);
//   stage A the window's bytes go to LDS, row by row, as ALIGNED dwords: consecutive threads load consecutive dwords (a row of the
//           crop starts at an arbitrary byte: x0 * C and W * C are not multiples of 4, so each LDS row keeps its 0 .. 3 lead-in bytes);
//   stage B the horizontal pass, ONCE per source row of the window (the per-pixel kernel of pool.hip repeats it for every vertical
//           tap): thread (row, column) forms the C channels, rounds and clips them to 8 bits exactly as Pillow stores them, and
//           writes them as one packed dword of the LDS byte tile Hs[row][column];
//   stage C the vertical pass over Hs and the blends in registers; a wave stores one 256-byte row segment per channel plane.
// Where a tile's window does not fit the launch's LDS (strong down-scaling) the block takes pixel_path instead: one thread per
// output pixel straight from global memory, the same integer arithmetic, hence the same bits.  The host sizes the LDS from a
// bound on the window (augment_lds_bytes) and launches without LDS staging when the bound exceeds the budget; the kernel
// compares the ACTUAL window with what it was given, so a wrong bound can cost speed, never safety.
// No atomics, no scratch.
#include "drn_common.h"
#include "../../include/drn_wsod.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int TX = 64, TY = 16, NT = 256;
constexpr int PB = 22, HALF = 1 << (PB - 1);
constexpr int HDR = 16;                  // bytes in front of the staging area: the tile's window (4 ints)
constexpr int LDS_BUDGET = 40 * 1024;    // staging bytes a launch may ask for: under the 48-KB default, 3 blocks per CU at the most

struct AugArgs {
  const unsigned char* src;
  int H, W, x0, y0, cw, ch;
  float* dst;
  int Ho, Wo;
  const int *xb, *xk, *yb, *yk;
  int ksx, ksy;
  int flip, bright, sat;
  float wb, ws;
  double oms;
  int cap;  // staging bytes behind the header
};

// taps of output position i: source positions [lo, lo + n) of an axis of n_in positions.  No table: the identity.  Table values are
// clamped into the axis (Pillow's own tables already are), so every address formed from them stays inside the crop.
__device__ __forceinline__ void tap_window(const int* __restrict__ b, int i, int n_in, int ks, int& lo, int& n) {
  if (!b) {
    lo = i;  // (no pass: the size is unchanged, i < n_in)
    n = 1;
    return;
  }
  lo = min(max(b[2 * i], 0), n_in - 1);
  n = min(max(b[2 * i + 1], 0), min(ks, n_in - lo));
}

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

// BlendTransform twice (brightness: float32; saturation: float64 with the grey value summed in a fixed order), the flip, the store
template <int C>
__device__ __forceinline__ void blend_store(const AugArgs& a, const int (&r)[C], int yy, int xx) {
  int v[C];
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = r[c];
  if (a.bright) {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = (int)fminf(fmaxf(a.wb * (float)v[c], 0.f), 255.f);
  }
  if constexpr (C == 3) {
    if (a.sat) {
      const double g = ((double)v[0] * 0.299 + (double)v[1] * 0.587) + (double)v[2] * 0.114;
      const double sg = a.oms * g;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double t = sg + (double)(a.ws * (float)v[c]);
        v[c] = (int)fmin(fmax(t, 0.0), 255.0);
      }
    }
  }
  const int xo = a.flip ? a.Wo - 1 - xx : xx;
#pragma unroll
  for (int c = 0; c < C; ++c) a.dst[((long)c * a.Ho + yy) * a.Wo + xo] = (float)v[c];
}

// one thread = one output pixel of the tile, straight from global memory (byte loads inside the crop)
template <int C>
__device__ void pixel_path(const AugArgs& a, int tx0, int ty0, int tw, int th) {
  for (int i = threadIdx.x; i < TX * TY; i += NT) {
    const int lx = i % TX, ly = i / TX;
    if (lx >= tw || ly >= th) continue;
    const int xx = tx0 + lx, yy = ty0 + ly;
    int xmin, xn, ymin, yn;
    tap_window(a.xb, xx, a.cw, a.ksx, xmin, xn);
    tap_window(a.yb, yy, a.ch, a.ksy, ymin, yn);
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = HALF;
    for (int y = 0; y < yn; ++y) {
      const unsigned char* row = a.src + ((long)(a.y0 + ymin + y) * a.W + a.x0 + xmin) * C;
      int h[C];
      if (a.xb) {
        int s[C];
#pragma unroll
        for (int c = 0; c < C; ++c) s[c] = HALF;
        for (int x = 0; x < xn; ++x) {
          const int k = a.xk[(long)xx * a.ksx + x];
#pragma unroll
          for (int c = 0; c < C; ++c) s[c] += (int)row[x * C + c] * k;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) h[c] = clip8(s[c] >> PB);
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) h[c] = row[c];
      }
      if (a.yb) {
        const int k = a.yk[(long)yy * a.ksy + y];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += h[c] * k;
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = h[c];
      }
    }
    int r[C];
#pragma unroll
    for (int c = 0; c < C; ++c) r[c] = a.yb ? clip8(acc[c] >> PB) : acc[c];
    blend_store<C>(a, r, yy, xx);
  }
}

template <int C>
__global__ __launch_bounds__(NT) void augment_u8_kernel(AugArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* hdr = (int*)smem;
  const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * TY;
  const int tw = min(TX, a.Wo - tx0), th = min(TY, a.Ho - ty0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  if (wave < 2) {  // wave 0: columns, wave 1: rows
    int lo = INT_MAX, hi = 0;
    if (lane < (wave ? th : tw)) {
      int n;
      if (wave) tap_window(a.yb, ty0 + lane, a.ch, a.ksy, lo, n);
      else tap_window(a.xb, tx0 + lane, a.cw, a.ksx, lo, n);
      hi = lo + n;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o, 64));
      hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) {
      hdr[2 * wave] = lo;
      hdr[2 * wave + 1] = max(hi, lo);
    }
  }
  __syncthreads();
  const int xlo = hdr[0], ylo = hdr[2];
  const int ncols = hdr[1] - xlo, nrows = hdr[3] - ylo;
  const int span = ncols * C;        // bytes of one source row that the tile reads
  const int srow = (span + 6) >> 2;  // dwords of an LDS row: up to 3 lead-in bytes + span, rounded up
  if ((long)nrows * (srow + TX) * 4 > (long)a.cap) {  // (the same for the whole block)
    pixel_path<C>(a, tx0, ty0, tw, th);
    return;
  }
  unsigned int* S = (unsigned int*)(smem + HDR);
  unsigned int* Hs = S + nrows * srow;

  // Stage A.  Bound: the bytes the tile needs of source row r are [first, first + span); they lie inside the crop (tap_window), hence
  // inside [src, src + H*W*C).  Only dwords that hold at least one of those bytes are touched, and a dword that reaches across
  // either end of the buffer - the lead-in in front of an unaligned src, the partial last dword behind a crop flush with the
  // bottom-right corner - is assembled from byte loads of its bytes inside the buffer.
  const uintptr_t buf_lo = (uintptr_t)a.src, buf_hi = buf_lo + (size_t)a.H * a.W * C;
  for (int i = tid; i < nrows * srow; i += NT) {
    const int r = i / srow, j = i - r * srow;
    const uintptr_t first = buf_lo + ((size_t)(a.y0 + ylo + r) * a.W + a.x0 + xlo) * C;
    const uintptr_t p = (first & ~(uintptr_t)3) + 4 * (uintptr_t)j;
    if (p >= first + span) continue;
    unsigned int v = 0;
    if (p >= buf_lo && p + 4 <= buf_hi) {
      v = *(const unsigned int*)p;
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (p + b >= buf_lo && p + b < buf_hi) v |= (unsigned int)(*(const unsigned char*)(p + b)) << (8 * b);
    }
    S[i] = v;
  }
  __syncthreads();

  // Stage B: TX == the wave size, so a thread keeps its column and walks the window's rows
  if (lane < tw) {
    const unsigned char* Sb = (const unsigned char*)S;
    int xmin, xn;
    tap_window(a.xb, tx0 + lane, a.cw, a.ksx, xmin, xn);
    const int* kx = a.xb ? a.xk + (long)(tx0 + lane) * a.ksx : nullptr;
    for (int r = wave; r < nrows; r += NT / 64) {
      const int lead = (int)((buf_lo + ((size_t)(a.y0 + ylo + r) * a.W + a.x0 + xlo) * C) & 3);
      const unsigned char* row = Sb + (long)r * srow * 4 + lead + (xmin - xlo) * C;
      unsigned int pk = 0;
      if (a.xb) {
        int s[C];
#pragma unroll
        for (int c = 0; c < C; ++c) s[c] = HALF;
        for (int x = 0; x < xn; ++x) {
          const int k = kx[x];
#pragma unroll
          for (int c = 0; c < C; ++c) s[c] += (int)row[x * C + c] * k;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) pk |= (unsigned int)clip8(s[c] >> PB) << (8 * c);
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) pk |= (unsigned int)row[c] << (8 * c);
      }
      Hs[r * TX + lane] = pk;
    }
  }
  __syncthreads();

  // Stage C
  if (lane < tw) {
    for (int ly = wave; ly < th; ly += NT / 64) {
      const int yy = ty0 + ly;
      int ymin, yn;
      tap_window(a.yb, yy, a.ch, a.ksy, ymin, yn);
      int r[C];
      if (a.yb) {
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = HALF;
        const int* ky = a.yk + (long)yy * a.ksy;
        for (int y = 0; y < yn; ++y) {
          const unsigned int pk = Hs[(ymin - ylo + y) * TX + lane];
          const int k = ky[y];
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] += (int)((pk >> (8 * c)) & 255u) * k;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) r[c] = clip8(acc[c] >> PB);
      } else {
        const unsigned int pk = Hs[(ymin - ylo) * TX + lane];
#pragma unroll
        for (int c = 0; c < C; ++c) r[c] = (int)((pk >> (8 * c)) & 255u);
      }
      blend_store<C>(a, r, yy, tx0 + lane);
    }
  }
}

// source positions a tile of `tile` output positions can read: (tile - 1) * scale between the first and the last centre, the
// filter's support on either side, and the roundings
long window_bound(int n_in, int n_out, int tile, int pass) {
  if (!pass) return tile < n_in ? tile : n_in;
  const double scale = (double)n_in / n_out, support = scale > 1.0 ? scale : 1.0;
  const long n = (long)ceil(tile * scale + 2.0 * support) + 2;
  return n < n_in ? n : n_in;
}

long augment_lds_bytes(int cw, int ch, int Ho, int Wo, int C, int xpass, int ypass) {
  const long ncols = window_bound(cw, Wo, TX, xpass), nrows = window_bound(ch, Ho, TY, ypass);
  const long srow = (ncols * C + 6) >> 2;
  const long need = nrows * (srow + TX) * 4;
  return need <= LDS_BUDGET ? need : 0;
}

template <int C>
int launch(const AugArgs& a, hipStream_t st) {
  const dim3 grid((a.Wo + TX - 1) / TX, (a.Ho + TY - 1) / TY);
  hipLaunchKernelGGL(augment_u8_kernel<C>, grid, dim3(NT), (size_t)(HDR + a.cap), st, a);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // namespace

extern "C" {

long drn_augment_lds_bytes(int cw, int ch, int Ho, int Wo, int C, int xpass, int ypass) {
  if (cw <= 0 || ch <= 0 || Ho <= 0 || Wo <= 0 || C < 1 || C > 4) return DRN_ERR_ARG;
  return augment_lds_bytes(cw, ch, Ho, Wo, C, xpass, ypass);
}

int drn_augment_u8(const void* src_hwc, int H, int W, int C, int x0, int y0, int cw, int ch, float* dst_chw, int Ho, int Wo,
                   const int* xbounds, const int* xcoef, int ksx, const int* ybounds, const int* ycoef, int ksy, int flip,
                   int brightness_on, float wb, int saturation_on, double one_minus_ws, float ws, void* stream) {
  if (!src_hwc || !dst_chw || H <= 0 || W <= 0 || (C != 1 && C != 3 && C != 4) || Ho <= 0 || Wo <= 0) return DRN_ERR_ARG;
  if (x0 < 0 || y0 < 0 || cw <= 0 || ch <= 0 || (long)x0 + cw > W || (long)y0 + ch > H) return DRN_ERR_ARG;  // crop inside the image
  if ((xbounds && (!xcoef || ksx < 1)) || (ybounds && (!ycoef || ksy < 1))) return DRN_ERR_ARG;
  if ((!xbounds && Wo != cw) || (!ybounds && Ho != ch)) return DRN_ERR_ARG;  // no pass in a direction: the size stays
  if (saturation_on && C != 3) return DRN_ERR_ARG;  // "RandomSaturation only works on RGB images"
  if ((Ho + TY - 1) / TY > 65535) return DRN_ERR_UNSUPPORTED;
  AugArgs a;
  a.src = (const unsigned char*)src_hwc;
  a.H = H, a.W = W, a.x0 = x0, a.y0 = y0, a.cw = cw, a.ch = ch;
  a.dst = dst_chw;
  a.Ho = Ho, a.Wo = Wo;
  a.xb = xbounds, a.xk = xcoef, a.yb = ybounds, a.yk = ycoef;
  a.ksx = ksx, a.ksy = ksy;
  a.flip = flip != 0, a.bright = brightness_on != 0, a.sat = saturation_on != 0;
  a.wb = wb, a.ws = ws, a.oms = one_minus_ws;
  a.cap = (int)((augment_lds_bytes(cw, ch, Ho, Wo, C, xbounds != nullptr, ybounds != nullptr) + 15) & ~15L);
  hipStream_t st = (hipStream_t)stream;
  if (C == 1) return launch<1>(a, st);
  if (C == 3) return launch<3>(a, st);
  return launch<4>(a, st);
}

}  // extern "C"
