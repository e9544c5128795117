// Stand-alone NMS for gfx950: torchvision nms and detectron2's batched_nms (detectron2/layers/nms.py:10-29) over ALL candidates,
// bit-exact against the oracle's restatement (oracle/roi_ops.c:223-268; built with -ffp-contract=off).
//
// detect.hip's nms_topk_wave is one wave that walks the sorted list against the <= 1024 boxes kept so far: right for "top 100 of
// 40 000", O(n * kept) on one CU when most candidates survive.  Here the pairwise work is spread over the device:
//   order     the package's stable radix passes (radix_sort.h): descending score, equal scores in input order
//   prep      the boxes gathered into sorted order (class offset added below 40 000 candidates), the removed-bitmap started
//   per panel of PANEL = 512 sorted rows, two launches:
//     mask    64 x 64 IoU tiles, one wave per tile: word (row, cb) has bit j set iff row suppresses column 64 cb + j (a later row,
//             IoU > thr, same class in per-class mode).  Rows and columns that earlier panels removed are skipped.
//     scan    every workgroup resolves the panel's own 512 x 512 corner in order (one wave, 8 words of removed-bits in registers,
//             the corner staged in LDS) - the same answer in each - then ORs the words of the KEPT rows into its slice of the
//             removed-bitmap beyond the panel; workgroup 0 appends the kept rows to the output.
// Greedy NMS is order-causal, so resolving panel after panel gives the serial result.  Nothing is read by the host, no float
// atomics; the launch count depends on the capacity alone.
#include "nms_shared.h"
#include "radix_sort.h"

namespace drn_supp {
namespace {

constexpr int PW = PANEL / 64;  // 64-bit words of one panel's rows
constexpr int CG = 8;           // column blocks per mask workgroup: a row's 8 words leave as one 64-byte line
static_assert(PW == CG, "a panel starts on a column-group boundary");

inline int stride_words(long cap) { return (int)(((cap + 63) / 64 + CG - 1) / CG * CG); }
inline long up64(long v) { return (v + 63) / 64 * 64; }

struct Carve {
  float4* sb; int* scls; unsigned long long* removed; unsigned long long* panel; int stride;
};
inline Carve carve(void* ws, long cap) {
  Carve c;
  char* w = (char*)ws;
  const long rows = up64(cap < 1 ? 1 : cap);
  c.stride = stride_words(cap < 1 ? 1 : cap);
  c.sb = (float4*)w; w += rows * 16;
  c.scls = (int*)w; w += rows * 4;
  c.removed = (unsigned long long*)w; w += up64((long)c.stride * 8);
  c.panel = (unsigned long long*)w;
  return c;
}

struct SupParams {
  const float* boxes; const int* cls; const int* order; const int* count;
  const float* maxcoord_f; const unsigned* maxcoord_key;
  int per_class_from; float thr; int limit;
  float4* sb; int* scls; unsigned long long* removed; unsigned long long* panel; int stride;
  int* keep32; long long* keep64; int* n_keep;
};

__device__ __forceinline__ float key_to_float(unsigned asc) {
  return __builtin_bit_cast(float, (asc >> 31) ? asc ^ 0x80000000u : ~asc);
}
__device__ __forceinline__ unsigned float_to_key(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// sorted position i <- candidate order[i]: its box (idxs.to(boxes) * (boxes.max() + 1) added below the per-class switch) and
// class; removed-bitmap: clear for the n live positions, set beyond them; n_keep = 0
__global__ __launch_bounds__(256) void nms_prep_kernel(SupParams p) {
  const int n = p.count[0];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) p.n_keep[0] = 0;
  if (i < p.stride) {
    const long live = (long)n - 64L * i;
    p.removed[i] = live >= 64 ? 0ULL : live <= 0 ? ~0ULL : ~0ULL << live;
  }
  if (i >= n) return;
  const int id = p.order[i];
  float x1 = p.boxes[4 * (long)id], y1 = p.boxes[4 * (long)id + 1], x2 = p.boxes[4 * (long)id + 2], y2 = p.boxes[4 * (long)id + 3];
  int c = 0;
  if (p.cls) {
    c = p.cls[id];
    if (n < p.per_class_from) {
      const float mx = p.maxcoord_f ? p.maxcoord_f[0] : key_to_float(p.maxcoord_key[0]);
      const float off = (float)c * (mx + 1.f);
      x1 = x1 + off; y1 = y1 + off; x2 = x2 + off; y2 = y2 + off;
    }
  }
  p.sb[i] = make_float4(x1, y1, x2, y2);
  p.scls[i] = c;
}

// grid (column groups from the panel's own to the last, 8 row tiles); wave w of a workgroup takes column blocks w and w + 4 of the
// group against the tile's 64 rows (lane = row)
__global__ __launch_bounds__(256) void nms_mask_kernel(SupParams p, int r0) {
  __shared__ float4 cbox[CG * 64];
  __shared__ float carea[CG * 64];
  __shared__ int ccls[CG * 64];
  __shared__ unsigned long long wds[64][CG];
  const int n = p.count[0];
  if (r0 >= n || p.n_keep[0] >= p.limit) return;
  const int pb = r0 >> 6, cb0 = pb + (int)blockIdx.x * CG, rt = blockIdx.y, rb = pb + rt;
  if ((long)cb0 * 64 >= n || (long)rb * 64 >= n) return;  // (block-uniform: nobody waits at a barrier)
  const bool per_class = p.cls != nullptr && n >= p.per_class_from;
  for (int t = threadIdx.x; t < CG * 64; t += 256) {
    const long col = (long)cb0 * 64 + t;
    const float4 b = col < n ? p.sb[col] : make_float4(0.f, 0.f, 0.f, 0.f);
    cbox[t] = b;
    carea[t] = (b.z - b.x) * (b.w - b.y);
    ccls[t] = col < n ? p.scls[col] : -1;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long row = (long)rb * 64 + lane;
  const bool rlive = row < n && !((p.removed[rb] >> lane) & 1ULL);  // rows removed by earlier panels contribute nothing
  const float4 r = rlive ? p.sb[row] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float rarea = (r.z - r.x) * (r.w - r.y);
  const int rcls = rlive ? p.scls[row] : -1;
  const float thr = p.thr;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int g = w + 4 * q, cb = cb0 + g;
    unsigned long long word = 0;
    if (cb >= rb && (long)cb * 64 < n && rlive) {
      const unsigned long long colrem = p.removed[cb];
      const long left = (long)n - (long)cb * 64;
      const int ncol = left < 64 ? (int)left : 64;
      for (int j = 0; j < ncol; ++j) {
        if ((colrem >> j) & 1ULL) continue;  // (wave-uniform)
        if (cb == rb && j <= lane) continue; // only later rows are suppressed
        if (per_class && ccls[g * 64 + j] != rcls) continue;
        const float4 c = cbox[g * 64 + j];
        const float iw = fmaxf(0.f, fminf(r.z, c.z) - fmaxf(r.x, c.x));
        const float ih = fmaxf(0.f, fminf(r.w, c.w) - fmaxf(r.y, c.y));
        const float inter = iw * ih;
        // inter <= 0 gives a ratio of +-0 or NaN: never > a threshold >= 0, so the division is skipped there
        if ((inter > 0.f || thr < 0.f) && inter / (rarea + carea[g * 64 + j] - inter) > thr) word |= 1ULL << j;
      }
    }
    wds[lane][g] = word;
  }
  __syncthreads();
  const int rl = threadIdx.x >> 2, h = threadIdx.x & 3;
  unsigned long long* dst = p.panel + (long)(rt * 64 + rl) * p.stride + cb0 + 2 * h;
  *(ulonglong2*)dst = make_ulonglong2(wds[rl][2 * h], wds[rl][2 * h + 1]);
}

// lane l's 64-bit value, for a wave-uniform l
__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// grid: one workgroup per 64 words of the removed-bitmap beyond the panel (at least one)
__global__ __launch_bounds__(256) void nms_scan_kernel(SupParams p, int r0) {
  __shared__ unsigned long long diag[PANEL][PW + 1];  // (one word of padding: a lane per row reads without bank conflicts)
  __shared__ unsigned long long keptw[PW];
  __shared__ unsigned long long part[4][64];
  const int n = p.count[0];
  if (r0 >= n) return;
  // Workgroup 0 raises n_keep when it is done, so a workgroup that starts later may see the new value: one thread reads it for the
  // whole workgroup (all leave or none), and the workgroup leaves only when the limit is reached - after which no later launch
  // reads the bitmap.
  __shared__ int sbase;
  if (threadIdx.x == 0) sbase = p.n_keep[0];
  __syncthreads();
  const int base = sbase;
  if (base >= p.limit) return;
  const int pb = r0 >> 6, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int rows = n - r0 < PANEL ? n - r0 : PANEL;
  for (int t = threadIdx.x; t < rows * PW; t += 256) diag[t / PW][t % PW] = p.panel[(long)(t / PW) * p.stride + pb + t % PW];
  __syncthreads();
  if (w == 0) {
    // Lane q < PW holds word q of the panel's removed-bits.  The panel is resolved 64 rows (one word) at a time, lane = row: the
    // rows' own 64 x 64 corner decides who is kept - a scalar loop over the rows still alive, each one clearing what its diagonal
    // word suppresses (wave-uniform 64-bit operations, one v_readlane pair per kept row) - and the kept rows' words for the later
    // chunks are OR-reduced across the wave into the lanes that hold them.
    unsigned long long rem = lane < PW ? p.removed[pb + lane] : 0ULL;
    const int nchunk = (rows + 63) >> 6;
#pragma unroll
    for (int c = 0; c < PW; ++c) {
      if (c >= nchunk) {  // (positions beyond n were set in the bitmap from the start: nothing is kept there)
        if (lane == 0) keptw[c] = 0ULL;
        continue;
      }
      const int r = c * 64 + lane;
      unsigned long long mw[PW];
#pragma unroll
      for (int q = c; q < PW; ++q) mw[q] = r < rows ? diag[r][q] : 0ULL;
      unsigned long long alive = ~readlane64(rem, c), pending = alive;
      while (pending) {
        const int i = __ffsll((long long)pending) - 1;  // row i is kept: what it suppresses is removed
        alive &= ~readlane64(mw[c], i);
        pending = alive & ((~0ULL << i) << 1);
      }
      if (lane == 0) keptw[c] = alive;
      const bool mine = (alive >> lane) & 1ULL;
#pragma unroll
      for (int q = c + 1; q < PW; ++q) {
        unsigned long long v = mine ? mw[q] : 0ULL;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
        if (lane == q) rem |= v;
      }
    }
  }
  __syncthreads();
  const int nblk = (n + 63) >> 6;
  const int c = pb + PW + (int)blockIdx.x * 64 + lane;
  unsigned long long acc = 0;
  if (c < nblk)
    for (int wi = 2 * w; wi < 2 * w + 2; ++wi) {
      unsigned long long k = keptw[wi];
      while (k) {
        const int b = __ffsll((long long)k) - 1;
        k &= k - 1;
        acc |= p.panel[(long)(wi * 64 + b) * p.stride + c];
      }
    }
  part[w][lane] = acc;
  __syncthreads();
  if (w == 0 && c < nblk) p.removed[c] |= part[0][lane] | part[1][lane] | part[2][lane] | part[3][lane];
  if (blockIdx.x == 0 && w == 0) {
    int pos = base;
    for (int wi = 0; wi < PW; ++wi) {
      const unsigned long long k = keptw[wi];
      if ((k >> lane) & 1ULL) {
        const int o = pos + __popcll(k & ((1ULL << lane) - 1ULL));
        if (o < p.limit) {
          const int id = p.order[r0 + wi * 64 + lane];
          if (p.keep32) p.keep32[o] = id; else p.keep64[o] = id;
        }
      }
      pos += __popcll(k);
    }
    if (lane == 0) p.n_keep[0] = pos < p.limit ? pos : p.limit;
  }
}

// ---- the front of drn_nms / drn_batched_nms: count and the largest coordinate on the device --------------------------------
__global__ void nms_init_kernel(int* count, unsigned* maxkey, int n) {
  if (threadIdx.x == 0) { count[0] = n; maxkey[0] = 0u; }
}

// boxes.max(): an integer max on order-preserving keys (exact whatever the order the workgroups arrive in)
__global__ __launch_bounds__(256) void nms_maxcoord_kernel(const float* __restrict__ boxes, long total, unsigned* maxkey) {
  unsigned k = 0u;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256L) {
    const unsigned v = float_to_key(boxes[i]);
    k = v > k ? v : k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned u = (unsigned)__shfl_xor((int)k, o, 64);
    k = u > k ? u : k;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(maxkey, k);
}

__global__ void nms_zero_kernel(int* n_keep) {
  if (threadIdx.x == 0) n_keep[0] = 0;
}

struct Front { unsigned* key0; unsigned* key1; int* val0; int* order; int* hist; int* count; unsigned* maxkey; char* rest; };
inline int sort_tiles(long n) { return (int)((n + SORT_TILE - 1) / SORT_TILE); }
inline Front carve_front(void* ws, long n) {
  Front f;
  char* w = (char*)ws;
  const long rows = up64(n);
  f.count = (int*)w; f.maxkey = (unsigned*)(w + 8); w += 256;
  f.key0 = (unsigned*)w; w += rows * 4;
  f.key1 = (unsigned*)w; w += rows * 4;
  f.val0 = (int*)w; w += rows * 4;
  f.order = (int*)w; w += rows * 4;
  f.hist = (int*)w; w += (long)SORT_BINS * sort_tiles(n) * 4;
  f.rest = w;
  return f;
}
// 256 + 16 (n + 63) + 8192 (n / 4096 + 1) + suppress_ws_bytes(n) <= 104 n + 65536
inline long nms_ws_bytes(long n) { return 104L * (n < 0 ? 0 : n) + 65536L; }

int nms_entry(const float* boxes, const float* scores, const int* idxs, long n, float thr, void* workspace, long ws_bytes,
              long long* keep, int* n_keep, void* stream) {
  if (n < 0 || !n_keep) return DRN_ERR_ARG;
  if (n > MAX_N) return DRN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    hipLaunchKernelGGL(nms_zero_kernel, dim3(1), dim3(64), 0, st, n_keep);
    DRN_CHECK_LAUNCH();
    return DRN_OK;
  }
  if (!boxes || !scores || !keep || !workspace || ((uintptr_t)workspace & 15) || ws_bytes < nms_ws_bytes(n)) return DRN_ERR_ARG;
  Front f = carve_front(workspace, n);
  hipLaunchKernelGGL(nms_init_kernel, dim3(1), dim3(64), 0, st, f.count, f.maxkey, (int)n);
  if (idxs && n < 40000) {
    const long blocks = (4 * n + 255) / 256;
    hipLaunchKernelGGL(nms_maxcoord_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, boxes, 4 * n,
                       f.maxkey);
  }
  // stable descending order: (score, index) -> key1/order -> key0/val0 -> key1/order
  const int tiles = sort_tiles(n);
  const int shifts[3] = {0, 11, 22}, bits[3] = {11, 11, 10};
  for (int ps = 0; ps < 3; ++ps) {
    const bool even = (ps & 1) == 0;
    SortPass sp{scores, even ? f.key0 : f.key1, even ? f.val0 : f.order, even ? f.key1 : f.key0,
                even ? f.order : f.val0, f.hist, f.count, tiles, shifts[ps], bits[ps], ps == 0};
    hipLaunchKernelGGL(sort_hist_kernel, dim3(tiles), dim3(SORT_THREADS), 0, st, sp);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 0, st, sp);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(tiles), dim3(SORT_THREADS), 0, st, sp);
  }
  SuppressIn in{boxes, idxs, f.order, f.count, nullptr, f.maxkey, 40000, thr, 0x7fffffff};
  launch_suppress(in, (int)n, f.rest, nullptr, keep, n_keep, st);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // namespace

long suppress_ws_bytes(long cap) { return 88L * (cap < 1 ? 1 : cap) + 49152L; }

void launch_suppress(const SuppressIn& in, int cap, void* ws, int* keep32, long long* keep64, int* n_keep, hipStream_t st) {
  const Carve c = carve(ws, cap);
  SupParams p{in.boxes, in.cls, in.order, in.count, in.maxcoord_f, in.maxcoord_key, in.per_class_from, in.thr, in.limit,
              c.sb, c.scls, c.removed, c.panel, c.stride, keep32, keep64, n_keep};
  const int prep = cap > c.stride ? cap : c.stride;
  hipLaunchKernelGGL(nms_prep_kernel, dim3((prep + 255) / 256), dim3(256), 0, st, p);
  for (int r0 = 0; r0 < cap; r0 += PANEL) {
    const int pb = r0 >> 6;
    hipLaunchKernelGGL(nms_mask_kernel, dim3((c.stride - pb) / CG, PW), dim3(256), 0, st, p, r0);
    const int beyond = c.stride - pb - PW;
    hipLaunchKernelGGL(nms_scan_kernel, dim3(beyond > 0 ? (beyond + 63) / 64 : 1), dim3(256), 0, st, p, r0);
  }
}

}  // namespace drn_supp

extern "C" {

long drn_nms_workspace_bytes(long n) { return drn_supp::nms_ws_bytes(n); }

int drn_nms(const float* boxes, const float* scores, long n, float iou_thr, void* workspace, long workspace_bytes,
            long long* keep, int* n_keep, void* stream) {
  return drn_supp::nms_entry(boxes, scores, nullptr, n, iou_thr, workspace, workspace_bytes, keep, n_keep, stream);
}

int drn_batched_nms(const float* boxes, const float* scores, const int* idxs, long n, float iou_thr, void* workspace,
                    long workspace_bytes, long long* keep, int* n_keep, void* stream) {
  if (n > 0 && !idxs) return DRN_ERR_ARG;
  return drn_supp::nms_entry(boxes, scores, idxs, n, iou_thr, workspace, workspace_bytes, keep, n_keep, stream);
}

}  // extern "C"
