// Inference tail for gfx950: score threshold + compaction in row-major (nonzero) order, stable
// descending sort, class-offset greedy NMS with early exit at top-k.  Indices must be bit-exact
// vs the CPU path, so every float op follows the oracle's order (built with -ffp-contract=off).
//
// Replaces fast_rcnn_inference_single_image (projects/WSL/wsl/modeling/roi_heads/fast_rcnn.py:88-141)
// and batched_nms (detectron2/layers/nms.py:10-29 over torchvision nms / batched_nms).
//
// Design: the reference sorts and suppresses ALL candidates (up to R*K = 40k-320k) and then keeps
// keep[:100].  Greedy NMS is order-causal: whether candidate i survives depends only on survivors
// before it, so we walk the sorted list 64 candidates (one wave) at a time against the <= topk
// survivors held in LDS and stop as soon as topk are kept - identical output, O(n*topk) work.
#include "drn_common.h"
#include "nms_shared.h"
#include "radix_sort.h"

namespace {

// TransformList([ResizeTransform, HFlipTransform?]).inverse().apply_box on one box, in float32 op for op like the numpy code the
// reference runs on the host: HFlipTransform.inverse (x -> W' - x, flip_w < 0 = not flipped), ResizeTransform.inverse (x * sx,
// y * sy) on the four corners, then their bounding box.  Shared by the AVG accumulation and the UNION candidates.
__device__ __forceinline__ void tta_inverse_box(const float* __restrict__ b, float sx, float sy, float flip_w, float o[4]) {
  float x0 = b[0], y0 = b[1], x1 = b[2], y1 = b[3];
  if (flip_w >= 0.f) { x0 = flip_w - x0; x1 = flip_w - x1; }
  x0 = x0 * sx; x1 = x1 * sx; y0 = y0 * sy; y1 = y1 * sy;
  o[0] = fminf(x0, x1); o[1] = fminf(y0, y1); o[2] = fmaxf(x0, x1); o[3] = fmaxf(y0, y1);
}

struct CandParams {
  const float* boxes;   // [R][4*nreg]
  const float* scores;  // [R][K+1]
  int R, K, nreg;
  float img_h, img_w, thresh;
  float* c_box;   // [cap][4] clipped boxes
  float* c_score; // [cap]
  int* c_row; int* c_cls;  // [cap]
  int* count;     // [1]
  float* maxcoord;  // [1] max over candidate box coordinates
  int cap;
  int* rowmap;    // [R] scratch: index of row r among the finite rows, or -1
};

// finite-row filter (fast_rcnn.py:108-111), one wave per row over many blocks: rowmap[r] = 0 (all K+1 scores and 4*nreg box
// coordinates finite) or -1.  Inside the single-block kernel below this was 101 loads per thread, each waiting for the previous one's
// verdict (`&& finite`), from ONE CU: ~120 of that kernel's 150 us (profiles/r5_63_infer480_kernel_stats.txt).
__global__ __launch_bounds__(256) void rows_finite_kernel(CandParams p) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= p.R) return;
  const float* srow = p.scores + (long)r * (p.K + 1);
  const float* brow = p.boxes + (long)r * 4 * p.nreg;
  bool finite = true;
  for (int k = lane; k <= p.K; k += 64) finite = finite && isfinite(srow[k]);
  for (int k = lane; k < 4 * p.nreg; k += 64) finite = finite && isfinite(brow[k]);
  const bool all = __ballot(!finite) == 0;
  if (lane == 0) p.rowmap[r] = all ? 0 : -1;
}

// single block: the rows that passed rows_finite_kernel, numbered in order - rows with any non-finite box or score are dropped BEFORE
// indexing (fast_rcnn.py:108-111), so every later row index refers to the compacted arrays
__global__ __launch_bounds__(1024) void rows_number_kernel(CandParams p) {
  __shared__ int wcnt[16];
  __shared__ int base;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) {
    base = 0;
    p.maxcoord[0] = -INFINITY;
  }
  __syncthreads();
  for (int start = 0; start < p.R; start += 1024) {
    const int r = start + threadIdx.x;
    const bool finite = r < p.R && p.rowmap[r] >= 0;
    const unsigned long long bal = __ballot(finite);
    const int wprefix = __popcll(bal & ((1ULL << lane) - 1ULL));
    if (lane == 0) wcnt[w] = __popcll(bal);
    __syncthreads();
    int woff = 0, tot = 0;
    for (int q = 0; q < 16; ++q) { if (q < w) woff += wcnt[q]; tot += wcnt[q]; }
    if (r < p.R) p.rowmap[r] = finite ? base + woff + wprefix : -1;
    __syncthreads();
    if (threadIdx.x == 0) base += tot;
    __syncthreads();
  }
}

// threshold + ordered compaction of the R x K scores (row-major = nonzero order) over many blocks: a tile of CAND_TILE consecutive
// entries per block, a thread takes CAND_EPT CONSECUTIVE entries (entry order = thread order = output order).  Pass 0 leaves
// every tile's count, pass 1 places a tile behind the sum of the counts in front of it - the output is a function of the input
// alone, as in the single-block form this replaces (150 us per image from one CU: 40 000 entries, 280 000 scattered 4-byte stores;
// profiles/r5_63_infer480_kernel_stats.txt).  The largest candidate coordinate is an atomic max on the bits of non-negative
// floats (the boxes are clipped to the image first): exact whatever the order.
constexpr int CAND_THREADS = 256, CAND_EPT = 8, CAND_TILE = CAND_THREADS * CAND_EPT;
template <int PASS>
__global__ __launch_bounds__(CAND_THREADS) void candidates_kernel(CandParams p, int* tile_cnt, int ntiles) {
  __shared__ int wcnt[CAND_THREADS / 64];
  __shared__ int sbase;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long total = (long)p.R * p.K;
  const long i0 = (long)blockIdx.x * CAND_TILE + (long)threadIdx.x * CAND_EPT;
  unsigned flags = 0;
  float sv[CAND_EPT];
  int n_mine = 0;
#pragma unroll
  for (int e = 0; e < CAND_EPT; ++e) {
    const long i = i0 + e;
    sv[e] = 0.f;
    if (i < total) {
      const int r = (int)(i / p.K), c = (int)(i - (long)r * p.K);
      sv[e] = p.scores[(long)r * (p.K + 1) + c];
      if (p.rowmap[r] >= 0 && sv[e] > p.thresh) flags |= 1u << e, ++n_mine;
    }
  }
  // inclusive prefix of n_mine over the wave's lanes, then over the block's waves
  int incl = n_mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wcnt[w] = incl;
  if (PASS == 1 && threadIdx.x == 0) {
    int b = 0;
    for (int t = 0; t < (int)blockIdx.x; ++t) b += tile_cnt[t];
    sbase = b;
  }
  __syncthreads();
  int woff = 0, tot = 0;
  for (int q = 0; q < CAND_THREADS / 64; ++q) { if (q < w) woff += wcnt[q]; tot += wcnt[q]; }
  if (PASS == 0) {
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
    return;
  }
  int pos = sbase + woff + incl - n_mine;
  float mymax = -INFINITY;
#pragma unroll
  for (int e = 0; e < CAND_EPT; ++e)
    if (flags >> e & 1) {
      if (pos < p.cap) {
        const long i = i0 + e;
        const int r = (int)(i / p.K), c = (int)(i - (long)r * p.K);
        const float* b = p.boxes + (long)r * 4 * p.nreg + (p.nreg == 1 ? 0 : 4 * c);
        const float x1 = fminf(fmaxf(b[0], 0.f), p.img_w), y1 = fminf(fmaxf(b[1], 0.f), p.img_h);
        const float x2 = fminf(fmaxf(b[2], 0.f), p.img_w), y2 = fminf(fmaxf(b[3], 0.f), p.img_h);
        p.c_box[4 * (long)pos] = x1; p.c_box[4 * (long)pos + 1] = y1; p.c_box[4 * (long)pos + 2] = x2; p.c_box[4 * (long)pos + 3] = y2;
        p.c_score[pos] = sv[e]; p.c_row[pos] = p.rowmap[r]; p.c_cls[pos] = c;
        mymax = fmaxf(mymax, fmaxf(fmaxf(x1, y1), fmaxf(x2, y2)));
      }
      ++pos;
    }
  mymax = wave_max(mymax);
  // (clipped coordinates are >= 0, or NaN-free by the finite filter: their bit patterns order like the values; -inf stays for "none")
  if (lane == 0 && mymax >= 0.f) atomicMax((int*)p.maxcoord, __builtin_bit_cast(int, mymax));
  if ((int)blockIdx.x == ntiles - 1 && threadIdx.x == 0) {
    const int n = sbase + tot;
    p.count[0] = n < p.cap ? n : p.cap;
  }
}

// (the stable descending sort of the candidates by score lives in radix_sort.h: sort_hist_kernel / sort_scan_kernel /
// sort_scatter_kernel, shared with cocoeval.hip)

struct NmsParams {
  const float* c_box; const float* c_score; const int* c_cls;
  const int* order;  // candidate ids sorted by descending score (stable)
  const int* count; const float* maxcoord;
  float thr; int topk; int per_class_from;
  int* keep;       // [topk] candidate ids
  int* n_keep;     // [1]
};

constexpr int NMS_MAXK = 1024;

// one wave per image: the n candidates order[0 .. n) of one image, its own largest coordinate; leaves keep[0 .. n_keep[0])
__device__ __forceinline__ void nms_topk_wave(const NmsParams& p, const int* order, const int n, const float* maxcoord,
                                              int* keep, int* n_keep) {
  __shared__ float kb[NMS_MAXK][4];
  __shared__ float ka[NMS_MAXK];
  __shared__ int kc[NMS_MAXK];
  const int lane = threadIdx.x;
  // detectron2/layers/nms.py:19-29: >= 40000 boxes => per-class NMS on the raw boxes, no offsets
  const bool per_class = n >= p.per_class_from;
  const float offs = per_class ? 0.f : maxcoord[0] + 1.f;
  int nk = 0;
  for (int start = 0; start < n && nk < p.topk; start += 64) {
    const int i = start + lane;
    const bool valid = i < n;
    float x1 = 0, y1 = 0, x2 = 0, y2 = 0, area = 0;
    int id = -1, cls = -1;
    bool alive = valid;
    if (valid) {
      id = order[i];
      cls = p.c_cls[id];
      const float off = (float)cls * offs;  // idxs.to(boxes) * (boxes.max() + 1)
      x1 = p.c_box[4 * (long)id] + off; y1 = p.c_box[4 * (long)id + 1] + off;
      x2 = p.c_box[4 * (long)id + 2] + off; y2 = p.c_box[4 * (long)id + 3] + off;
      area = (x2 - x1) * (y2 - y1);
      for (int k = 0; k < nk && alive; ++k) {
        if (per_class && kc[k] != cls) continue;
        const float w = fmaxf(0.f, fminf(kb[k][2], x2) - fmaxf(kb[k][0], x1));
        const float h = fmaxf(0.f, fminf(kb[k][3], y2) - fmaxf(kb[k][1], y1));
        const float inter = w * h;
        if (inter / (ka[k] + area - inter) > p.thr) alive = false;
      }
    }
    // resolve the chunk in order: the lowest alive lane is kept and suppresses later lanes
    unsigned long long pending = __ballot(alive);
    while (pending && nk < p.topk) {
      const int l = __ffsll((long long)pending) - 1;
      const float bx1 = __shfl(x1, l, 64), by1 = __shfl(y1, l, 64), bx2 = __shfl(x2, l, 64), by2 = __shfl(y2, l, 64);
      const float ba = __shfl(area, l, 64);
      const int bid = __shfl(id, l, 64);
      const int bcls = __shfl(cls, l, 64);
      if (lane == 0) { kc[nk] = bcls; kb[nk][0] = bx1; kb[nk][1] = by1; kb[nk][2] = bx2; kb[nk][3] = by2; ka[nk] = ba; keep[nk] = bid; }
      ++nk;
      if (alive && lane > l && (!per_class || bcls == cls)) {
        const float w = fmaxf(0.f, fminf(bx2, x2) - fmaxf(bx1, x1));
        const float h = fmaxf(0.f, fminf(by2, y2) - fmaxf(by1, y1));
        const float inter = w * h;
        if (inter / (ba + area - inter) > p.thr) alive = false;
      }
      if (lane == l) alive = false;
      pending = __ballot(alive);
    }
    __syncthreads();
  }
  if (lane == 0) n_keep[0] = nk;
}

__global__ __launch_bounds__(64) void nms_topk_kernel(NmsParams p) {
  nms_topk_wave(p, p.order, p.count[0], p.maxcoord, p.keep, p.n_keep);
}

}  // namespace

namespace {

__global__ void gather_kernel(const float* c_box, const float* c_score, const int* c_row, const int* c_cls,
                              const int* keep, const int* n_keep, float* ob, float* os, int* oc, int* orow) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_keep[0]) return;
  const int id = keep[i];
  for (int e = 0; e < 4; ++e) ob[4 * i + e] = c_box[4 * (long)id + e];
  os[i] = c_score[id]; oc[i] = c_cls[id]; orow[i] = c_row[id];
}

struct Ws {
  float* c_box; float* c_score; unsigned* key0; int* c_row; int* c_cls; int* val0; int* order; int* count;
  float* maxcoord; unsigned* key1; int* hist;
};

inline int sort_tiles(int cap) { return (cap + SORT_TILE - 1) / SORT_TILE; }
inline long ws_fixed_bytes(int cap) { return (long)cap * (16 + 4 * 7) + 256 + (long)SORT_BINS * sort_tiles(cap) * 4; }

inline Ws carve(void* workspace, long bytes, int cap) {
  (void)bytes;
  Ws k;
  char* w = (char*)workspace;
  k.c_box = (float*)w; w += (long)cap * 16;
  k.c_score = (float*)w; w += (long)cap * 4;
  k.key0 = (unsigned*)w; w += (long)cap * 4;   // sort ping (doubles as the finite-row map until pass 1 writes it)
  k.c_row = (int*)w; w += (long)cap * 4;
  k.c_cls = (int*)w; w += (long)cap * 4;
  k.val0 = (int*)w; w += (long)cap * 4;
  k.order = (int*)w; w += (long)cap * 4;        // sort pong values = the final order
  k.key1 = (unsigned*)w; w += (long)cap * 4;
  k.count = (int*)w; k.maxcoord = (float*)(w + 8); w += 256;
  k.hist = (int*)w;
  return k;
}

// ---- the batched tail: all images of a call through ONE launch chain ----------------------------------------------
// The rows of image b are img_off[b] .. img_off[b+1]; every per-image rule of the reference stays per image (finite-row
// numbering, the boxes.max() + 1 offset, the >= 40000 switch, the clip, the early exit).  Global row-major entry order is
// already image-major, so ONE ordered compaction serves all images; it also leaves seg_off[b] = candidates in front of
// image b.  Three stable score passes over all candidates and one stable pass by image id then put every image's segment
// in descending score order with ties in candidate order; the NMS and the gather / postprocess run one wave per image.
constexpr int DET_MAX_IMAGES = 16;                      // include/drn_wsod.h DRN_DETECT_MAX_IMAGES
constexpr long DET_MAX_ENTRIES = (long)SORT_BINS * CAND_TILE;  // DRN_DETECT_BATCH_MAX_ENTRIES: the tile counts live in the histogram area

struct BatchGeom {
  int img_off[DET_MAX_IMAGES + 1];
  float h[DET_MAX_IMAGES], w[DET_MAX_IMAGES];    // the candidates are clipped to the image they were predicted on
  float oh[DET_MAX_IMAGES], ow[DET_MAX_IMAGES];  // detector_postprocess: scale by (sx, sy), clip to (oh, ow), drop empty
  float sx[DET_MAX_IMAGES], sy[DET_MAX_IMAGES];
  int n_img;
};

struct BatchParams {
  const float* boxes; const float* scores;
  int M, K, nreg;
  float thresh;
  float* c_box; float* c_score; int* c_row; int* c_cls;
  int* count;       // [1] candidates of all images
  int* seg_off;     // [n_img + 1]
  float* maxcoord;  // [n_img]
  int cap;
  int* rowmap;      // [M]
};

__device__ __forceinline__ int image_of(const int* off, int n_img, int v) {
  int b = 0;
  while (b + 1 < n_img && v >= off[b + 1]) ++b;
  return b;
}

// one workgroup per image: rows_number_kernel on the image's own rows
__global__ __launch_bounds__(1024) void rows_number_batch_kernel(BatchParams p, BatchGeom g) {
  __shared__ int wcnt[16];
  __shared__ int base;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r0 = g.img_off[blockIdx.x], r1 = g.img_off[blockIdx.x + 1];
  if (threadIdx.x == 0) {
    base = 0;
    p.maxcoord[blockIdx.x] = -INFINITY;
  }
  __syncthreads();
  for (int start = r0; start < r1; start += 1024) {
    const int r = start + threadIdx.x;
    const bool finite = r < r1 && p.rowmap[r] >= 0;
    const unsigned long long bal = __ballot(finite);
    const int wprefix = __popcll(bal & ((1ULL << lane) - 1ULL));
    if (lane == 0) wcnt[w] = __popcll(bal);
    __syncthreads();
    int woff = 0, tot = 0;
    for (int q = 0; q < 16; ++q) { if (q < w) woff += wcnt[q]; tot += wcnt[q]; }
    if (r < r1) p.rowmap[r] = finite ? base + woff + wprefix : -1;
    __syncthreads();
    if (threadIdx.x == 0) base += tot;
    __syncthreads();
  }
}

// candidates_kernel over the M x K entries of all images.  Pass 1 also leaves seg_off: the thread that holds an image's first entry
// knows how many candidates lie in front of it.  The largest clipped coordinate is kept per image (integer-bits atomic max: exact
// whatever the order); a thread whose entries cross an image boundary hands in what it has when the image changes.
template <int PASS>
__global__ __launch_bounds__(CAND_THREADS) void candidates_batch_kernel(BatchParams p, BatchGeom g, int* tile_cnt, int ntiles) {
  __shared__ int wcnt[CAND_THREADS / 64];
  __shared__ int sbase;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long total = (long)p.M * p.K;
  const long i0 = (long)blockIdx.x * CAND_TILE + (long)threadIdx.x * CAND_EPT;
  unsigned flags = 0;
  float sv[CAND_EPT];
  int n_mine = 0;
#pragma unroll
  for (int e = 0; e < CAND_EPT; ++e) {
    const long i = i0 + e;
    sv[e] = 0.f;
    if (i < total) {
      const int r = (int)(i / p.K), c = (int)(i - (long)r * p.K);
      sv[e] = p.scores[(long)r * (p.K + 1) + c];
      if (p.rowmap[r] >= 0 && sv[e] > p.thresh) flags |= 1u << e, ++n_mine;
    }
  }
  int incl = n_mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wcnt[w] = incl;
  if (PASS == 1 && threadIdx.x == 0) {
    int b = 0;
    for (int t = 0; t < (int)blockIdx.x; ++t) b += tile_cnt[t];
    sbase = b;
  }
  __syncthreads();
  int woff = 0, tot = 0;
  for (int q = 0; q < CAND_THREADS / 64; ++q) { if (q < w) woff += wcnt[q]; tot += wcnt[q]; }
  if (PASS == 0) {
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
    return;
  }
  int pos = sbase + woff + incl - n_mine;
  int img = -1;
  bool crossed = false;
  float mymax = -INFINITY;
#pragma unroll
  for (int e = 0; e < CAND_EPT; ++e) {
    const long i = i0 + e;
    if (i >= total) break;
    const int r = (int)(i / p.K), c = (int)(i - (long)r * p.K);
    if (c == 0)  // the first entry of image b (an image without rows shares it with its successor)
      for (int b = 0; b < g.n_img; ++b)
        if (g.img_off[b] == r) p.seg_off[b] = pos;
    if (flags >> e & 1) {
      const int b = image_of(g.img_off, g.n_img, r);
      if (b != img) {
        if (mymax >= 0.f) atomicMax((int*)p.maxcoord + img, __builtin_bit_cast(int, mymax));
        crossed = crossed || img >= 0;
        img = b;
        mymax = -INFINITY;
      }
      if (pos < p.cap) {
        const float* bx = p.boxes + (long)r * 4 * p.nreg + (p.nreg == 1 ? 0 : 4 * c);
        const float iw = g.w[b], ih = g.h[b];
        const float x1 = fminf(fmaxf(bx[0], 0.f), iw), y1 = fminf(fmaxf(bx[1], 0.f), ih);
        const float x2 = fminf(fmaxf(bx[2], 0.f), iw), y2 = fminf(fmaxf(bx[3], 0.f), ih);
        p.c_box[4 * (long)pos] = x1; p.c_box[4 * (long)pos + 1] = y1; p.c_box[4 * (long)pos + 2] = x2; p.c_box[4 * (long)pos + 3] = y2;
        p.c_score[pos] = sv[e]; p.c_row[pos] = p.rowmap[r]; p.c_cls[pos] = c;
        mymax = fmaxf(mymax, fmaxf(fmaxf(x1, y1), fmaxf(x2, y2)));
      }
      ++pos;
    }
  }
  // one atomic per wave where all its candidates lie in one image, one per lane where an image boundary runs through the wave
  int lo = img < 0 ? DET_MAX_IMAGES : img, hi = img;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o, 64));
    hi = max(hi, __shfl_xor(hi, o, 64));
  }
  if (__ballot(crossed) == 0 && lo >= hi) {
    mymax = wave_max(mymax);
    if (lane == 0 && hi >= 0 && mymax >= 0.f) atomicMax((int*)p.maxcoord + hi, __builtin_bit_cast(int, mymax));
  } else if (img >= 0 && mymax >= 0.f) {
    atomicMax((int*)p.maxcoord + img, __builtin_bit_cast(int, mymax));
  }
  if ((int)blockIdx.x == ntiles - 1 && threadIdx.x == 0) {
    const int n = sbase + tot;
    p.count[0] = n < p.cap ? n : p.cap;
    for (int b = 0; b <= g.n_img; ++b)  // images without rows at the end, and the end itself
      if (g.img_off[b] >= p.M) p.seg_off[b] = n;
  }
}

// key[j] = image of the candidate at sorted position j: candidate ids are image-major, seg_off bounds them
__global__ void image_key_kernel(const int* __restrict__ order, const int* __restrict__ count, const int* __restrict__ seg_off,
                                 int n_img, unsigned* __restrict__ key) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count[0]) return;
  key[j] = (unsigned)image_of(seg_off, n_img, order[j]);
}

// one wave per image on its own segment of the sorted order
__global__ __launch_bounds__(64) void nms_topk_batch_kernel(NmsParams p, const int* seg_off) {
  const int b = blockIdx.x, s0 = seg_off[b];
  nms_topk_wave(p, p.order + s0, seg_off[b + 1] - s0, p.maxcoord + b, p.keep + (long)b * p.topk, p.n_keep + b);
}

struct PostParams {
  const float* c_box; const float* c_score; const int* c_row; const int* c_cls;
  const int* keep; const int* n_keep;
  int topk, postprocess;
  float* ob; float* os; int* oc; int* orow; int* ocount;
};

// one wave per image: drn_detect_gather, then detector_postprocess (scale, clip to the output size, drop boxes with w <= 0 or
// h <= 0 keeping the order: a ballot prefix), then the fill of the slots at and beyond the count
__global__ __launch_bounds__(64) void gather_post_kernel(PostParams p, BatchGeom g) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nk = min(p.n_keep[b], p.topk);
  const float sx = g.sx[b], sy = g.sy[b], ow = g.ow[b], oh = g.oh[b];
  const long o0 = (long)b * p.topk;
  int base = 0;
  for (int start = 0; start < nk; start += 64) {
    const int s = start + lane;
    bool live = s < nk;
    float x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    int id = 0;
    if (live) {
      id = p.keep[o0 + s];
      x1 = p.c_box[4 * (long)id]; y1 = p.c_box[4 * (long)id + 1]; x2 = p.c_box[4 * (long)id + 2]; y2 = p.c_box[4 * (long)id + 3];
      if (p.postprocess) {
        x1 = x1 * sx; x2 = x2 * sx; y1 = y1 * sy; y2 = y2 * sy;
        x1 = fminf(fmaxf(x1, 0.f), ow); y1 = fminf(fmaxf(y1, 0.f), oh);
        x2 = fminf(fmaxf(x2, 0.f), ow); y2 = fminf(fmaxf(y2, 0.f), oh);
        live = (x2 - x1) > 0.f && (y2 - y1) > 0.f;
      }
    }
    const unsigned long long bal = __ballot(live);
    if (live) {
      const long o = o0 + base + __popcll(bal & ((1ULL << lane) - 1ULL));
      p.ob[4 * o] = x1; p.ob[4 * o + 1] = y1; p.ob[4 * o + 2] = x2; p.ob[4 * o + 3] = y2;
      p.os[o] = p.c_score[id]; p.oc[o] = p.c_cls[id]; p.orow[o] = p.c_row[id];
    }
    base += __popcll(bal);
  }
  for (int s = base + lane; s < p.topk; s += 64) {
    const long o = o0 + s;
    p.ob[4 * o] = 0.f; p.ob[4 * o + 1] = 0.f; p.ob[4 * o + 2] = 0.f; p.ob[4 * o + 3] = 0.f;
    p.os[o] = 0.f; p.oc[o] = -1; p.orow[o] = -1;
  }
  if (lane == 0) p.ocount[b] = base;
}

struct BatchWs {
  int* seg_off; float* maxcoord; int* n_keep; int* keep;
};
constexpr long BATCH_WS_HEAD = 512;
inline long batch_ws_bytes(int cap, int n_img) { return ws_fixed_bytes(cap) + BATCH_WS_HEAD + (long)n_img * NMS_MAXK * 4; }
inline BatchWs carve_batch(void* workspace, int cap) {
  char* w = (char*)workspace + ws_fixed_bytes(cap);
  return BatchWs{(int*)w, (float*)(w + 128), (int*)(w + 256), (int*)(w + BATCH_WS_HEAD)};
}

// ---- the tail shared by the batched entries: everything behind the candidates -----------------------------------------
// On entry c_box / c_score / c_row / c_cls hold the candidates of all images in image-major order, count[0] their number (held
// to cap), seg_off[b] the candidates in front of image b and maxcoord[b] the image's largest clipped coordinate (-inf: none).
// Stable descending by score over all candidates: -> key1/order -> key0/val0 -> key1/order; then stable by image: -> key0/val0;
// the NMS and the gather / postprocess run one wave per image.  15 launches whatever n_images is.
void launch_sorted_tail(const Ws& k, const BatchWs& bw, const BatchGeom& g, int cap, int n_images, int postprocess,
                        float nms_thresh, int topk, float* out_boxes, float* out_scores, int* out_classes, int* out_rows,
                        int* out_count, hipStream_t st) {
  const int tiles = sort_tiles(cap);
  const int shifts[3] = {0, 11, 22}, bits[3] = {11, 11, 10};
  for (int ps = 0; ps < 3; ++ps) {
    const bool even = (ps & 1) == 0;
    SortPass sp{k.c_score, even ? k.key0 : k.key1, even ? k.val0 : k.order, even ? k.key1 : k.key0,
                even ? k.order : k.val0, k.hist, k.count, tiles, shifts[ps], bits[ps], ps == 0};
    hipLaunchKernelGGL(sort_hist_kernel, dim3(tiles), dim3(SORT_THREADS), 0, st, sp);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 0, st, sp);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(tiles), dim3(SORT_THREADS), 0, st, sp);
  }
  hipLaunchKernelGGL(image_key_kernel, dim3((cap + 255) / 256), dim3(256), 0, st, k.order, k.count, bw.seg_off, n_images,
                     k.key1);
  {
    SortPass sp{nullptr, k.key1, k.order, k.key0, k.val0, k.hist, k.count, tiles, 0, 4, 0};  // 4 bits: DET_MAX_IMAGES = 16
    hipLaunchKernelGGL(sort_hist_kernel, dim3(tiles), dim3(SORT_THREADS), 0, st, sp);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 0, st, sp);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(tiles), dim3(SORT_THREADS), 0, st, sp);
  }
  NmsParams np{k.c_box, k.c_score, k.c_cls, k.val0, k.count, bw.maxcoord, nms_thresh, topk, 40000, bw.keep, bw.n_keep};
  hipLaunchKernelGGL(nms_topk_batch_kernel, dim3(n_images), dim3(64), 0, st, np, (const int*)bw.seg_off);
  PostParams pp{k.c_box, k.c_score, k.c_row, k.c_cls, bw.keep, bw.n_keep, topk, postprocess ? 1 : 0, out_boxes, out_scores,
                out_classes, out_rows, out_count};
  hipLaunchKernelGGL(gather_post_kernel, dim3(n_images), dim3(64), 0, st, pp, g);
}

// ---- union of per-pass detections (wsl/modeling/test_time_augmentation_union.py:228-264) ---------------------------------
// The candidates of the merge come from padded detection blocks instead of an [M][K+1] score matrix: slot s of block b is a
// union row iff s < min(count[b], blk_topk); the blocks of image i are img_off[i] .. img_off[i+1].  Its box is mapped back
// to the original image with the block's own (sx, sy, flip_w) and the row is dropped BEFORE numbering when the mapped box or the
// score is not finite (detectron2 fast_rcnn.py:95-98); it is a candidate iff score > thresh and 0 <= class < K (the one non-zero
// entry of its row of the reference's one-hot [n, K+1] matrix), with the box clipped to the original (h, w).  Candidates are
// written in (block, slot) order = the row-major nonzero() order of that matrix.  One wave per block, two launches: pass 0
// leaves every block's finite-row and candidate counts (and keeps the per-block transforms, which arrive as kernel arguments,
// for pass 1), pass 1 places a block behind the sums of the counts in front of it.  Nothing beyond a block's count is read.
constexpr int UNION_MAX_BLOCKS = 256;  // include/drn_wsod.h DRN_DETECT_UNION_MAX_BLOCKS

// Per block (sx, sy, flip_w): 3 KiB of kernel arguments, which the runtime copies at the launch - so the host array is free when
// the entry returns, without a staging buffer or a copy engine in the chain.  Only pass 0 takes the table and leaves it in the
// workspace (three 4-byte stores per block) for pass 1: pass 1 already carries BatchGeom, and UnionParams + BatchGeom + this table
// would come to ~3.6 KiB of the 4 KiB a launch may pass - too close to the limit to grow either struct later.
// Both passes evaluate union_slot in full (load, back-transform, finite / candidate test): that is the price of two passes;
// keeping pass 0's verdicts and boxes instead would cost a 20-byte store and load per slot to save ~10 VALU operations.
struct UnionTfm { float v[UNION_MAX_BLOCKS][3]; };

struct UnionParams {
  const float* blk_boxes; const float* blk_scores; const int* blk_classes; const int* blk_count;
  int n_blocks, blk_topk, K;
  float thresh;
  float* c_box; float* c_score; int* c_row; int* c_cls;
  int* count;       // [1] candidates of all images
  int* seg_off;     // [n_img + 1]
  float* maxcoord;  // [n_img]
  int cap;
  int* blk_fin;     // [n_blocks] finite rows of the block
  int* blk_cand;    // [n_blocks] candidates of the block
  float* tfm;       // [n_blocks][3]
};

struct UnionWs { int* blk_fin; int* blk_cand; float* tfm; };
constexpr long UNION_WS_BYTES = (long)UNION_MAX_BLOCKS * (4 + 4 + 12);
inline UnionWs carve_union(void* workspace, int cap, int n_img) {
  char* w = (char*)workspace + batch_ws_bytes(cap, n_img);
  return UnionWs{(int*)w, (int*)(w + UNION_MAX_BLOCKS * 4), (float*)(w + UNION_MAX_BLOCKS * 8)};
}

// what slot s of block b is: bit 0 = a union row (finite), bit 1 = a candidate; o = the box on the original image, unclipped
__device__ __forceinline__ int union_slot(const UnionParams& p, int b, int s, float sx, float sy, float flip_w, float o[4],
                                          float* score, int* cls) {
  const long i = (long)b * p.blk_topk + s;
  const float* raw = p.blk_boxes + 4 * i;
  tta_inverse_box(raw, sx, sy, flip_w, o);
  *score = p.blk_scores[i];
  *cls = p.blk_classes[i];
  // (numpy's min / max hand a NaN corner on, fminf / fmaxf drop it: the raw coordinates are looked at as well)
  const bool finite = isfinite(raw[0]) && isfinite(raw[1]) && isfinite(raw[2]) && isfinite(raw[3]) && isfinite(o[0]) &&
                      isfinite(o[1]) && isfinite(o[2]) && isfinite(o[3]) && isfinite(*score);
  const bool cand = finite && *score > p.thresh && *cls >= 0 && *cls < p.K;
  return (finite ? 1 : 0) | (cand ? 2 : 0);
}

__global__ __launch_bounds__(64) void union_count_kernel(UnionParams p, UnionTfm t, int n_img) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float sx = t.v[b][0], sy = t.v[b][1], flip_w = t.v[b][2];
  if (b == 0 && lane < n_img) p.maxcoord[lane] = -INFINITY;
  if (lane < 3) p.tfm[3 * b + lane] = t.v[b][lane];
  const int n = min(max(p.blk_count[b], 0), p.blk_topk);
  int nfin = 0, ncand = 0;
  for (int start = 0; start < n; start += 64) {
    const int s = start + lane;
    int what = 0;
    if (s < n) {
      float o[4], score;
      int cls;
      what = union_slot(p, b, s, sx, sy, flip_w, o, &score, &cls);
    }
    nfin += __popcll(__ballot(what & 1));
    ncand += __popcll(__ballot(what & 2));
  }
  if (lane == 0) { p.blk_fin[b] = nfin; p.blk_cand[b] = ncand; }
}

__global__ __launch_bounds__(64) void union_place_kernel(UnionParams p, BatchGeom g) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int img = image_of(g.img_off, g.n_img, b);
  // candidates of all blocks in front of this one; finite rows of this image's blocks in front of this one
  int cbase = 0, rbase = 0;
  for (int q = lane; q < b; q += 64) {
    cbase += p.blk_cand[q];
    if (q >= g.img_off[img]) rbase += p.blk_fin[q];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cbase += __shfl_xor(cbase, o, 64);
    rbase += __shfl_xor(rbase, o, 64);
  }
  if (lane == 0)  // the first block of image i (an image without blocks shares it with its successor)
    for (int i = 0; i < g.n_img; ++i)
      if (g.img_off[i] == b) p.seg_off[i] = cbase;
  const float sx = p.tfm[3 * b], sy = p.tfm[3 * b + 1], flip_w = p.tfm[3 * b + 2];
  const float iw = g.w[img], ih = g.h[img];
  const int n = min(max(p.blk_count[b], 0), p.blk_topk);
  int pos0 = cbase, row0 = rbase;
  float mymax = -INFINITY;
  for (int start = 0; start < n; start += 64) {
    const int s = start + lane;
    int what = 0, cls = -1;
    float o[4] = {0.f, 0.f, 0.f, 0.f}, score = 0.f;
    if (s < n) what = union_slot(p, b, s, sx, sy, flip_w, o, &score, &cls);
    const unsigned long long fbal = __ballot(what & 1), cbal = __ballot(what & 2);
    const unsigned long long below = (1ULL << lane) - 1ULL;
    if (what & 2) {
      const int pos = pos0 + __popcll(cbal & below);
      if (pos < p.cap) {
        const float x1 = fminf(fmaxf(o[0], 0.f), iw), y1 = fminf(fmaxf(o[1], 0.f), ih);
        const float x2 = fminf(fmaxf(o[2], 0.f), iw), y2 = fminf(fmaxf(o[3], 0.f), ih);
        p.c_box[4 * (long)pos] = x1; p.c_box[4 * (long)pos + 1] = y1; p.c_box[4 * (long)pos + 2] = x2; p.c_box[4 * (long)pos + 3] = y2;
        p.c_score[pos] = score; p.c_row[pos] = row0 + __popcll(fbal & below); p.c_cls[pos] = cls;
        mymax = fmaxf(mymax, fmaxf(fmaxf(x1, y1), fmaxf(x2, y2)));
      }
    }
    pos0 += __popcll(cbal);
    row0 += __popcll(fbal);
  }
  mymax = wave_max(mymax);
  // (clipped coordinates are >= 0 and finite: their bit patterns order like the values; -inf stays for "none")
  if (lane == 0 && mymax >= 0.f) atomicMax((int*)p.maxcoord + img, __builtin_bit_cast(int, mymax));
  if (b == p.n_blocks - 1 && lane == 0) {
    p.count[0] = pos0 < p.cap ? pos0 : p.cap;
    for (int i = 0; i <= g.n_img; ++i)  // images without blocks at the end, and the end itself
      if (g.img_off[i] >= p.n_blocks) p.seg_off[i] = pos0;
  }
}

// ---- padded blocks -> packed detections -------------------------------------------------------------------------------
// off[b] = sum of the counts (held to 0 .. topk) in front of block b, off[B] = n: one workgroup
__global__ __launch_bounds__(1024) void compact_offsets_kernel(const int* __restrict__ count, int B, int topk, int* __restrict__ off,
                                                               int* __restrict__ out_n) {
  __shared__ int wsum[16];
  __shared__ int base;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (int start = 0; start < B; start += 1024) {
    const int b = start + threadIdx.x;
    const int c = b < B ? min(max(count[b], 0), topk) : 0;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
    for (int q = 0; q < 16; ++q) { if (q < w) woff += wsum[q]; tot += wsum[q]; }
    if (b < B) off[b] = base + woff + incl - c;
    __syncthreads();
    if (threadIdx.x == 0) base += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) { off[B] = base; out_n[0] = base; }
}

__global__ __launch_bounds__(64) void compact_gather_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                            const int* __restrict__ classes, const int* __restrict__ image_index,
                                                            const int* __restrict__ off, int topk, float* __restrict__ ob,
                                                            float* __restrict__ os, int* __restrict__ oc, int* __restrict__ oi) {
  const int b = blockIdx.x;
  const int o0 = off[b], n = off[b + 1] - o0, im = image_index[b];
  for (int s = threadIdx.x; s < n; s += 64) {
    const long i = (long)b * topk + s, o = o0 + s;
    for (int e = 0; e < 4; ++e) ob[4 * o + e] = boxes[4 * i + e];
    os[o] = scores[i]; oc[o] = classes[i]; oi[o] = im;
  }
}

}  // namespace

// ---- test-time augmentation (wsl/modeling/test_time_augmentation_avg.py:269-294) --------------------------------
// One augmentation's predictions folded into the running averages on the device: every predicted box is mapped back
// to the original image - HFlipTransform.inverse (x -> W' - x) then ResizeTransform.inverse (x * sx, y * sy) applied
// to its four corners, then their bounding box, in float32 exactly like the numpy code the reference runs on the
// host - and added to acc_boxes; the scores are added to acc_scores.  The last augmentation divides by n_aug (torch.mean).
// The reference moves every augmentation's [R, 4K] boxes to the host and back for this.
__global__ void tta_accumulate_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                      float* __restrict__ acc_boxes, float* __restrict__ acc_scores, long nbox, long nscore,
                                      float sx, float sy, float flip_w, int first, int n_final) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i < nbox) {
    float o[4];
    tta_inverse_box(boxes + 4 * i, sx, sy, flip_w, o);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = first ? o[e] : acc_boxes[4 * i + e] + o[e];
      if (n_final > 0) v = v / (float)n_final;
      acc_boxes[4 * i + e] = v;
    }
  }
  if (i < nscore) {
    float v = first ? scores[i] : acc_scores[i] + scores[i];
    if (n_final > 0) v = v / (float)n_final;
    acc_scores[i] = v;
  }
}

namespace {

// The single-image candidate stages, shared by drn_detect_topk and drn_detect_all: finite-row filter, threshold + ordered compaction
// (background column dropped, boxes clipped), stable descending sort.  Leaves the candidates in k.c_*, their number in k.count,
// the largest clipped coordinate in k.maxcoord and the sorted candidate ids in k.order.
int launch_candidates_sorted(const Ws& k, const float* boxes, const float* scores, int R, int K, int nreg, float img_h, float img_w,
                             float score_thresh, int cap, hipStream_t st) {
  CandParams cp{boxes, scores, R, K, nreg, img_h, img_w, score_thresh, k.c_box, k.c_score, k.c_row, k.c_cls, k.count,
                k.maxcoord, cap, (int*)k.key0};  // key0 doubles as the row map until the sort's second pass overwrites it
  if (R > 0) hipLaunchKernelGGL(rows_finite_kernel, dim3((R + 3) / 4), dim3(256), 0, st, cp);
  hipLaunchKernelGGL(rows_number_kernel, dim3(1), dim3(1024), 0, st, cp);
  const long total = (long)R * K;
  const int ntiles = (int)((total + CAND_TILE - 1) / CAND_TILE);
  if (ntiles > SORT_BINS) return DRN_ERR_UNSUPPORTED;  // (8M scores per image; the tile counts live in the sort's histogram area)
  if (ntiles > 0) {
    hipLaunchKernelGGL(candidates_kernel<0>, dim3(ntiles), dim3(CAND_THREADS), 0, st, cp, k.hist, ntiles);
    hipLaunchKernelGGL(candidates_kernel<1>, dim3(ntiles), dim3(CAND_THREADS), 0, st, cp, k.hist, ntiles);
  } else {
    (void)hipMemsetAsync(k.count, 0, sizeof(int), st);
  }
  // stable descending order of the live candidates: (score, index) -> key1/order -> key0/val0 -> key1/order
  const int tiles = sort_tiles(cap);
  const int shifts[3] = {0, 11, 22}, bits[3] = {11, 11, 10};
  for (int ps = 0; ps < 3; ++ps) {
    const bool even = (ps & 1) == 0;
    SortPass sp{k.c_score, even ? k.key0 : k.key1, even ? k.val0 : k.order, even ? k.key1 : k.key0,
                even ? k.order : k.val0, k.hist, k.count, tiles, shifts[ps], bits[ps], ps == 0};
    hipLaunchKernelGGL(sort_hist_kernel, dim3(tiles), dim3(SORT_THREADS), 0, st, sp);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 0, st, sp);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(tiles), dim3(SORT_THREADS), 0, st, sp);
  }
  return DRN_OK;
}

// drn_detect_all's workspace: drn_detect_topk's, then (64-byte aligned) the kept candidate ids and the suppression stage's share
inline long all_keep_offset(int cap) { return (ws_fixed_bytes(cap) + 256 + 63) / 64 * 64; }

}  // namespace

extern "C" {

// bytes of scratch drn_detect_topk needs for up to `cap` candidates (cap = R*K is always enough)
long drn_detect_workspace_bytes(int cap) { return ws_fixed_bytes(cap < 1 ? 1 : cap) + 256; }

// Single image.  boxes [R][4*nreg], scores [R][K+1] (last column = background).  Leaves the kept
// candidate ids (descending score) in keep_ids[0..n_keep) on the device; drn_detect_gather expands them.
int drn_detect_topk(const float* boxes, const float* scores, int R, int K, int nreg, float img_h, float img_w,
                    float score_thresh, float nms_thresh, int topk, void* workspace, long workspace_bytes, int cap,
                    int* keep_ids, int* n_keep, void* stream) {
  if (!boxes || !scores || !workspace || !keep_ids || !n_keep || topk < 1 || topk > NMS_MAXK || cap < 1 || R < 0)
    return DRN_ERR_ARG;
  if (nreg != 1 && nreg != K) return DRN_ERR_ARG;
  if (cap < R) return DRN_ERR_ARG;
  if (workspace_bytes < drn_detect_workspace_bytes(cap)) return DRN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Ws k = carve(workspace, workspace_bytes, cap);
  const int rc = launch_candidates_sorted(k, boxes, scores, R, K, nreg, img_h, img_w, score_thresh, cap, st);
  if (rc != DRN_OK) return rc;
  NmsParams np{k.c_box, k.c_score, k.c_cls, k.order, k.count, k.maxcoord, nms_thresh, topk, 40000, keep_ids, n_keep};
  hipLaunchKernelGGL(nms_topk_kernel, dim3(1), dim3(64), 0, st, np);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_detect_gather(const void* workspace, long workspace_bytes, int cap, const int* keep_ids, const int* n_keep,
                      int topk, float* out_boxes, float* out_scores, int* out_classes, int* out_rows, void* stream) {
  if (!workspace || !keep_ids || !n_keep || !out_boxes || !out_scores || !out_classes || !out_rows) return DRN_ERR_ARG;
  Ws k = carve((void*)workspace, workspace_bytes, cap);
  hipLaunchKernelGGL(gather_kernel, dim3((topk + 63) / 64), dim3(64), 0, (hipStream_t)stream, k.c_box, k.c_score,
                     k.c_row, k.c_cls, keep_ids, n_keep, out_boxes, out_scores, out_classes, out_rows);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// bytes of scratch drn_detect_all needs: the candidate stages' share, the kept ids, the suppression stage of nms.hip
long drn_detect_all_workspace_bytes(int cap) {
  const long c = cap < 1 ? 1 : cap;
  return all_keep_offset((int)c) + (c * 4 + 63) / 64 * 64 + drn_supp::suppress_ws_bytes(c);
}

// The single-image tail without the 1024 cap (see include/drn_wsod.h): the candidate stages of drn_detect_topk, the panelled
// NMS of nms.hip over all sorted candidates, the gather.  topk < 0 keeps every survivor, topk >= 1 the first topk.
int drn_detect_all(const float* boxes, const float* scores, int R, int K, int nreg, float img_h, float img_w,
                   float score_thresh, float nms_thresh, int topk, void* workspace, long workspace_bytes, int cap,
                   float* out_boxes, float* out_scores, int* out_classes, int* out_rows, int* out_count, void* stream) {
  if (!boxes || !scores || !workspace || !out_boxes || !out_scores || !out_classes || !out_rows || !out_count || topk == 0 ||
      cap < 1 || R < 0 || K < 1)
    return DRN_ERR_ARG;
  if (nreg != 1 && nreg != K) return DRN_ERR_ARG;
  if (cap < R) return DRN_ERR_ARG;
  if ((long)R * K > drn_supp::MAX_N || cap > drn_supp::MAX_N) return DRN_ERR_UNSUPPORTED;
  if (((uintptr_t)workspace & 15) || workspace_bytes < drn_detect_all_workspace_bytes(cap)) return DRN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Ws k = carve(workspace, workspace_bytes, cap);
  const int rc = launch_candidates_sorted(k, boxes, scores, R, K, nreg, img_h, img_w, score_thresh, cap, st);
  if (rc != DRN_OK) return rc;
  char* w = (char*)workspace + all_keep_offset(cap);
  int* keep = (int*)w;
  w += ((long)cap * 4 + 63) / 64 * 64;
  drn_supp::SuppressIn in{k.c_box, k.c_cls, k.order, k.count, k.maxcoord, nullptr, 40000, nms_thresh, topk < 0 ? 0x7fffffff : topk};
  drn_supp::launch_suppress(in, cap, w, keep, nullptr, out_count, st);
  const int slots = topk < 0 || topk > cap ? cap : topk;
  hipLaunchKernelGGL(gather_kernel, dim3((slots + 63) / 64), dim3(64), 0, st, k.c_box, k.c_score, k.c_row, k.c_cls,
                     (const int*)keep, (const int*)out_count, out_boxes, out_scores, out_classes, out_rows);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// bytes of scratch drn_detect_topk_batch needs for n_images images with total_cap = M * K entries in all
long drn_detect_batch_workspace_bytes(int total_cap, int n_images) {
  return batch_ws_bytes(total_cap < 1 ? 1 : total_cap, n_images < 1 ? 1 : n_images) + 256;
}

// All images of a call (see include/drn_wsod.h).  img_off_host [n_images + 1] and geom_host [n_images][6] =
// (h, w, out_h, out_w, sx, sy) are HOST arrays, read before the call returns.  Nothing is read back from the device.
int drn_detect_topk_batch(const float* boxes, const float* scores, const int* img_off_host, int n_images, int K, int nreg,
                          const float* geom_host, int postprocess, float score_thresh, float nms_thresh, int topk,
                          void* workspace, long workspace_bytes, int total_cap, float* out_boxes, float* out_scores,
                          int* out_classes, int* out_rows, int* out_count, void* stream) {
  if (!boxes || !scores || !img_off_host || !geom_host || !workspace || !out_boxes || !out_scores || !out_classes ||
      !out_rows || !out_count || topk < 1 || topk > NMS_MAXK || total_cap < 1 || K < 1)
    return DRN_ERR_ARG;
  if (nreg != 1 && nreg != K) return DRN_ERR_ARG;
  if (n_images < 1 || n_images > DET_MAX_IMAGES) return DRN_ERR_UNSUPPORTED;
  BatchGeom g{};
  g.n_img = n_images;
  if (img_off_host[0] != 0) return DRN_ERR_ARG;
  for (int b = 0; b <= n_images; ++b) {
    g.img_off[b] = img_off_host[b];
    if (b > 0 && img_off_host[b] < img_off_host[b - 1]) return DRN_ERR_ARG;
  }
  for (int b = n_images + 1; b <= DET_MAX_IMAGES; ++b) g.img_off[b] = img_off_host[n_images];
  for (int b = 0; b < n_images; ++b) {
    const float* q = geom_host + 6 * b;
    g.h[b] = q[0]; g.w[b] = q[1]; g.oh[b] = q[2]; g.ow[b] = q[3]; g.sx[b] = q[4]; g.sy[b] = q[5];
  }
  const int M = img_off_host[n_images];
  const long total = (long)M * K;
  if (total > DET_MAX_ENTRIES) return DRN_ERR_UNSUPPORTED;
  if ((long)total_cap < total || total_cap > DET_MAX_ENTRIES) return DRN_ERR_ARG;
  const int cap = total_cap;
  if (workspace_bytes < drn_detect_batch_workspace_bytes(cap, n_images)) return DRN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  Ws k = carve(workspace, workspace_bytes, cap);
  BatchWs bw = carve_batch(workspace, cap);
  CandParams fp{boxes, scores, M, K, nreg, 0.f, 0.f, score_thresh, k.c_box, k.c_score, k.c_row, k.c_cls, k.count,
                k.maxcoord, cap, (int*)k.key0};  // key0 doubles as the row map until the sort's second pass overwrites it
  BatchParams bp{boxes, scores, M, K, nreg, score_thresh, k.c_box, k.c_score, k.c_row, k.c_cls, k.count, bw.seg_off,
                 bw.maxcoord, cap, (int*)k.key0};
  if (M > 0) hipLaunchKernelGGL(rows_finite_kernel, dim3((M + 3) / 4), dim3(256), 0, st, fp);
  hipLaunchKernelGGL(rows_number_batch_kernel, dim3(n_images), dim3(1024), 0, st, bp, g);
  const int ntiles = (int)((total + CAND_TILE - 1) / CAND_TILE);
  if (ntiles > 0) {
    hipLaunchKernelGGL(candidates_batch_kernel<0>, dim3(ntiles), dim3(CAND_THREADS), 0, st, bp, g, k.hist, ntiles);
    hipLaunchKernelGGL(candidates_batch_kernel<1>, dim3(ntiles), dim3(CAND_THREADS), 0, st, bp, g, k.hist, ntiles);
  } else {
    (void)(void)hipMemsetAsync(k.count, 0, sizeof(int), st);
    (void)hipMemsetAsync(bw.seg_off, 0, sizeof(int) * (DET_MAX_IMAGES + 1), st);
  }
  launch_sorted_tail(k, bw, g, cap, n_images, postprocess, nms_thresh, topk, out_boxes, out_scores, out_classes, out_rows,
                     out_count, st);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// bytes of scratch drn_detect_union_batch needs for n_images images with total_cap >= n_blocks * blk_topk slots in all
long drn_detect_union_workspace_bytes(int total_cap, int n_images) {
  return batch_ws_bytes(total_cap < 1 ? 1 : total_cap, n_images < 1 ? 1 : n_images) + UNION_WS_BYTES + 256;
}

// The union merge of per-pass detections (see include/drn_wsod.h).  img_off_host [n_images + 1] (in blocks), tfm_host
// [n_blocks][3] and geom_host [n_images][2] are HOST arrays, read before the call returns.  Nothing is read back from the device.
int drn_detect_union_batch(const float* blk_boxes, const float* blk_scores, const int* blk_classes, const int* blk_count,
                           int n_blocks, int blk_topk, const int* img_off_host, int n_images, const float* tfm_host,
                           const float* geom_host, int K, float score_thresh, float nms_thresh, int topk, void* workspace,
                           long workspace_bytes, int total_cap, float* out_boxes, float* out_scores, int* out_classes,
                           int* out_rows, int* out_count, void* stream) {
  if (!blk_boxes || !blk_scores || !blk_classes || !blk_count || !img_off_host || !tfm_host || !geom_host || !workspace ||
      !out_boxes || !out_scores || !out_classes || !out_rows || !out_count || total_cap < 1 || K < 1)
    return DRN_ERR_ARG;
  if (n_images < 1 || n_images > DET_MAX_IMAGES || n_blocks < 1 || n_blocks > UNION_MAX_BLOCKS || blk_topk < 1 ||
      blk_topk > NMS_MAXK || topk < 1 || topk > NMS_MAXK)
    return DRN_ERR_UNSUPPORTED;
  BatchGeom g{};
  g.n_img = n_images;
  if (img_off_host[0] != 0 || img_off_host[n_images] != n_blocks) return DRN_ERR_ARG;
  for (int b = 0; b <= n_images; ++b) {
    g.img_off[b] = img_off_host[b];
    if (b > 0 && img_off_host[b] < img_off_host[b - 1]) return DRN_ERR_ARG;
  }
  for (int b = n_images + 1; b <= DET_MAX_IMAGES; ++b) g.img_off[b] = n_blocks;
  for (int b = 0; b < n_images; ++b) {  // merged instances are not postprocessed: (oh, ow, sx, sy) only mirror (h, w, 1, 1)
    g.h[b] = g.oh[b] = geom_host[2 * b]; g.w[b] = g.ow[b] = geom_host[2 * b + 1];
    g.sx[b] = g.sy[b] = 1.f;
  }
  const long slots = (long)n_blocks * blk_topk;
  if ((long)total_cap < slots || total_cap > DET_MAX_ENTRIES) return DRN_ERR_ARG;
  const int cap = total_cap;
  if (workspace_bytes < drn_detect_union_workspace_bytes(cap, n_images)) return DRN_ERR_ARG;
  UnionTfm t{};
  for (int b = 0; b < n_blocks; ++b)
    for (int e = 0; e < 3; ++e) t.v[b][e] = tfm_host[3 * b + e];
  hipStream_t st = (hipStream_t)stream;
  Ws k = carve(workspace, workspace_bytes, cap);
  BatchWs bw = carve_batch(workspace, cap);
  UnionWs uw = carve_union(workspace, cap, n_images);
  UnionParams up{blk_boxes, blk_scores, blk_classes, blk_count, n_blocks, blk_topk, K, score_thresh, k.c_box, k.c_score,
                 k.c_row, k.c_cls, k.count, bw.seg_off, bw.maxcoord, cap, uw.blk_fin, uw.blk_cand, uw.tfm};
  hipLaunchKernelGGL(union_count_kernel, dim3(n_blocks), dim3(64), 0, st, up, t, n_images);
  hipLaunchKernelGGL(union_place_kernel, dim3(n_blocks), dim3(64), 0, st, up, g);
  launch_sorted_tail(k, bw, g, cap, n_images, 0, nms_thresh, topk, out_boxes, out_scores, out_classes, out_rows, out_count, st);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

// n_blocks padded blocks of topk slots -> the live slots packed in block order then slot order; offsets [n_blocks + 1] is scratch
int drn_detect_compact(const float* boxes, const float* scores, const int* classes, const int* count, const int* image_index,
                       int n_blocks, int topk, int* offsets, float* out_boxes, float* out_scores, int* out_classes,
                       int* out_images, int* out_n, void* stream) {
  if (!out_n || !offsets || n_blocks < 0 || topk < 1) return DRN_ERR_ARG;
  if (n_blocks > 0 && (!boxes || !scores || !classes || !count || !image_index || !out_boxes || !out_scores ||
                       !out_classes || !out_images))
    return DRN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(compact_offsets_kernel, dim3(1), dim3(1024), 0, st, count, n_blocks, topk, offsets, out_n);
  if (n_blocks > 0)
    hipLaunchKernelGGL(compact_gather_kernel, dim3(n_blocks), dim3(64), 0, st, boxes, scores, classes, image_index,
                       (const int*)offsets, topk, out_boxes, out_scores, out_classes, out_images);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_tta_accumulate(const float* boxes, const float* scores, float* acc_boxes, float* acc_scores, long n_boxes,
                       long n_scores, float sx, float sy, float flip_w, int first, int n_final, void* stream) {
  if (!boxes || !scores || !acc_boxes || !acc_scores || n_boxes < 0 || n_scores < 0) return DRN_ERR_ARG;
  const long n = n_boxes > n_scores ? n_boxes : n_scores;
  if (n == 0) return DRN_OK;
  hipLaunchKernelGGL(tta_accumulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, boxes,
                     scores, acc_boxes, acc_scores, n_boxes, n_scores, sx, sy, flip_w, first, n_final);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // extern "C"
