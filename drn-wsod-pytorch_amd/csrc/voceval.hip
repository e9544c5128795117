// PASCAL VOC detection evaluation for gfx950: AP (VOC07 11-point or area) and CorLoc on the device.  Pinned by
// evaluation.py's host path (voc_eval, voc_eval_corloc, voc_ap, _max_overlap, format_prediction), i.e. the reference's
// detectron2/evaluation/pascal_voc_evaluation.py.  Everything is integer counting plus single IEEE fp64 operations in
// the host's order (built with -ffp-contract=off), so on inputs without score ties the results are bit-identical to
// it; the area AP alone is a sum in another (fixed) order.  No float atomics; every reduction has a fixed order.
//
// drn_voc_match
//   rank stage    voc_key_kernel quantises the scores the way the reference's text files do (%.3f: rint(s * 1000) /
//                 1000 in fp64, exact for fp32 scores) and maps the fp64 value to a descending 64-bit key; six stable
//                 LSD radix passes over its two 32-bit halves, then one over the class (radix_sort.h, seg_sort.h)
//                 -> per class by descending quantised score, ties in input order; cls_off[K + 1]
//   match stage   voc_overlap_kernel, one thread per ranked detection: quantises the box (%.1f after the fp32 +1 of
//                 xmin / ymin) and takes ovmax / jmax over the GT of its (image, class) pair, _max_overlap operation
//                 for operation.  The rank positions are then stable-sorted by image, which groups them by pair (image,
//                 then class, then rank).  voc_walk_kernel, one wave per pair, lane t = IoU threshold t: walks the
//                 pair's detections in rank order with the per-GT `det` flags in two 64-bit registers per lane; one
//                 ballot of tp and one of fp give the detection's two result words.  The pair's CorLoc hit word comes
//                 from its first detection.
// drn_voc_accumulate
//   voc_ap_kernel, one wave per (class, threshold): scans the class's ranked segment 64 detections at a time, cumulative
//   tp / fp by ballot prefixes, rec / prec as the host computes them; VOC07: per recall threshold the largest precision
//   (a max: order-free), then the eleven sequential adds; area: a second, backward scan carrying the suffix maximum of
//   the precision (the monotone envelope), one term per recall step, summed per lane and then over the lanes in a fixed
//   tree.  CorLoc = set bits of the pairs' hit words / npos_im.
#include "drn_common.h"
#include "seg_sort.h"
#include "../../include/drn_wsod.h"

#include <float.h>

namespace {

typedef unsigned long long u64;

constexpr int MAX_GT = DRN_VOC_MAX_GT, MAX_REC = DRN_VOC_MAX_REC, GT_WORDS = MAX_GT / 64;
constexpr int WALK_WAVES = 4;

// format_prediction's "%.3f" read back with float(): s * 1000 is exact in fp64 for an fp32 s, rint rounds the exact
// value half-to-even like printf, and n / 1000.0 is the correctly rounded double of the decimal.  -0.0 becomes +0.0
// (the host compares them as equal).
__device__ __forceinline__ double quant_score(float s) {
  const double q = rint((double)s * 1000.0) / 1000.0;
  return q == 0.0 ? 0.0 : q;
}

__device__ __forceinline__ double quant_coord(float x) { return rint((double)x * 10.0) / 10.0; }

__device__ __forceinline__ int clamp_index(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

struct MatchParams {
  const float* det_box; const float* det_score; const int* det_pair; int n;
  const double* gt_box; const unsigned char* gt_diff; const int* gt_off;
  int P, K;
  const double* thr; int T;
  unsigned* key_hi; int* cls;                      // workspace, input order
  unsigned* r_key; int* r_val;                     // the sort buffer that holds the (class, score) order
  const int* p_val; const int* det_off;            // rank positions grouped by pair; det_off[P + 1]
  int* order; double* s_score; double* ovmax; int* jmax; u64* tp; u64* fp; u64* hit;
};

// descending 64-bit keys of the quantised scores: low half into the sort buffer (value = input index), high half aside
__global__ void voc_key_kernel(MatchParams p, unsigned* key_lo, int* val) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const u64 u = __builtin_bit_cast(u64, quant_score(p.det_score[i]));
  const u64 asc = u ^ ((u >> 63) ? ~0ULL : 0x8000000000000000ULL);  // ascending total order on the bits
  const u64 desc = ~asc;
  key_lo[i] = (unsigned)desc;
  val[i] = i;
  p.key_hi[i] = (unsigned)(desc >> 32);
  p.cls[i] = clamp_index(p.det_pair[i], p.P) % p.K;
}

__global__ void gather_hi_kernel(const unsigned* __restrict__ hi, const int* __restrict__ val,
                                 unsigned* __restrict__ key_out, int n) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) key_out[j] = hi[val[j]];
}

// per ranked detection r: its records, ovmax / jmax over its pair's GT, and the next sort's (key = image, value = r)
__global__ void voc_overlap_kernel(MatchParams p) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n) return;
  const int o = p.r_val[r];
  const int pair = clamp_index(p.det_pair[o], p.P);
  p.order[r] = o;
  p.s_score[r] = quant_score(p.det_score[o]);
  const float* B = p.det_box + (long)o * 4;
  const double b0 = quant_coord(B[0] + 1.0f), b1 = quant_coord(B[1] + 1.0f);  // the +1 is an fp32 add, like the host's
  const double b2 = quant_coord(B[2]), b3 = quant_coord(B[3]);
  const int g0 = p.gt_off[pair];
  int ng = p.gt_off[pair + 1] - g0;
  if (ng > MAX_GT || g0 < 0) ng = 0;  // (refused on the host before the launch)
  double best = -INFINITY;
  int jbest = -1;
  const double darea = (b2 - b0 + 1.0) * (b3 - b1 + 1.0);
  for (int g = 0; g < ng; ++g) {  // _max_overlap, operation for operation
    const double* Gb = p.gt_box + (long)(g0 + g) * 4;
    const double iw = fmax(fmin(Gb[2], b2) - fmax(Gb[0], b0) + 1.0, 0.0);
    const double ih = fmax(fmin(Gb[3], b3) - fmax(Gb[1], b1) + 1.0, 0.0);
    const double inters = iw * ih;
    const double uni = darea + (Gb[2] - Gb[0] + 1.0) * (Gb[3] - Gb[1] + 1.0) - inters;
    const double ov = inters / uni;
    if (g == 0 || ov > best) {  // np.argmax: the first index on equal maxima
      best = ov;
      jbest = g;
    }
  }
  p.ovmax[r] = best;
  p.jmax[r] = jbest;
  p.r_key[r] = (unsigned)(pair / p.K);
  p.r_val[r] = r;
}

__global__ void pair_key_kernel(MatchParams p, unsigned* key) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < p.n) key[j] = (unsigned)clamp_index(p.det_pair[p.order[p.p_val[j]]], p.P);
}

__global__ __launch_bounds__(64 * WALK_WAVES) void voc_walk_kernel(MatchParams p) {
  const int pair = blockIdx.x * WALK_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pair >= p.P) return;
  const int g0 = p.gt_off[pair], ng = p.gt_off[pair + 1] - g0;
  const int d0 = p.det_off[pair], nd = p.det_off[pair + 1] - d0;
  if (nd <= 0 || ng > MAX_GT || ng < 0 || g0 < 0) {
    if (lane == 0) p.hit[pair] = 0;
    return;
  }
  const bool active = lane < p.T;
  const double thr = p.thr[active ? lane : 0];
  bool easy = false;  // a GT that is not difficult: the pair counts for CorLoc
  for (int g = lane; g < ng; g += 64) easy |= p.gt_diff[g0 + g] == 0;
  const bool counts = __ballot(easy) != 0;
  u64 det[GT_WORDS];
#pragma unroll
  for (int w = 0; w < GT_WORDS; ++w) det[w] = 0;
  for (int d = 0; d < nd; ++d) {
    const int r = p.p_val[d0 + d];
    const double ov = p.ovmax[r];
    const int jm = p.jmax[r];
    bool tp = false, fp = false;
    if (active) {
      if (ov > thr && jm >= 0) {
        if (!p.gt_diff[g0 + jm]) {
          const u64 bit = 1ULL << (jm & 63);
          bool seen = false;
#pragma unroll
          for (int w = 0; w < GT_WORDS; ++w)
            if (w == (jm >> 6)) {
              seen = (det[w] & bit) != 0;
              det[w] |= bit;
            }
          tp = !seen;
          fp = seen;
        }
      } else {
        fp = true;
      }
    }
    const u64 btp = __ballot(tp), bfp = __ballot(fp);
    if (lane == 0) {
      p.tp[r] = btp;
      p.fp[r] = bfp;
    }
    if (d == 0) {  // the class's top-ranked detection in this image decides CorLoc
      const u64 bh = __ballot(active && counts && ov > thr);
      if (lane == 0) p.hit[pair] = bh;
    }
  }
}

// ---- accumulate ------------------------------------------------------------------------------------------------------

struct ApParams {
  const u64* tp; const u64* fp; const int* cls_off; const u64* hit; const int* npos; const int* npos_im;
  int I, K, T;
  const double* rec_thr; int R; int use_07; int t_curve;
  double* ap; double* corloc; double* rec_out; double* prec_out;
};

__global__ __launch_bounds__(64) void voc_ap_kernel(ApParams p) {
  const int lane = threadIdx.x, k = blockIdx.x / p.T, t = blockIdx.x % p.T;
  const int c0 = p.cls_off[k], c1 = p.cls_off[k + 1], np = p.npos[k];
  const u64 lt = (1ULL << lane) - 1ULL, le = lt | (1ULL << lane);
  const bool curve = p.rec_out && p.prec_out && t == p.t_curve;
  double rt[MAX_REC], pm[MAX_REC];
#pragma unroll
  for (int i = 0; i < MAX_REC; ++i) {
    rt[i] = i < p.R ? p.rec_thr[i] : 0.0;
    pm[i] = 0.0;
  }
  int tp = 0, fp = 0;
  for (int base = c0; base < c1; base += 64) {
    const int j = base + lane;
    const bool in = j < c1;
    const bool bt = in && ((p.tp[j] >> t) & 1ULL), bf = in && ((p.fp[j] >> t) & 1ULL);
    const u64 btp = __ballot(bt), bfp = __ballot(bf);
    if (in) {
      const double dtp = (double)(tp + __popcll(btp & le)), dfp = (double)(fp + __popcll(bfp & le));
      const double rec = np > 0 ? dtp / (double)np : 0.0;
      const double prec = dtp / fmax(dtp + dfp, DBL_EPSILON);
      if (curve) {
        p.rec_out[j] = rec;
        p.prec_out[j] = prec;
      }
#pragma unroll
      for (int i = 0; i < MAX_REC; ++i)
        if (i < p.R && rec >= rt[i]) pm[i] = fmax(pm[i], prec);
    }
    tp += __popcll(btp);
    fp += __popcll(bfp);
  }
  double ap = 0.0;
  if (p.use_07) {
    // voc_ap, VOC07: p = max of prec over rec >= t (0 if there is none), ap = ap + p / 11.0 in threshold order
#pragma unroll
    for (int i = 0; i < MAX_REC; ++i) {
      double v = pm[i];
      for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
      if (i < p.R) ap = ap + v / (double)p.R;
    }
  } else {
    // voc_ap, area: the envelope mpre[e] = max of prec from e on; one term (rec[e] - rec[e - 1]) * mpre[e] per recall
    // step, i.e. per tp.  The closing step to recall 1 multiplies the appended precision 0.
    double smax = 0.0, acc = 0.0;
    int tpe = tp, fpe = fp;
    const int nch = (c1 - c0 + 63) / 64;
    for (int ch = nch - 1; ch >= 0; --ch) {
      const int j = c0 + ch * 64 + lane;
      const bool in = j < c1;
      const bool bt = in && ((p.tp[j] >> t) & 1ULL), bf = in && ((p.fp[j] >> t) & 1ULL);
      const u64 btp = __ballot(bt), bfp = __ballot(bf);
      const int tp0 = tpe - __popcll(btp), fp0 = fpe - __popcll(bfp);
      const double dtp = (double)(tp0 + __popcll(btp & le)), dfp = (double)(fp0 + __popcll(bfp & le));
      double v = in ? dtp / fmax(dtp + dfp, DBL_EPSILON) : 0.0;
      for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_down(v, o, 64);
        if (lane + o < 64) v = fmax(v, u);
      }
      v = fmax(v, smax);
      if (bt && np > 0) acc += (dtp / (double)np - (dtp - 1.0) / (double)np) * v;
      smax = __shfl(v, 0, 64);
      tpe = tp0;
      fpe = fp0;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    ap = acc;
  }
  // CorLoc: hits / npos_im; 0 for a class without detections or without an image that counts (voc_eval_corloc)
  int hits = 0;
  for (int i = lane; i < p.I; i += 64) hits += (int)((p.hit[(long)i * p.K + k] >> t) & 1ULL);
  for (int o = 32; o > 0; o >>= 1) hits += __shfl_down(hits, o, 64);
  if (lane == 0) {
    const int ni = p.npos_im[k];
    p.ap[t * p.K + k] = ap;
    p.corloc[t * p.K + k] = (c1 > c0 && ni > 0) ? 1.0 * (double)hits / (double)ni : 0.0;
  }
}

}  // namespace

extern "C" {

int drn_voc_match(const float* det_box, const float* det_score, const int* det_pair, int n, const double* gt_box,
                  const unsigned char* gt_diff, const int* gt_off, int P, int K, int max_gt, const double* iou_thr, int T,
                  void* workspace, long workspace_bytes, int stages, int* order, double* s_score, int* cls_off,
                  double* ovmax, int* jmax, unsigned long long* tp, unsigned long long* fp, unsigned long long* hit,
                  void* stream) {
  if (n < 0 || P < 1 || K < 1 || P % K != 0 || T < 1 || max_gt < 0 || !gt_off || !iou_thr || !workspace || !cls_off ||
      !hit || (stages & ~3) || !(stages & 3))
    return DRN_ERR_ARG;
  if (n > 0 && (!det_box || !det_score || !det_pair || !order || !s_score || !ovmax || !jmax || !tp || !fp))
    return DRN_ERR_ARG;
  if (max_gt > 0 && (!gt_box || !gt_diff)) return DRN_ERR_ARG;
  if (((uintptr_t)workspace & 15) || workspace_bytes < DRN_VOC_WS_BYTES((long)n, (long)P)) return DRN_ERR_ARG;
  if (T > 64 || max_gt > MAX_GT) return DRN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Carve c{(char*)workspace, (char*)workspace + workspace_bytes};
  SortBufs b = carve_sort(c, n);
  const long m = n < 1 ? 1 : n;
  unsigned* key_hi = c.take<unsigned>(m);
  int* cls = c.take<int>(m);
  int* det_off = c.take<int>((long)P + 1);
  // the pass counts depend on K and P alone, so the buffers that hold the two orders are known without asking the device
  const int cur_rank = (6 + int_passes(K)) & 1, cur_pair = (cur_rank + int_passes(P / K)) & 1;
  MatchParams mp{det_box, det_score, det_pair, n, gt_box, gt_diff, gt_off, P, K, iou_thr, T, key_hi, cls,
                 b.key[cur_rank], b.val[cur_rank], b.val[cur_pair], det_off, order, s_score, ovmax, jmax, tp, fp, hit};
  const dim3 grid_n((n + 255) / 256), blk(256);
  if (stages & 1) {
    hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(1), 0, st, b.count, n);
    if (n > 0) hipLaunchKernelGGL(voc_key_kernel, grid_n, blk, 0, st, mp, b.key[0], b.val[0]);
    const int shifts[3] = {0, 11, 22}, bits[3] = {11, 11, 10};
    int at = 0;
    for (int half = 0; half < 2; ++half) {
      if (half == 1 && n > 0) hipLaunchKernelGGL(gather_hi_kernel, grid_n, blk, 0, st, key_hi, b.val[at], b.key[at], n);
      for (int ps = 0; ps < 3; ++ps) {
        sort_pass(b, at, nullptr, shifts[ps], bits[ps], st);
        at ^= 1;
      }
    }
    at = sort_by_int(b, at, cls, K, n, st);
    if (at != cur_rank) return DRN_ERR_LAUNCH;
    hipLaunchKernelGGL(seg_bounds_kernel, dim3(n / 256 + 1), blk, 0, st, b.key[cur_rank], n, K, cls_off);
  }
  if (stages & 2) {
    if (n > 0) hipLaunchKernelGGL(voc_overlap_kernel, grid_n, blk, 0, st, mp);
    const int at = sort_int_passes(b, cur_rank, P / K, st);
    if (at != cur_pair) return DRN_ERR_LAUNCH;
    if (n > 0) hipLaunchKernelGGL(pair_key_kernel, grid_n, blk, 0, st, mp, b.key[cur_pair]);
    hipLaunchKernelGGL(seg_bounds_kernel, dim3(n / 256 + 1), blk, 0, st, b.key[cur_pair], n, P, det_off);
    hipLaunchKernelGGL(voc_walk_kernel, dim3((P + WALK_WAVES - 1) / WALK_WAVES), dim3(64 * WALK_WAVES), 0, st, mp);
  }
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_voc_accumulate(const unsigned long long* tp, const unsigned long long* fp, int n, const int* cls_off,
                       const unsigned long long* hit, const int* npos, const int* npos_im, int I, int K, int T,
                       const double* rec_thr, int R, int use_07_metric, int t_curve, double* ap, double* corloc,
                       double* rec, double* prec, void* stream) {
  if (n < 0 || I < 1 || K < 1 || T < 1 || R < 0 || !cls_off || !hit || !npos || !npos_im || !ap || !corloc ||
      (use_07_metric && (!rec_thr || R < 1)) || (n > 0 && (!tp || !fp)) || (!rec != !prec))
    return DRN_ERR_ARG;
  if (T > 64 || R > MAX_REC) return DRN_ERR_UNSUPPORTED;
  ApParams ap_{tp, fp, cls_off, hit, npos, npos_im, I, K, T, rec_thr, use_07_metric ? R : 0, use_07_metric != 0, t_curve,
               ap, corloc, rec, prec};
  hipLaunchKernelGGL(voc_ap_kernel, dim3((unsigned)((long)K * T)), dim3(64), 0, (hipStream_t)stream, ap_);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // extern "C"
