// COCO box-AP evaluation for gfx950: per-(image, category) greedy matching and the precision / recall accumulation,
// both on the device.  Pinned by the reference's native component detectron2/layers/csrc/cocoeval/cocoeval.cpp
// (EvaluateImages :141-198 with its helpers :17-139, Accumulate :371-497 with BuildSortedDetectionList :222-272 and
// ComputePrecisionRecallCurve :283-370); the IoU is pycocotools' bbIou, which the reference tree does not hold and
// which is restated here.  Everything is integer counting plus single IEEE fp64 operations in the reference's order
// (built with -ffp-contract=off), so the results are bit-identical to the C++.
//
// drn_coco_match
//   order stage   stable LSD radix passes (radix_sort.h): by descending score, then by the (image, category) pair id
//                 -> detections grouped by pair, descending score inside, ties in input order (cocoeval.cpp:17-29);
//                 seg_bounds_kernel turns the sorted pair ids into det_off[P + 1]
//   match stage   coco_match_kernel, one wave per pair.  The pair's GT boxes sit in LDS; for every area range the GT is
//                 stable-partitioned not-ignored first (:33-56) by two ballot-prefix passes in original order.  Lane
//                 a * T + t owns (area range a, IoU threshold t): per detection the wave first computes the IoU row
//                 against every GT once into LDS (fp64), then each lane walks its partitioned GT list sequentially
//                 (:86-131).  Matched-GT flags are one 64-bit LDS word per GT, bit = lane.  One ballot of "matched"
//                 and one of "ignored" give the detection's two 64-bit result words, stored by lane 0.
// drn_coco_accumulate
//   order stage   by descending score, then by category: per category the list the reference builds image by image and
//                 stable-sorts (:222-272); the per-detection records are gathered into that order once
//   curve stage   coco_curve_kernel, one wave per (category, area range, maxDet, IoU threshold) scans its category's
//                 segment 64 detections at a time, counts tp / fp with ballot prefixes and keeps, per "number of recall
//                 thresholds reached" bucket, the largest precision and the first detection; the backward envelope and
//                 the lower_bound sampling (:345-369) are then one suffix walk over the <= 128 buckets.
#include "drn_common.h"
#include "seg_sort.h"
#include "../../include/drn_wsod.h"

namespace {

typedef unsigned long long u64;

constexpr int MAX_GT = DRN_COCO_MAX_GT, MAX_AREAS = DRN_COCO_MAX_AREAS, MAX_REC = DRN_COCO_MAX_REC;

__global__ void fill_f64_kernel(double* p, long n, double v) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// stable descending by score (value = input index); returns the buffer that holds the result
int sort_by_score(const SortBufs& b, const float* score, hipStream_t st) {
  const int shifts[3] = {0, 11, 22}, bits[3] = {11, 11, 10};
  int cur = 0;
  for (int ps = 0; ps < 3; ++ps) {
    sort_pass(b, cur, ps == 0 ? score : nullptr, shifts[ps], bits[ps], st);
    cur ^= 1;
  }
  return cur;
}

// ---- match ---------------------------------------------------------------------------------------------------------

struct MatchParams {
  const double* det_box; const float* det_score; const int* det_pair; int n;
  const double* gt_box; const double* gt_area; const unsigned char* gt_crowd; const int* gt_off;
  int P, K;
  const double* iou_thr; int T;
  const double* area_rng; int A;
  int max_det;
  const unsigned* s_key; const int* s_val; const int* det_off;
  int* order; float* s_score; int* s_cat; int* s_rank;
  u64* dm; u64* di; int* npig; unsigned char* gt_ign;
};

// the sorted detections' records: input index, score, category, rank inside the pair
__global__ void match_finish_order_kernel(MatchParams p) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p.n) return;
  const int o = p.s_val[j], pair = (int)p.s_key[j];
  p.order[j] = o;
  p.s_score[j] = p.det_score[o];
  p.s_cat[j] = pair % p.K;
  p.s_rank[j] = j - p.det_off[pair];
}

__device__ __forceinline__ bool area_ignored(double area, bool crowd, double lo, double hi) {
  return crowd || area < lo || area > hi;  // cocoeval.cpp:41-42 (inclusive bounds)
}

__global__ __launch_bounds__(64) void coco_match_kernel(MatchParams p) {
  __shared__ double gbox[MAX_GT][4];
  __shared__ double giou[MAX_GT];
  __shared__ u64 gmatched[MAX_GT];
  __shared__ unsigned short gord[MAX_AREAS][MAX_GT];
  __shared__ unsigned char gcrowd[MAX_GT];
  __shared__ int s_npig[MAX_AREAS];

  const int pair = blockIdx.x, lane = threadIdx.x;
  const int g0 = p.gt_off[pair], ng = p.gt_off[pair + 1] - g0;
  const int d0 = p.det_off[pair], nd = p.det_off[pair + 1] - d0;
  if (ng > MAX_GT || ng < 0 || g0 < 0) return;  // (refused on the host before the launch)
  if (ng == 0 && nd == 0) {
    if (lane < p.A) p.npig[(long)pair * p.A + lane] = 0;
    return;
  }
  const u64 lt = (1ULL << lane) - 1ULL;

  for (int g = lane; g < ng; g += 64) {
#pragma unroll
    for (int e = 0; e < 4; ++e) gbox[g][e] = p.gt_box[(long)(g0 + g) * 4 + e];
    gcrowd[g] = p.gt_crowd[g0 + g];
    gmatched[g] = 0;
    unsigned bits = 0;
    for (int a = 0; a < p.A; ++a)
      bits |= (unsigned)area_ignored(p.gt_area[g0 + g], gcrowd[g] != 0, p.area_rng[2 * a], p.area_rng[2 * a + 1]) << a;
    p.gt_ign[g0 + g] = (unsigned char)bits;
  }
  // stable partition per area range, not-ignored first (cocoeval.cpp:33-56): two passes in original order
  for (int a = 0; a < p.A; ++a) {
    const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];
    int base = 0;
    for (int pass = 0; pass < 2; ++pass)
      for (int c = 0; c < ng; c += 64) {
        const int g = c + lane;
        const bool in = g < ng;
        const bool ign = in && area_ignored(p.gt_area[g0 + (in ? g : 0)], p.gt_crowd[g0 + (in ? g : 0)] != 0, lo, hi);
        const bool mine = in && (ign == (pass == 1));
        const u64 m = __ballot(mine);
        if (mine) gord[a][base + __popcll(m & lt)] = (unsigned short)g;
        base += __popcll(m);
        if (pass == 0 && c + 64 >= ng && lane == 0) s_npig[a] = base;
      }
    if (ng == 0 && lane == 0) s_npig[a] = 0;
  }
  __syncthreads();
  if (lane < p.A) p.npig[(long)pair * p.A + lane] = s_npig[lane];
  if (nd == 0) return;

  const int AT = p.A * p.T;
  const bool active = lane < AT;
  const int a = active ? lane / p.T : 0, t = active ? lane % p.T : 0;
  const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];
  const double thr0 = fmin(p.iou_thr[t], 1 - 1e-10);  // cocoeval.cpp:89
  const int my_npig = s_npig[a];
  const int nkeep = nd < p.max_det ? nd : p.max_det;  // :171-173

  for (int d = 0; d < nkeep; ++d) {
    const double* D = p.det_box + (long)p.order[d0 + d] * 4;
    const double dx = D[0], dy = D[1], dw = D[2], dh = D[3];
    const double da = dw * dh;
    // pycocotools bbIou (maskApi.c), operation for operation
    for (int g = lane; g < ng; g += 64) {
      const double gx = gbox[g][0], gy = gbox[g][1], gw = gbox[g][2], gh = gbox[g][3];
      const double ga = gw * gh;
      double o = 0;
      const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
      if (w > 0) {
        const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
        if (h > 0) {
          const double i = w * h;
          const double u = gcrowd[g] ? da : da + ga - i;
          o = i / u;
        }
      }
      giou[g] = o;
    }
    __syncthreads();
    bool matched = false, ignored = false;
    if (active) {
      double best = thr0;
      int match = -1;
      for (int pos = 0; pos < ng; ++pos) {
        const int g = gord[a][pos];
        if (((gmatched[g] >> lane) & 1ULL) && !gcrowd[g]) continue;         // :94-97
        if (match >= 0 && match < my_npig && pos >= my_npig) break;        // :102-105
        if (giou[g] >= best) {                                              // :108-111
          best = giou[g];
          match = pos;
        }
      }
      if (match >= 0) {
        matched = true;
        ignored = match >= my_npig;                                         // :116
        atomicOr(&gmatched[gord[a][match]], 1ULL << lane);
      } else {
        ignored = da < lo || da > hi;                                       // :126-129
      }
    }
    const u64 bm = __ballot(matched), bi = __ballot(ignored);
    if (lane == 0) {
      p.dm[d0 + d] = bm;
      p.di[d0 + d] = bi;
    }
    __syncthreads();
  }
  for (int d = nkeep + lane; d < nd; d += 64) {  // beyond maxDets[-1]: dropped (rank >= max_det never counts)
    p.dm[d0 + d] = 0;
    p.di[d0 + d] = 0;
  }
}

// ---- accumulate ------------------------------------------------------------------------------------------------------

struct CurveParams {
  const float* s_score; const int* s_cat; const int* s_rank; const u64* dm; const u64* di; int n;
  const int* npig; int I, K, T, A;
  const int* max_dets; int M;
  const double* rec_thr; int R;
  const int* c_val; const int* cat_off;
  float* c_score; int* c_rank; u64* c_dm; u64* c_di; int* npig_k;
  double* precision; double* scores; double* recall;
};

__global__ void curve_gather_kernel(CurveParams p) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p.n) return;
  const int o = p.c_val[j];
  p.c_score[j] = p.s_score[o];
  p.c_rank[j] = p.s_rank[o];
  p.c_dm[j] = p.dm[o];
  p.c_di[j] = p.di[o];
}

// npig_k[k][a] = sum over images of npig[i * K + k][a]  (cocoeval.cpp:252-256)
__global__ void npig_sum_kernel(CurveParams p) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.K * p.A) return;
  const int k = q / p.A, a = q % p.A;
  int s = 0;
  for (int i = 0; i < p.I; ++i) s += p.npig[((long)i * p.K + k) * p.A + a];
  p.npig_k[q] = s;
}

__global__ __launch_bounds__(64) void coco_curve_kernel(CurveParams p) {
  __shared__ u64 bmax[MAX_REC + 1];    // bucket b: detections whose recall reaches exactly b thresholds: max precision (bits)
  __shared__ u64 bfirst[MAX_REC + 1];  // ... and the first of them: (list index << 32) | score bits
  __shared__ double rthr[MAX_REC];
  const int lane = threadIdx.x;
  int b = blockIdx.x;
  const int t = b % p.T; b /= p.T;
  const int m = b % p.M; b /= p.M;
  const int a = b % p.A;
  const int k = b / p.A;
  const int np = p.npig_k[k * p.A + a];
  if (np == 0) return;  // cocoeval.cpp:433-435: the entries stay -1
  const int md = p.max_dets[m], bit = a * p.T + t;
  for (int r = lane; r <= p.R; r += 64) {
    bmax[r] = 0;
    bfirst[r] = ~0ULL;
    if (r < p.R) rthr[r] = p.rec_thr[r];
  }
  __syncthreads();
  const u64 lt = (1ULL << lane) - 1ULL, le = lt | (1ULL << lane);
  const int c0 = p.cat_off[k], c1 = p.cat_off[k + 1];
  int tp = 0, fp = 0, idx = 0;
  for (int base = c0; base < c1; base += 64) {
    const int j = base + lane;
    const bool inl = j < c1 && p.c_rank[j] < md;  // :245-251
    bool ig = true, mt = false;
    unsigned sbits = 0;
    if (inl) {
      ig = (p.c_di[j] >> bit) & 1ULL;
      mt = (p.c_dm[j] >> bit) & 1ULL;
      sbits = __builtin_bit_cast(unsigned, p.c_score[j]);
    }
    const u64 btp = __ballot(inl && !ig && mt), bfp = __ballot(inl && !ig && !mt), bin = __ballot(inl);  // :323-324
    if (inl) {
      const int mytp = tp + __popcll(btp & le), myfp = fp + __popcll(bfp & le), myidx = idx + __popcll(bin & lt);
      const double rc = (double)mytp / (double)np;                       // :332-333
      const int nv = mytp + myfp;
      const double pr = nv > 0 ? (double)mytp / (double)nv : 0.0;          // :335-339
      int lo_ = 0, hi_ = p.R;  // number of thresholds <= rc
      while (lo_ < hi_) {
        const int mid = (lo_ + hi_) >> 1;
        if (rthr[mid] <= rc) lo_ = mid + 1; else hi_ = mid;
      }
      atomicMax(&bmax[lo_], __builtin_bit_cast(u64, pr));  // pr >= 0: its bit pattern orders like its value
      atomicMin(&bfirst[lo_], ((u64)(unsigned)myidx << 32) | sbits);
    }
    tp += __popcll(btp);
    fp += __popcll(bfp);
    idx += __popcll(bin);
  }
  __syncthreads();
  const long KAM = (long)p.K * p.A * p.M, kam = ((long)k * p.A + a) * p.M + m;
  if (lane == 0) p.recall[(long)t * KAM + kam] = (double)tp / (double)np;  // :343 (0 for an empty list)
  // P[r] = max precision over detections whose recall reaches threshold r (:345-349 + lower_bound :354-356)
  for (int r = lane; r < p.R; r += 64) {
    u64 mx = 0, first = ~0ULL;
    for (int q = p.R; q > r; --q) {
      if (bmax[q] > mx) mx = bmax[q];
      if (bfirst[q] != ~0ULL) first = bfirst[q];
    }
    double pv = 0, sv = 0;  // :365-368
    if (first != ~0ULL) {
      pv = __builtin_bit_cast(double, mx);
      sv = (double)__builtin_bit_cast(float, (unsigned)(first & 0xFFFFFFFFULL));
    }
    const long o = ((long)t * p.R + r) * KAM + kam;
    p.precision[o] = pv;
    p.scores[o] = sv;
  }
}

}  // namespace

extern "C" {

int drn_coco_match(const double* det_box, const float* det_score, const int* det_pair, int n, const double* gt_box,
                   const double* gt_area, const unsigned char* gt_crowd, const int* gt_off, int P, int K, int max_gt,
                   const double* iou_thr, int T, const double* area_rng, int A, int max_det, void* workspace,
                   long workspace_bytes, int stages, int* order, float* s_score, int* s_cat, int* s_rank,
                   unsigned long long* dm, unsigned long long* di, int* npig, unsigned char* gt_ign, void* stream) {
  if (n < 0 || P < 1 || K < 1 || P % K != 0 || T < 1 || A < 1 || max_det < 1 || max_gt < 0 || !gt_off || !iou_thr ||
      !area_rng || !workspace || !npig || (stages & ~3) || !(stages & 3))
    return DRN_ERR_ARG;
  if (n > 0 && (!det_box || !det_score || !det_pair || !order || !s_score || !s_cat || !s_rank || !dm || !di))
    return DRN_ERR_ARG;
  if (max_gt > 0 && (!gt_box || !gt_area || !gt_crowd || !gt_ign)) return DRN_ERR_ARG;
  if (((uintptr_t)workspace & 15) || workspace_bytes < DRN_COCO_WS_BYTES((long)n, (long)P)) return DRN_ERR_ARG;
  if (A > MAX_AREAS || A * T > 64 || max_gt > MAX_GT) return DRN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Carve c{(char*)workspace, (char*)workspace + workspace_bytes};
  SortBufs b = carve_sort(c, n);
  int* det_off = c.take<int>((long)P + 1);
  // the pass count depends on P alone, so the final buffer is known without asking the device
  int nbits = 1;
  while (nbits < 31 && (1L << nbits) < P) ++nbits;
  const int cur = (3 + (nbits + 10) / 11) & 1;
  MatchParams mp{det_box, det_score, det_pair, n, gt_box, gt_area, gt_crowd, gt_off, P, K, iou_thr, T, area_rng, A, max_det,
                 b.key[cur], b.val[cur], det_off, order, s_score, s_cat, s_rank, dm, di, npig, gt_ign};
  if (stages & 1) {
    hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(1), 0, st, b.count, n);
    int at = sort_by_score(b, det_score, st);
    at = sort_by_int(b, at, det_pair, P, n, st);
    if (at != cur) return DRN_ERR_LAUNCH;
    hipLaunchKernelGGL(seg_bounds_kernel, dim3(n / 256 + 1), dim3(256), 0, st, b.key[cur], n, P, det_off);
    if (n > 0) hipLaunchKernelGGL(match_finish_order_kernel, dim3((n + 255) / 256), dim3(256), 0, st, mp);
  }
  if (stages & 2) hipLaunchKernelGGL(coco_match_kernel, dim3(P), dim3(64), 0, st, mp);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_coco_accumulate(const float* s_score, const int* s_cat, const int* s_rank, const unsigned long long* dm,
                        const unsigned long long* di, int n, const int* npig, int I, int K, int T, int A,
                        const int* max_dets, int M, const double* rec_thr, int R, void* workspace, long workspace_bytes,
                        int stages, double* precision, double* scores, double* recall, void* stream) {
  if (n < 0 || I < 1 || K < 1 || T < 1 || A < 1 || M < 1 || R < 1 || !npig || !max_dets || !rec_thr || !workspace ||
      !precision || !scores || !recall || (stages & ~3) || !(stages & 3))
    return DRN_ERR_ARG;
  if (n > 0 && (!s_score || !s_cat || !s_rank || !dm || !di)) return DRN_ERR_ARG;
  if (((uintptr_t)workspace & 15) || workspace_bytes < DRN_COCO_WS_BYTES((long)n, (long)K)) return DRN_ERR_ARG;
  if (A > MAX_AREAS || A * T > 64 || R > MAX_REC) return DRN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Carve c{(char*)workspace, (char*)workspace + workspace_bytes};
  SortBufs b = carve_sort(c, n);
  const long m = n < 1 ? 1 : n;
  u64* c_dm = c.take<u64>(m);
  u64* c_di = c.take<u64>(m);
  float* c_score = c.take<float>(m);
  int* c_rank = c.take<int>(m);
  int* cat_off = c.take<int>((long)K + 1);
  int* npig_k = c.take<int>((long)K * A);
  int nbits = 1;
  while (nbits < 31 && (1L << nbits) < K) ++nbits;
  const int cur = (3 + (nbits + 10) / 11) & 1;
  CurveParams cp{s_score, s_cat, s_rank, dm, di, n, npig, I, K, T, A, max_dets, M, rec_thr, R, b.val[cur], cat_off,
                 c_score, c_rank, c_dm, c_di, npig_k, precision, scores, recall};
  if (stages & 1) {
    hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(1), 0, st, b.count, n);
    int at = sort_by_score(b, s_score, st);
    at = sort_by_int(b, at, s_cat, K, n, st);
    if (at != cur) return DRN_ERR_LAUNCH;
    hipLaunchKernelGGL(seg_bounds_kernel, dim3(n / 256 + 1), dim3(256), 0, st, b.key[cur], n, K, cat_off);
    if (n > 0) hipLaunchKernelGGL(curve_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, st, cp);
    hipLaunchKernelGGL(npig_sum_kernel, dim3((K * A + 255) / 256), dim3(256), 0, st, cp);
  }
  if (stages & 2) {
    const long np_ = (long)T * R * K * A * M, nr_ = (long)T * K * A * M;
    hipLaunchKernelGGL(fill_f64_kernel, dim3((unsigned)((np_ + 255) / 256)), dim3(256), 0, st, precision, np_, -1.0);
    hipLaunchKernelGGL(fill_f64_kernel, dim3((unsigned)((np_ + 255) / 256)), dim3(256), 0, st, scores, np_, -1.0);
    hipLaunchKernelGGL(fill_f64_kernel, dim3((unsigned)((nr_ + 255) / 256)), dim3(256), 0, st, recall, nr_, -1.0);
    hipLaunchKernelGGL(coco_curve_kernel, dim3((unsigned)((long)K * A * M * T)), dim3(64), 0, st, cp);
  }
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // extern "C"
