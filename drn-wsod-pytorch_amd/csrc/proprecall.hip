// Box-proposal recall (AR@k by area) for gfx950: the greedy proposal <-> ground-truth matching of the reference's
// _evaluate_box_proposals (detectron2/evaluation/coco_evaluation.py:372-480) for every (image, area range, limit) triple
// in one launch.  The IoU is pairwise_iou in float32 in torch's operation order (box_shared.h pair_iou, built with
// -ffp-contract=off), everything else is comparing and counting, so the recorded overlaps are bit-identical to the
// reference's and do not change from run to run.
//
// drn_proposal_recall
//   order stage   stable LSD radix passes (radix_sort.h): by descending objectness logit, then by image index ->
//                 every image's proposals in descending order, equal logits in input order.  The input is grouped by image,
//                 so the sorted segments are the input's (prop_off).  The boxes are gathered into that order once.
//   match stage   recall_match_kernel, one workgroup per (image, area range, limit).  The image's boxes inside the area
//                 range sit in LDS in annotation order, each with a cached (best IoU, best proposal) pair over the proposals
//                 not yet retired; one bit per proposal says "retired".  First pass: one box per wave, lanes stride over the
//                 proposals.  Round j (:441-456): reduce over the live boxes (largest cached IoU, lowest box index on ties),
//                 record it as entry j, retire the box and its proposal, recompute the boxes whose cached proposal was the
//                 retired one (IoUs are recomputed, never stored: [P', G'] does not fit the LDS).  "Lowest index wins" holds
//                 for the proposals because a lane walks its proposals upwards and takes only a strictly larger IoU, and
//                 the wave reduction prefers the lower index on equal IoUs - what torch.max does on the CPU.
//                 Counts and num_pos are integer atomics onto zeroed words: order-free.
#include "drn_common.h"
#include "seg_sort.h"
#include "box_shared.h"
#include "../../include/drn_wsod.h"

namespace {

typedef unsigned long long u64;

constexpr int MAX_GT = DRN_PROPOSAL_MAX_GT, MAX_PROP = DRN_PROPOSAL_MAX_PER_IMAGE, THREADS = 256, WAVES = THREADS / 64;
static_assert(MAX_GT == THREADS, "one thread per box in the reductions");

__global__ void fill_f32_kernel(float* p, long n, float v) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

__global__ void zero_u64_kernel(u64* a, int na, u64* b, int nb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < na) a[i] = 0;
  if (i < nb) b[i] = 0;
}

// img[j] = the image whose segment [off[i], off[i + 1]) holds j (off ascending; empty segments are skipped)
__global__ void prop_image_kernel(const int* __restrict__ off, int I, int n, int* __restrict__ img) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int lo = 0, hi = I;  // the last i in [0, I) with off[i] <= j
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= j) lo = mid; else hi = mid;
  }
  img[j] = lo;
}

__global__ void gather_box_kernel(const float4* __restrict__ box, const int* __restrict__ val, int n, float4* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned o = (unsigned)val[j];
  out[j] = box[o < (unsigned)n ? o : 0];
}

struct RecallParams {
  const float4* sbox; const int* prop_off; int P;
  const float* gt_box; const float* gt_area; const int* gt_off; int G, I;
  const float* area_rng; int A;
  const int* limits; int L;
  const float* thr; int T;
  float* overlaps; u64* counts; u64* num_pos;
};

// (a, ai) <- the better of (a, ai) and (b, bi): the larger IoU, the lower index on equal IoUs
__device__ __forceinline__ void take_better(float& a, int& ai, float b, int bi) {
  if (b > a || (b == a && bi < ai)) { a = b; ai = bi; }
}

__device__ __forceinline__ void wave_best(float& v, int& vi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float b = __shfl_xor(v, o, 64);
    const int bi = __shfl_xor(vi, o, 64);
    take_better(v, vi, b, bi);
  }
}

// one wave: the best proposal among the first np of `sbox` that is not retired, for the box g (corners + corner area)
__device__ __forceinline__ void best_proposal(const float4* __restrict__ sbox, int np, const unsigned* used, const float* g,
                                              float garea, int lane, float& best, int& at) {
  best = -1.f;  // every IoU is >= 0
  at = 0x7fffffff;
  for (int q = lane; q < np; q += 64) {
    if ((used[q >> 5] >> (q & 31)) & 1u) continue;
    const float4 b = sbox[q];
    const float iou = drn_box::pair_iou(g[0], g[1], g[2], g[3], garea, b.x, b.y, b.z, b.w, (b.z - b.x) * (b.w - b.y));
    if (iou > best) { best = iou; at = q; }
  }
  wave_best(best, at);
}

__global__ __launch_bounds__(THREADS) void recall_match_kernel(RecallParams p) {
  __shared__ float gb[MAX_GT][4];
  __shared__ float garea[MAX_GT];       // the corner area pairwise_iou uses (not the annotation's)
  __shared__ float biou[MAX_GT];
  __shared__ int bidx[MAX_GT];
  __shared__ float ent[MAX_GT];
  __shared__ unsigned char retired[MAX_GT];
  __shared__ unsigned used[MAX_PROP / 32];
  __shared__ int wcnt[WAVES];
  __shared__ float r_iou[WAVES];
  __shared__ int r_g[WAVES];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int b = blockIdx.x;
  const int l = b % p.L; b /= p.L;
  const int a = b % p.A;
  const int i = b / p.A;
  const int g0 = p.gt_off[i], ng = p.gt_off[i + 1] - g0;
  const int p0 = p.prop_off[i], np_all = p.prop_off[i + 1] - p0;
  // (refused on the host before the launch; nothing is read or written out of bounds whatever the tables hold)
  if (g0 < 0 || ng < 0 || ng > MAX_GT || (long)g0 + ng > p.G || p0 < 0 || np_all < 0 || (long)p0 + np_all > p.P) return;
  float* out = p.overlaps + ((long)a * p.L + l) * p.G + g0;
  if (ng == 0 || np_all == 0) {  // :424-425: the image is skipped before anything is counted
    if (tid < ng) out[tid] = -1.f;
    return;
  }
  const int lim = p.limits[l];
  int np = lim > 0 && lim < np_all ? lim : np_all;  // :435-436
  if (np > MAX_PROP) np = MAX_PROP;
  const float4* sbox = p.sbox + p0;

  // the boxes inside the area range (:427-428, both ends inclusive, fp32), compacted in annotation order
  const float lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];
  bool in = false;
  if (tid < ng) {
    const float ar = p.gt_area[g0 + tid];
    in = ar >= lo && ar <= hi;
  }
  const u64 m = __ballot(in);
  if (lane == 0) wcnt[w] = __popcll(m);
  for (int q = tid; q < MAX_PROP / 32; q += THREADS) used[q] = 0;
  __syncthreads();
  int pos = __popcll(m & ((1ULL << lane) - 1ULL)), gn = 0;
#pragma unroll
  for (int q = 0; q < WAVES; ++q) {
    if (q < w) pos += wcnt[q];
    gn += wcnt[q];
  }
  if (in) {
    const float* s = p.gt_box + (long)(g0 + tid) * 4;
    const float x1 = s[0], y1 = s[1], x2 = s[2], y2 = s[3];
    gb[pos][0] = x1; gb[pos][1] = y1; gb[pos][2] = x2; gb[pos][3] = y2;
    garea[pos] = (x2 - x1) * (y2 - y1);
  }
  ent[tid] = 0.f;  // entries past min(P', G') stay 0 (:440)
  retired[tid] = 0;
  if (l == 0 && tid == 0) atomicAdd(&p.num_pos[a], (u64)gn);  // :430, before the cut and whatever gn is
  __syncthreads();

  const int rounds = np < gn ? np : gn;
  if (rounds > 0) {
    for (int g = w; g < gn; g += WAVES) {
      float v;
      int at;
      best_proposal(sbox, np, used, gb[g], garea[g], lane, v, at);
      if (lane == 0) { biou[g] = v; bidx[g] = at; }
    }
    __syncthreads();
  }
  for (int j = 0; j < rounds; ++j) {
    // the best-covered live box (:447), lowest index on equal IoUs
    float v = tid < gn && !retired[tid] ? biou[tid] : -2.f;
    int vg = tid;
    wave_best(v, vg);
    if (lane == 0) { r_iou[w] = v; r_g[w] = vg; }
    __syncthreads();
    v = r_iou[0];
    vg = r_g[0];
#pragma unroll
    for (int q = 1; q < WAVES; ++q) take_better(v, vg, r_iou[q], r_g[q]);
    const int pj = bidx[vg];
    __syncthreads();
    if (tid == 0) {
      ent[j] = v;  // :452
      retired[vg] = 1;  // :455-456
      if ((unsigned)pj < (unsigned)np) used[pj >> 5] |= 1u << (pj & 31);
    }
    __syncthreads();
    if (j + 1 < rounds) {
      for (int g = w; g < gn; g += WAVES) {
        if (retired[g] || bidx[g] != pj) continue;  // (wave-uniform)
        float nv;
        int at;
        best_proposal(sbox, np, used, gb[g], garea[g], lane, nv, at);
        if (lane == 0) { biou[g] = nv; bidx[g] = at; }
      }
      __syncthreads();
    }
  }
  if (tid < ng) out[tid] = tid < gn ? ent[tid] : -1.f;
  for (int t = tid; t < p.T; t += THREADS) {  // :471, as integers
    const float th = p.thr[t];
    int c = 0;
    for (int g = 0; g < gn; ++g) c += ent[g] >= th;
    if (c) atomicAdd(&p.counts[((long)a * p.L + l) * p.T + t], (u64)c);
  }
}

}  // namespace

extern "C" {

long drn_proposal_recall_workspace_bytes(int P) {
  const long n = P < 0 ? 0 : P;
  return 40L * (n + 4) + 8192L * ((n + 4095) / 4096 + 1) + 1024L;
}

int drn_proposal_recall(const float* prop_box, const float* prop_logit, const int* prop_off, int P, const float* gt_box,
                        const float* gt_area, const int* gt_off, int G, int I, int max_gt, int max_prop,
                        const float* area_rng, int A, const int* limits, int L, const float* thresholds, int T,
                        void* workspace, long workspace_bytes, int stages, float* overlaps, unsigned long long* counts,
                        unsigned long long* num_pos, void* stream) {
  if (P < 0 || G < 0 || I < 1 || A < 1 || L < 1 || T < 1 || max_gt < 0 || max_prop < 0 || !prop_off || !gt_off || !area_rng ||
      !limits || !thresholds || !workspace || !counts || !num_pos || (stages & ~3) || !(stages & 3))
    return DRN_ERR_ARG;
  if (P > 0 && (!prop_box || !prop_logit)) return DRN_ERR_ARG;
  if (G > 0 && (!gt_box || !gt_area || !overlaps)) return DRN_ERR_ARG;
  if (((uintptr_t)workspace & 15) || workspace_bytes < drn_proposal_recall_workspace_bytes(P)) return DRN_ERR_ARG;
  if (((uintptr_t)prop_box & 15)) return DRN_ERR_ARG;  // rows are read as float4
  if (max_gt > MAX_GT || max_prop > MAX_PROP || (long)I * A * L > 0x7fffffffL || (long)A * L * T > 0x7fffffffL)
    return DRN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Carve c{(char*)workspace, (char*)workspace + workspace_bytes};
  SortBufs b = carve_sort(c, P);
  const long m = P < 1 ? 1 : P;
  int* img = c.take<int>(m);
  float4* sbox = c.take<float4>(m);
  // the pass count depends on I alone, so the final buffer is known without asking the device
  const int cur = (3 + int_passes(I)) & 1;
  if ((stages & 1) && P > 0) {
    hipLaunchKernelGGL(set_int_kernel, dim3(1), dim3(1), 0, st, b.count, P);
    hipLaunchKernelGGL(prop_image_kernel, dim3((P + 255) / 256), dim3(256), 0, st, prop_off, I, P, img);
    const int shifts[3] = {0, 11, 22}, bits[3] = {11, 11, 10};
    int at = 0;
    for (int ps = 0; ps < 3; ++ps) {  // stable descending by logit (value = input index)
      sort_pass(b, at, ps == 0 ? prop_logit : nullptr, shifts[ps], bits[ps], st);
      at ^= 1;
    }
    at = sort_by_int(b, at, img, I, P, st);
    if (at != cur) return DRN_ERR_LAUNCH;
    hipLaunchKernelGGL(gather_box_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (const float4*)prop_box, b.val[cur], P,
                       sbox);
  }
  if (stages & 2) {
    const long no = (long)A * L * G;
    if (no > 0)
      hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, st, overlaps, no, -1.f);
    const int nc = A * L * T;
    hipLaunchKernelGGL(zero_u64_kernel, dim3(((nc > A ? nc : A) + 255) / 256), dim3(256), 0, st, counts, nc, num_pos, A);
    RecallParams rp{sbox, prop_off, P, gt_box, gt_area, gt_off, G, I, area_rng, A, limits, L, thresholds, T, overlaps,
                    counts, num_pos};
    hipLaunchKernelGGL(recall_match_kernel, dim3((unsigned)((long)I * A * L)), dim3(THREADS), 0, st, rp);
  }
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // extern "C"
