// Pairwise IoU and Matcher as stand-alone device ops for gfx950.  The IoU is box_shared.h's pair_iou - the arithmetic the annotated-box
// labelling and the proposal-recall matching already run inside their own kernels - so the matrix is bit-equal to what they see
// (built with -ffp-contract=off).
#include "box_shared.h"

namespace {

// detectron2/structures/boxes.py:329-361: one thread per (i, j), j fastest (the output is the traffic: N * M coalesced stores)
__global__ __launch_bounds__(256) void pairwise_iou_kernel(const float* __restrict__ a, const float* __restrict__ b, long N, long M,
                                                           float* __restrict__ out) {
  const long idx = blockIdx.x * 256L + threadIdx.x;
  if (idx >= N * M) return;
  const long i = idx / M, j = idx - i * M;
  const float ax1 = a[4 * i], ay1 = a[4 * i + 1], ax2 = a[4 * i + 2], ay2 = a[4 * i + 3];
  const float bx1 = b[4 * j], by1 = b[4 * j + 1], bx2 = b[4 * j + 2], by2 = b[4 * j + 3];
  out[idx] = drn_box::pair_iou(ax1, ay1, ax2, ay2, (ax2 - ax1) * (ay2 - ay1), bx1, by1, bx2, by2, (bx2 - bx1) * (by2 - by1));
}

// detectron2/modeling/matcher.py:61-103 without low-quality matches: one thread per column, rows walked in order (neighbouring threads
// read neighbouring words of a row); the first row wins a tie, as torch.max does on the CPU
__global__ __launch_bounds__(256) void match_kernel(const float* __restrict__ q, long N, long M, drn_box::MatcherArgs a,
                                                    long long* __restrict__ matches, signed char* __restrict__ match_labels) {
  const long j = blockIdx.x * 256L + threadIdx.x;
  if (j >= M) return;
  if (N == 0) {  // matcher.py:75-85: no ground truth - matched 0, the lowest interval's label
    matches[j] = 0;
    match_labels[j] = (signed char)a.lab[0];
    return;
  }
  float best = q[j];
  long bi = 0;
  for (long i = 1; i < N; ++i) {
    const float v = q[i * M + j];
    if (v > best) { best = v; bi = i; }
  }
  int ml = 1;
  for (int t = 0; t <= a.nthr; ++t) {
    const float lo = t == 0 ? -INFINITY : a.thr[t - 1];
    const float hi = t == a.nthr ? INFINITY : a.thr[t];
    if (best >= lo && best < hi) ml = a.lab[t];
  }
  matches[j] = bi;
  match_labels[j] = (signed char)ml;
}

}  // namespace

extern "C" {

int drn_pairwise_iou(const float* a, const float* b, long N, long M, float* out, void* stream) {
  if (N < 0 || M < 0) return DRN_ERR_ARG;
  if (N == 0 || M == 0) return DRN_OK;
  if (!a || !b || !out) return DRN_ERR_ARG;
  const long blocks = (N * M + 255) / 256;
  if (blocks > 0x7fffffffL) return DRN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pairwise_iou_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, N, M, out);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_match(const float* quality, long N, long M, const float* thresholds, int n_thr, const int* labels, long long* matches,
              signed char* match_labels, void* stream) {
  if (N < 0 || M < 0 || n_thr < 0 || !labels || (n_thr > 0 && !thresholds)) return DRN_ERR_ARG;
  if (n_thr > 3) return DRN_ERR_UNSUPPORTED;
  drn_box::MatcherArgs a;
  if (!drn_box::matcher_args(thresholds, labels, n_thr, a)) return DRN_ERR_ARG;
  if (M == 0) return DRN_OK;
  if ((N > 0 && !quality) || !matches || !match_labels) return DRN_ERR_ARG;
  hipLaunchKernelGGL(match_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, quality, N, M, a, matches,
                     match_labels);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // extern "C"
