// Per-step training metrics without a host sync: label statistics of the refinement branches (drn_head_metrics) and the step's
// record in a device-side ring (drn_metrics_record).  The reference floats every scalar on the host each iteration
// (fast_rcnn.py:1098-1126 _log_accuracy, roi_heads.py:338-349 / roi_heads_oicr.py:366-374 num_*_samples, train_loop.py:260-289
// _write_metrics); here the device writes one record per step and the host copies the ring every N steps.  Opt-in beside them, the
// annotated-box block: drn_label_proposals (roi_heads.py:256-353) and drn_mil_metrics (fast_rcnn.py:213-235) in front of
// drn_metrics_record_annot.
#include "drn_common.h"
#include "box_shared.h"
#include "../../include/drn_wsod.h"

namespace {

enum { HM_THREADS = 1024, HM_WAVES = HM_THREADS / 64, HM_ROWS_PER_BLOCK = DRN_METRICS_ROWS_PER_BLOCK,
       HM_NC = DRN_METRICS_COUNTERS, HM_STRIDE = DRN_METRICS_COUNT_STRIDE };

struct HeadArgs {
  const int* labels[DRN_METRICS_MAX_HEADS];
  int col0[DRN_METRICS_MAX_HEADS];
};

// arg-max candidate of a lane: the FIRST maximal index (torch.argmax's documented tie rule; 0.0 == -0.0 is a tie).  idx == INT_MAX
// marks "nothing seen yet", so an all -inf row still answers its first column.
struct Best { float v; int i; };
__device__ __forceinline__ void best_take(Best& b, float v, int i) {
  if (b.i == 0x7fffffff || v > b.v) { b.v = v; b.i = i; }
}
__device__ __forceinline__ void best_merge(Best& b, float v, int i) {
  if (v > b.v || (v == b.v && i < b.i)) { b.v = v; b.i = i; }
}

// Grid (ceil(M / 64), nh): a workgroup owns 64 consecutive rows of ONE branch.  A row is read by a sub-group of `sg` lanes of one
// wave (sg = power of two >= the 16-byte quads a row of K + 1 floats can touch, so 64 / sg rows per wave at a time): lane q of the
// sub-group takes quad q of the row's aligned span as one 16-byte load when the quad lies inside the branch's columns, and
// element by element at the two ragged ends - no column outside [col0, col0 + K] and no row >= M is ever read.  The arg-max is
// merged across the sub-group by shuffles, the six counters across the wave by ballots (exact integers), across the sixteen waves
// through LDS, and across workgroups with one atomicAdd(int*) per non-zero counter.  Sixteen waves per workgroup: the launch sits on
// the heads' dependent chain and is latency-bound, so a wave makes at most four passes (K + 1 = 81: two), while 64 rows per
// workgroup keep the atomics per counter at M / 64.
//
// MIL = true (drn_mil_metrics): the same walk over ONE matrix of K columns whose "background" is its last column, K - 1 - the
// statistics WSDDNOutputs._log_accuracy takes of the MIL scores (fast_rcnn.py:213-235: bg_class_ind = shape[1] - 1).  The labels'
// own three counters belong to drn_label_proposals; this variant adds [3] n_acc, [4] n_fg_acc, [5] n_fneg and [6] its own
// foreground count #{0 <= g < K - 1}.
template <bool MIL>
__global__ __launch_bounds__(HM_THREADS) void head_metrics_kernel(const float* __restrict__ logits, long ldl, HeadArgs a, int K,
                                                                   int M, int sg, int* __restrict__ counts) {
  constexpr int NC = MIL ? HM_NC + 1 : HM_NC;
  __shared__ int s_cnt[HM_WAVES][NC];
  const int k = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rpw = 64 / sg;                 // rows per wave and pass
  const int sub = lane / sg, q0 = lane - sub * sg;
  const int* __restrict__ lab = a.labels[k];
  const int col0 = a.col0[k];
  const int ncol = MIL ? K : K + 1;
  const int bgi = ncol - 1;  // the column that counts as background
  int acc[NC] = {};
  for (int base = wave * rpw; base < HM_ROWS_PER_BLOCK; base += HM_WAVES * rpw) {
    const int r = blockIdx.x * HM_ROWS_PER_BLOCK + base + sub;
    const bool live = base + sub < HM_ROWS_PER_BLOCK && r < M;
    const bool lead = live && q0 == 0;
    const int g = lead ? lab[r] : -2;  // (issued in front of the row's loads: one round trip, not two)
    Best b = {-INFINITY, 0x7fffffff};
    if (live) {
      const float* row = logits + (long)r * ldl + col0;
      const int mis = (int)(((uintptr_t)row >> 2) & 3);  // elements between the 16-byte line below and the row's first column
      const int nquad = (mis + ncol + 3) >> 2;
      for (int q = q0; q < nquad; q += sg) {
        const int j0 = q * 4 - mis;  // first column (relative to col0) of this quad
        if (j0 >= 0 && j0 + 4 <= ncol) {
          const f32x4_t v = *reinterpret_cast<const f32x4_t*>(row + j0);
          best_take(b, v[0], j0);
          best_take(b, v[1], j0 + 1);
          best_take(b, v[2], j0 + 2);
          best_take(b, v[3], j0 + 3);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (j0 + e >= 0 && j0 + e < ncol) best_take(b, row[j0 + e], j0 + e);
        }
      }
    }
    for (int o = sg >> 1; o > 0; o >>= 1) {  // (the partners of a sub-group share `live`)
      const float ov = __shfl_xor(b.v, o, 64);
      const int oi = __shfl_xor(b.i, o, 64);
      best_merge(b, ov, oi);
    }
    const int p = b.i;
    const bool fg = lead && g >= 0 && g < bgi;
    if (!MIL) {
      acc[0] += __popcll(__ballot(lead && g == -1));
      acc[1] += __popcll(__ballot(lead && g == K));
      acc[2] += __popcll(__ballot(fg));
    } else {
      acc[HM_NC] += __popcll(__ballot(fg));
    }
    acc[3] += __popcll(__ballot(lead && p == g));
    acc[4] += __popcll(__ballot(fg && p == g));
    acc[5] += __popcll(__ballot(fg && p == bgi));
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) s_cnt[wave][c] = acc[c];
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < HM_WAVES; ++w) s += s_cnt[w][threadIdx.x];
    if (s) atomicAdd(&counts[k * HM_STRIDE + threadIdx.x], s);
  }
}

// drn_label_proposals: label_and_sample_proposals of the reference (roi_heads.py:256-353) up to its early return - pairwise_iou
// (detectron2/structures/boxes.py:329-361) of an image's annotated boxes against its proposals, Matcher without low-quality matches
// (detectron2/modeling/matcher.py), the class of the matched box.  Grid (ceil(max_rows / 256), n_img): a workgroup owns 256
// consecutive rows of ONE image, one thread per row, the image's annotated boxes and their areas in LDS (every lane reads the same
// box: a broadcast).  fp32, the reference's operation order, no contraction (this file is built with -ffp-contract=off): the IoU
// equals torch's bit for bit.  The three label counters go wave -> LDS -> one integer atomicAdd per non-zero counter and workgroup.
using drn_box::AnnotLds;
using drn_box::LP_MAX_GT;
using drn_box::LP_THREADS;
using drn_box::LP_WAVES;
using drn_box::MatcherArgs;
static_assert(LP_MAX_GT == DRN_LABEL_MAX_GT, "box_shared.h and include/drn_wsod.h disagree");

// (the staging of the boxes, the IoU and the Matcher are box_shared.h's: drn_annot_box_reg labels with the same code)
__global__ __launch_bounds__(LP_THREADS) void label_proposals_kernel(const float* __restrict__ props,
                                                                     const int* __restrict__ img_off,
                                                                     const float* __restrict__ gt_boxes,
                                                                     const int* __restrict__ gt_classes,
                                                                     const int* __restrict__ gt_count, int max_gt, MatcherArgs a,
                                                                     int K, int M, int* __restrict__ labels,
                                                                     int* __restrict__ matched, int* __restrict__ counts) {
  __shared__ AnnotLds s_ann;
  __shared__ int s_cnt[LP_WAVES][3];
  const int img = blockIdx.y;
  const int r0 = img_off[img], r1 = min(img_off[img + 1], M);
  const int base = r0 + blockIdx.x * LP_THREADS;
  if (base >= r1) return;  // (the whole workgroup: no barrier is left behind)
  const int G = max(min(gt_count[img], max_gt), 0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = base + threadIdx.x;
  const bool live = r < r1;
  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
  if (live) {
    const f32x4_t b = *reinterpret_cast<const f32x4_t*>(props + 4 * (long)r);
    x1 = b[0]; y1 = b[1]; x2 = b[2]; y2 = b[3];
  }
  drn_box::stage_annot(s_ann, gt_boxes, gt_classes, img, max_gt, G);
  __syncthreads();
  int bg;
  const int cls = drn_box::label_row(s_ann, G, x1, y1, x2, y2, a, K, bg);
  if (live) {
    labels[r] = cls;
    matched[r] = bg;
  }
  const int n_ig = __popcll(__ballot(live && cls == -1));
  const int n_bg = __popcll(__ballot(live && cls == K));
  const int n_lv = __popcll(__ballot(live));
  if (lane == 0) {
    s_cnt[wave][0] = n_ig;
    s_cnt[wave][1] = n_bg;
    s_cnt[wave][2] = n_lv - n_bg - n_ig;  // (roi_heads.py:340: whatever is neither background nor ignored)
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < LP_WAVES; ++w) s += s_cnt[w][threadIdx.x];
    if (s) atomicAdd(&counts[threadIdx.x], s);
  }
}

struct RecLossPtrs { const float* p[DRN_METRICS_MAX_LOSSES]; };

// One wave.  Every lane keeps its own word of `counts` (64 words = one wave), the words meet in LDS, and the lane stores zero back
// into the word it read - the next step's drn_head_metrics finds the scratch cleared without a memset node.  The slot comes from
// state[0] in device memory, so a replayed graph walks through the ring.
// annot != 0 (drn_metrics_record_annot): the annotated-box block - row DRN_METRICS_ANNOT_ROW of `counts` - goes into the record's last
// head slot, its seventh counter into word 68, and word 70 says that the block is there.
__global__ __launch_bounds__(64) void metrics_record_kernel(RecLossPtrs lp, int n, int* __restrict__ counts, int nh, int M,
                                                           unsigned* __restrict__ ring, int S, int* __restrict__ state,
                                                           int annot) {
  __shared__ unsigned s_w[64];
  const int lane = threadIdx.x;
  const int idx = state[0];
  s_w[lane] = (unsigned)counts[lane];
  counts[lane] = 0;
  unsigned lossbits = 0u;
#pragma unroll
  for (int i = 0; i < DRN_METRICS_MAX_LOSSES; ++i)  // (unrolled: static indices into the argument block)
    if (lane == 4 + i && i < n) lossbits = __builtin_bit_cast(unsigned, lp.p[i][0]);  // (lane 4 + i stores word 4 + i)
  __syncthreads();
  unsigned* rec = ring + (long)(idx % S) * DRN_METRICS_RECORD_WORDS;
  for (int w = lane; w < DRN_METRICS_RECORD_WORDS; w += 64) {
    unsigned v = 0u;
    if (w == 0 || w == DRN_METRICS_RECORD_WORDS - 1) v = (unsigned)idx;
    else if (w == 1) v = (unsigned)n;
    else if (w == 2) v = (unsigned)nh;
    else if (w == 3) v = (unsigned)M;
    else if (w < 4 + DRN_METRICS_MAX_LOSSES) v = lossbits;
    else if (w < 4 + DRN_METRICS_MAX_LOSSES + HM_NC * DRN_METRICS_MAX_HEADS) {
      const int c = w - 4 - DRN_METRICS_MAX_LOSSES, br = c / HM_NC;
      v = (br < nh || (annot && br == DRN_METRICS_ANNOT_ROW)) ? s_w[br * HM_STRIDE + (c - br * HM_NC)] : 0u;
    } else if (annot && w == DRN_METRICS_ANNOT_WORD_FG) v = s_w[DRN_METRICS_ANNOT_ROW * HM_STRIDE + HM_NC];
    else if (annot && w == DRN_METRICS_ANNOT_WORD_FLAG) v = DRN_METRICS_ANNOT_FLAG;
    rec[w] = v;
  }
  if (lane == 0) state[0] = idx + 1;
}

}  // namespace

extern "C" {

int drn_head_metrics(const float* logits, long ldl, const int* col0s, int nh, int K, const void* const* labels, int M, int* counts,
                     void* stream) {
  if (nh < 0 || M < 0 || K < 1) return DRN_ERR_ARG;
  if (nh > DRN_METRICS_MAX_HEADS || K + 1 > 1024) return DRN_ERR_UNSUPPORTED;
  if (nh == 0 || M == 0) return DRN_OK;
  if (!logits || !col0s || !labels || !counts || ((uintptr_t)logits & 3)) return DRN_ERR_ARG;
  HeadArgs a;
  for (int k = 0; k < DRN_METRICS_MAX_HEADS; ++k) {
    const int s = k < nh ? k : 0;
    a.labels[k] = (const int*)labels[s];
    a.col0[k] = col0s[s];
    if (!a.labels[k] || a.col0[k] < 0 || (long)a.col0[k] + K + 1 > ldl) return DRN_ERR_ARG;
  }
  int sg = 2;  // lanes per row: a power of two >= the quads of a misaligned row
  while (sg < 64 && sg < (K + 1 + 3 + 3) / 4) sg <<= 1;
  const dim3 grid((M + HM_ROWS_PER_BLOCK - 1) / HM_ROWS_PER_BLOCK, nh);
  hipLaunchKernelGGL(head_metrics_kernel<false>, grid, dim3(HM_THREADS), 0, (hipStream_t)stream, logits, ldl, a, K, M, sg, counts);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_mil_metrics(const float* scores, long lds, int ncol, int bg_ind, const int* labels, int M, int* counts, void* stream) {
  if (M < 0 || ncol < 1) return DRN_ERR_ARG;
  if (ncol > 1024 || bg_ind != ncol - 1) return DRN_ERR_UNSUPPORTED;
  if (M == 0) return DRN_OK;
  if (!scores || !labels || !counts || ((uintptr_t)scores & 3) || lds < ncol) return DRN_ERR_ARG;
  HeadArgs a;
  for (int k = 0; k < DRN_METRICS_MAX_HEADS; ++k) {
    a.labels[k] = labels;
    a.col0[k] = 0;
  }
  int sg = 2;
  while (sg < 64 && sg < (ncol + 3 + 3) / 4) sg <<= 1;
  const dim3 grid((M + HM_ROWS_PER_BLOCK - 1) / HM_ROWS_PER_BLOCK, 1);
  hipLaunchKernelGGL(head_metrics_kernel<true>, grid, dim3(HM_THREADS), 0, (hipStream_t)stream, scores, lds, a, ncol, M, sg, counts);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_label_proposals(const float* proposals, const int* img_off, int n_img, int M, int max_rows, const float* gt_boxes,
                        const int* gt_classes, const int* gt_count, int max_gt, const float* thresholds, const int* match_labels,
                        int nthr, int K, int* labels, int* matched, int* counts, void* stream) {
  if (n_img < 0 || M < 0 || max_rows < 0 || max_gt < 1 || nthr < 1 || K < 1) return DRN_ERR_ARG;
  if (max_gt > DRN_LABEL_MAX_GT || nthr > 3) return DRN_ERR_UNSUPPORTED;
  if (n_img == 0 || M == 0 || max_rows == 0) return DRN_OK;
  if (!proposals || !img_off || !gt_boxes || !gt_classes || !gt_count || !thresholds || !match_labels || !labels || !matched ||
      !counts || ((uintptr_t)proposals & 15))
    return DRN_ERR_ARG;
  MatcherArgs a;
  if (!drn_box::matcher_args(thresholds, match_labels, nthr, a)) return DRN_ERR_ARG;
  const dim3 grid((max_rows + LP_THREADS - 1) / LP_THREADS, n_img);
  hipLaunchKernelGGL(label_proposals_kernel, grid, dim3(LP_THREADS), 0, (hipStream_t)stream, proposals, img_off, gt_boxes,
                     gt_classes, gt_count, max_gt, a, K, M, labels, matched, counts);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_metrics_record_annot(const void* const* losses, int n, int* counts, int nh, int M, int annot, unsigned* ring, int slots,
                             int* state, void* stream) {
  if (!losses || !counts || !ring || !state || n < 1 || nh < 0 || M < 0 || slots < 1) return DRN_ERR_ARG;
  if (n > DRN_METRICS_MAX_LOSSES || nh > DRN_METRICS_MAX_HEADS || (annot && nh > DRN_METRICS_ANNOT_ROW)) return DRN_ERR_UNSUPPORTED;
  RecLossPtrs lp;
  for (int i = 0; i < DRN_METRICS_MAX_LOSSES; ++i) {
    lp.p[i] = (const float*)losses[i < n ? i : 0];
    if (!lp.p[i]) return DRN_ERR_ARG;
  }
  hipLaunchKernelGGL(metrics_record_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, lp, n, counts, nh, M, ring, slots, state,
                     annot ? 1 : 0);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_metrics_record(const void* const* losses, int n, int* counts, int nh, int M, unsigned* ring, int slots, int* state,
                       void* stream) {
  return drn_metrics_record_annot(losses, n, counts, nh, M, 0, ring, slots, state, stream);
}

}  // extern "C"
