// Box regression of the PCL heads (reg/pcl_* recipes), gfx950:
//   drn_annot_box_reg      PCLOutputs.box_reg_loss, fast_rcnn.py:1746-1811, on the labels of roi_heads.py:214-353: the proposals are
//                          labelled against the ANNOTATED boxes and regress onto the matched annotated box - labelling, target, loss
//                          and gradient of every regressing branch and every image in one launch pair
//   drn_apply_deltas_mean  predict_boxes_K, fast_rcnn.py:1534-1559: decode of the mean of the branches' deltas
// The IoU / Matcher, the target and the decode are box_shared.h's - the code drn_label_proposals, drn_box_reg_loss and
// drn_apply_deltas run - so the documented bit equalities hold by construction.  Built with -ffp-contract=off.
#include "drn_common.h"
#include "box_shared.h"
#include "../../include/drn_wsod.h"

namespace {

using drn_box::AnnotLds;
using drn_box::LP_THREADS;
using drn_box::MatcherArgs;
static_assert(drn_box::LP_MAX_GT == DRN_LABEL_MAX_GT, "box_shared.h and include/drn_wsod.h disagree");
static_assert(LP_THREADS == 256, "the tree reduction below is written for 256 threads");

struct AnnotRegParams {
  const float* logits; long ld; int col0[DRN_BOXREG_MAX_HEADS]; int n_heads; int K;
  const float* props; const int* img_off; int n_img; int M;
  const float* gt_boxes; const int* gt_classes; const int* gt_count; int max_gt;
  MatcherArgs a; float wx, wy, ww, wh;
  float* dlogits; long ld_d; float loss_scale, inv_n_img;
  int* labels; int* matched; float* partial; int nbx; float* loss;
};

// Grid (ceil(max_rows / 256), n_img): a workgroup owns 256 consecutive rows of ONE image, the image's annotated boxes in LDS.
// Phase 1, one thread per row: label (once - it does not depend on the branch), target, then per listed head the row's
// sum_e |pred_e - target_e| and the workgroup's tree sum -> partial[(head * n_img + img) * nbx + blockIdx.x] (drn_box_reg_loss'
// row arithmetic and tree: for one image the partials are that entry's).  Phase 2: the workgroup's rows x 4K gradient block of
// every head with the lanes running along the columns - each wave instruction stores 64 consecutive floats of a row (or the end of
// one and the start of the next) instead of 64 rows' words ld_d apart; a row's label and target come from LDS, the thread that owns
// one of the class' four columns recomputes pred - target from the same two fp32 values: the same sign.
__global__ __launch_bounds__(LP_THREADS) void annot_boxreg_rows_kernel(AnnotRegParams p) {
  __shared__ AnnotLds s_ann;
  __shared__ float s_tgt[LP_THREADS][4];
  __shared__ int s_lab[LP_THREADS];
  __shared__ float s_red[LP_THREADS];
  const int img = blockIdx.y;
  const int r0 = max(p.img_off[img], 0), r1 = min(p.img_off[img + 1], p.M);
  const int base = r0 + blockIdx.x * LP_THREADS;
  if (base >= r1) return;  // (the whole workgroup: no barrier is left behind)
  const int G = max(min(p.gt_count[img], p.max_gt), 0);
  const int tid = threadIdx.x;
  const int r = base + tid;
  const bool live = r < r1;
  float s4[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const f32x4_t b = *reinterpret_cast<const f32x4_t*>(p.props + 4 * (long)r);
    s4[0] = b[0]; s4[1] = b[1]; s4[2] = b[2]; s4[3] = b[3];
  }
  drn_box::stage_annot(s_ann, p.gt_boxes, p.gt_classes, img, p.max_gt, G);
  __syncthreads();
  int bg;
  const int cls = drn_box::label_row(s_ann, G, s4[0], s4[1], s4[2], s4[3], p.a, p.K, bg);
  if (live && p.labels) p.labels[r] = cls;
  if (live && p.matched) p.matched[r] = bg;
  const bool fg = live && cls >= 0 && cls < p.K;  // (G > 0 on every such row: without boxes the label is K)
  float d[4] = {0.f, 0.f, 0.f, 0.f};
  if (fg) drn_box::box_target(s4, s_ann.box[bg], p.wx, p.wy, p.ww, p.wh, d);
  s_lab[tid] = fg ? cls : -1;
#pragma unroll
  for (int e = 0; e < 4; ++e) s_tgt[tid][e] = d[e];
  for (int h = 0; h < p.n_heads; ++h) {
    float l = 0.f;
    if (fg) {
      const float* pr = p.logits + (long)r * p.ld + p.col0[h] + 4 * cls;
      for (int e = 0; e < 4; ++e) l += fabsf(pr[e] - d[e]);
    }
    s_red[tid] = l;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) s_red[tid] += s_red[tid + o];
      __syncthreads();
    }
    if (tid == 0) p.partial[((long)h * p.n_img + img) * p.nbx + blockIdx.x] = s_red[0];
    __syncthreads();  // (s_red is rewritten by the next head; s_lab / s_tgt are complete behind the first of these barriers)
  }
  if (!p.dlogits) return;
  const float Mi = (float)(r1 - r0);
  const int C4 = 4 * p.K;
  const int n = min(r1 - base, (int)LP_THREADS) * C4;  // (<= 256 * 4K: K <= DRN_BOXREG_MAX_K keeps it inside an int)
  for (int h = 0; h < p.n_heads; ++h) {
    const float* lg = p.logits + (long)base * p.ld + p.col0[h];
    float* dl = p.dlogits + (long)base * p.ld_d + p.col0[h];
    for (int i = tid; i < n; i += LP_THREADS) {
      const int row = i / C4, j = i - row * C4;
      const int lab = s_lab[row];
      float g = 0.f;
      if (lab >= 0 && (j >> 2) == lab) {
        const float diff = lg[(long)row * p.ld + j] - s_tgt[row][j & 3];
        g = (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f)) / Mi * p.inv_n_img * p.loss_scale;
      }
      dl[(long)row * p.ld_d + j] = g;
    }
  }
}

// One thread per head: L_i = (the image's partials in ascending workgroup order) / M_i, the mean over the images as an fp64 sum
// in ascending image order rounded once (drn_pcl_refine_batch's definition; one image: L_0 itself).  An image without rows adds 0.
__global__ __launch_bounds__(64) void annot_boxreg_combine_kernel(AnnotRegParams p) {
  const int h = threadIdx.x;
  if (h >= p.n_heads) return;
  double acc = 0.0;
  for (int i = 0; i < p.n_img; ++i) {
    const int r0 = max(p.img_off[i], 0), r1 = min(p.img_off[i + 1], p.M);
    const int Mi = r1 - r0;
    if (Mi <= 0) continue;
    const int nb = min((Mi + LP_THREADS - 1) / LP_THREADS, p.nbx);
    const float* part = p.partial + ((long)h * p.n_img + i) * p.nbx;
    float l = 0.f;
    for (int q = 0; q < nb; ++q) l += part[q];
    acc += (double)(l / (float)Mi);
  }
  p.loss[h] = (float)(acc / (double)p.n_img);
}

struct MeanDeltaCols { int col0[DRN_BOXREG_MAX_HEADS]; int n; };

// one thread per (row, class): d = ((+0 + d_k0) + d_k1 + ...) / n_total, then drn_apply_deltas' decode
__global__ __launch_bounds__(256) void apply_deltas_mean_kernel(const float* logits, long ld, MeanDeltaCols c, float n_total,
                                                                const float* boxes, float* out, int M, int K, float wx, float wy,
                                                                float ww, float wh, float clampv) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)M * K) return;
  const int r = i / K, k = i - (long)r * K;
  const float x1 = boxes[4 * (long)r], y1 = boxes[4 * (long)r + 1], x2 = boxes[4 * (long)r + 2], y2 = boxes[4 * (long)r + 3];
  float d[4] = {0.f, 0.f, 0.f, 0.f};
  for (int h = 0; h < c.n; ++h) {
    const float* s = logits + (long)r * ld + c.col0[h] + 4 * k;
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = d[e] + s[e];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) d[e] = d[e] / n_total;
  drn_box::decode_box(c.n ? d : nullptr, x1, y1, x2, y2, wx, wy, ww, wh, clampv, out + (long)r * 4 * K + 4 * k);
}

}  // namespace

extern "C" {

int drn_annot_box_reg(const float* logits, long ld, const int* col0s_host, int n_heads, int K, const float* proposals,
                      const int* img_off, int n_img, int M, int max_rows, const float* gt_boxes, const int* gt_classes,
                      const int* gt_count, int max_gt, const float* thresholds, const int* match_labels, int nthr,
                      const float* weights4_host, float* dlogits, long ld_d, float loss_scale, float* loss, int* labels,
                      int* matched, float* scratch, void* stream) {
  if (n_img < 0 || M < 0 || max_rows < 0 || max_gt < 1 || nthr < 1 || K < 1 || n_heads < 1) return DRN_ERR_ARG;
  if (max_gt > DRN_LABEL_MAX_GT || nthr > 3 || n_heads > DRN_BOXREG_MAX_HEADS || n_img > DRN_BOXREG_MAX_IMAGES ||
      K > DRN_BOXREG_MAX_K)
    return DRN_ERR_UNSUPPORTED;
  if (n_img == 0 || M == 0 || max_rows == 0) return DRN_OK;
  if (!logits || !col0s_host || !proposals || !img_off || !gt_boxes || !gt_classes || !gt_count || !thresholds || !match_labels ||
      !weights4_host || !loss || !scratch || ((uintptr_t)proposals & 15) || ((uintptr_t)logits & 3) || ((uintptr_t)dlogits & 3))
    return DRN_ERR_ARG;
  AnnotRegParams p = {};
  if (!drn_box::matcher_args(thresholds, match_labels, nthr, p.a)) return DRN_ERR_ARG;
  for (int h = 0; h < n_heads; ++h) {
    p.col0[h] = col0s_host[h];
    if (p.col0[h] < 0 || (long)p.col0[h] + 4L * K > ld || (dlogits && (long)p.col0[h] + 4L * K > ld_d)) return DRN_ERR_ARG;
  }
  p.logits = logits; p.ld = ld; p.n_heads = n_heads; p.K = K;
  p.props = proposals; p.img_off = img_off; p.n_img = n_img; p.M = M;
  p.gt_boxes = gt_boxes; p.gt_classes = gt_classes; p.gt_count = gt_count; p.max_gt = max_gt;
  p.wx = weights4_host[0]; p.wy = weights4_host[1]; p.ww = weights4_host[2]; p.wh = weights4_host[3];
  p.dlogits = dlogits; p.ld_d = ld_d; p.loss_scale = loss_scale; p.inv_n_img = 1.f / (float)n_img;
  p.labels = labels; p.matched = matched; p.partial = scratch; p.loss = loss;
  p.nbx = (max_rows + LP_THREADS - 1) / LP_THREADS;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(annot_boxreg_rows_kernel, dim3(p.nbx, n_img), dim3(LP_THREADS), 0, st, p);
  hipLaunchKernelGGL(annot_boxreg_combine_kernel, dim3(1), dim3(64), 0, st, p);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

int drn_apply_deltas_mean(const float* logits, long ld, const int* col0s_host, int n_heads, int n_total, const float* boxes,
                          float* out, int M, int K, const float* weights4_host, float scale_clamp, void* stream) {
  if (!boxes || !out || !weights4_host || K < 1 || M < 0 || n_heads < 0 || n_total < 1) return DRN_ERR_ARG;
  if (n_heads > DRN_BOXREG_MAX_HEADS) return DRN_ERR_UNSUPPORTED;
  if (M == 0) return DRN_OK;
  MeanDeltaCols c = {};
  c.n = n_heads;
  if (n_heads && (!logits || !col0s_host)) return DRN_ERR_ARG;
  for (int h = 0; h < n_heads; ++h) {
    c.col0[h] = col0s_host[h];
    if (c.col0[h] < 0 || (long)c.col0[h] + 4L * K > ld) return DRN_ERR_ARG;
  }
  const long tot = (long)M * K;
  hipLaunchKernelGGL(apply_deltas_mean_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits, ld,
                     c, (float)n_total, boxes, out, M, K, weights4_host[0], weights4_host[1], weights4_host[2],
                     weights4_host[3], scale_clamp);
  DRN_CHECK_LAUNCH();
  return DRN_OK;
}

}  // extern "C"
