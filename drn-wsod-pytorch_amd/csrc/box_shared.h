// Box arithmetic shared by the translation units that must agree bit for bit: the annotated-box labelling (pairwise_iou + Matcher)
// of drn_label_proposals and drn_annot_box_reg, the regression target (Box2BoxTransform.get_deltas) of drn_box_reg_loss and
// drn_annot_box_reg, and the decode (Box2BoxTransform.apply_deltas) of drn_apply_deltas and drn_apply_deltas_mean.  One definition
// each, so the equalities hold by construction.  Every unit that includes this is built with -ffp-contract=off.
#pragma once
#include "drn_common.h"

namespace drn_box {

enum { LP_THREADS = 256, LP_WAVES = LP_THREADS / 64, LP_MAX_GT = 256 };  // (= DRN_LABEL_MAX_GT: asserted where the header is seen)

struct MatcherArgs { float thr[3]; int lab[4]; int nthr; };

// the annotated boxes of ONE image in LDS: corners, areas, classes (at most 256 x 6 words)
struct AnnotLds {
  float box[LP_MAX_GT][4];
  float area[LP_MAX_GT];
  int cls[LP_MAX_GT];
};

// boxes 0 .. G of image `img` -> LDS (the whole workgroup; the caller's barrier follows)
__device__ __forceinline__ void stage_annot(AnnotLds& s, const float* __restrict__ gt_boxes, const int* __restrict__ gt_classes,
                                            int img, int max_gt, int G) {
  for (int g = threadIdx.x; g < G; g += LP_THREADS) {
    const float* gb = gt_boxes + ((long)img * max_gt + g) * 4;
    const float gx1 = gb[0], gy1 = gb[1], gx2 = gb[2], gy2 = gb[3];
    s.box[g][0] = gx1; s.box[g][1] = gy1; s.box[g][2] = gx2; s.box[g][3] = gy2;
    s.area[g] = (gx2 - gx1) * (gy2 - gy1);
    s.cls[g] = gt_classes[(long)img * max_gt + g];
  }
}

// one proposal against the G staged boxes: pairwise_iou (detectron2/structures/boxes.py:329-361) in the reference's operation
// order, the best box (lowest index on ties), Matcher without low-quality matches -> class (K background, -1 ignore); bg = the box
__device__ __forceinline__ int label_row(const AnnotLds& s, int G, float x1, float y1, float x2, float y2, const MatcherArgs& a,
                                         int K, int& bg) {
  const float a2 = (x2 - x1) * (y2 - y1);
  float best = -1.f;  // every IoU is >= 0: box 0 is always taken, a later box only when strictly better (lowest index on ties)
  bg = 0;
  for (int g = 0; g < G; ++g) {
    const float iw = fmaxf(fminf(s.box[g][2], x2) - fmaxf(s.box[g][0], x1), 0.f);
    const float ih = fmaxf(fminf(s.box[g][3], y2) - fmaxf(s.box[g][1], y1), 0.f);
    const float inter = iw * ih;
    const float iou = inter > 0.f ? inter / (s.area[g] + a2 - inter) : 0.f;
    if (iou > best) { best = iou; bg = g; }
  }
  int cls = K;  // an image without annotated boxes: every row background, matched 0 (roi_heads.py:234-246)
  if (G > 0) {
    int ml = 1;  // Matcher: labels default 1, then per interval low <= v < high over [-inf, thr.., +inf]
    for (int q = 0; q <= a.nthr; ++q) {
      const float lo = q == 0 ? -INFINITY : a.thr[q - 1];
      const float hi = q == a.nthr ? INFINITY : a.thr[q];
      if (best >= lo && best < hi) ml = a.lab[q];
    }
    cls = ml == 0 ? K : ml == -1 ? -1 : s.cls[bg];
  }
  return cls;
}

// pairwise_iou (boxes.py:329-361) of ONE pair, the arithmetic of label_row's loop body: g = the staged box with its corner area,
// (x1, y1, x2, y2) / a2 = the other box and its corner area.  Used by the proposal-recall matching (proprecall.hip).
__device__ __forceinline__ float pair_iou(float gx1, float gy1, float gx2, float gy2, float garea, float x1, float y1, float x2,
                                          float y2, float a2) {
  const float iw = fmaxf(fminf(gx2, x2) - fmaxf(gx1, x1), 0.f);
  const float ih = fmaxf(fminf(gy2, y2) - fmaxf(gy1, y1), 0.f);
  const float inter = iw * ih;
  return inter > 0.f ? inter / (garea + a2 - inter) : 0.f;
}

// host side: thresholds / labels -> MatcherArgs; false = a label outside {-1, 0, 1}
inline bool matcher_args(const float* thresholds, const int* match_labels, int nthr, MatcherArgs& a) {
  a = MatcherArgs{};
  a.nthr = nthr;
  for (int q = 0; q < nthr; ++q) a.thr[q] = thresholds[q];
  for (int q = 0; q <= nthr; ++q) {
    a.lab[q] = match_labels[q];
    if (a.lab[q] < -1 || a.lab[q] > 1) return false;
  }
  return true;
}

// Box2BoxTransform.get_deltas (box_regression.py:38-71): s = the proposal, t = the target box
__device__ __forceinline__ void box_target(const float* s, const float* t, float wx, float wy, float ww, float wh,
                                           float (&d)[4]) {
  const float sw = s[2] - s[0], sh = s[3] - s[1];
  const float sx = s[0] + 0.5f * sw, sy = s[1] + 0.5f * sh;
  const float tw = t[2] - t[0], th = t[3] - t[1];
  const float tx = t[0] + 0.5f * tw, ty = t[1] + 0.5f * th;
  d[0] = wx * (tx - sx) / sw; d[1] = wy * (ty - sy) / sh;
  d[2] = ww * logf(tw / sw); d[3] = wh * logf(th / sh);
}

// Box2BoxTransform.apply_deltas (box_regression.py:73-110) of one (row, class): d = its four deltas, or NULL for zeros
__device__ __forceinline__ void decode_box(const float* d, float x1, float y1, float x2, float y2, float wx, float wy, float ww,
                                           float wh, float clampv, float* o) {
  const float w = x2 - x1, h = y2 - y1;
  const float cx = x1 + 0.5f * w, cy = y1 + 0.5f * h;
  float dx = 0.f, dy = 0.f, dw = 0.f, dh = 0.f;
  if (d) {
    dx = d[0] / wx; dy = d[1] / wy; dw = fminf(d[2] / ww, clampv); dh = fminf(d[3] / wh, clampv);
  }
  const float pcx = dx * w + cx, pcy = dy * h + cy;
  const float pw = expf(dw) * w, ph = expf(dh) * h;
  o[0] = pcx - 0.5f * pw; o[1] = pcy - 0.5f * ph; o[2] = pcx + 0.5f * pw; o[3] = pcy + 0.5f * ph;
}

}  // namespace drn_box
