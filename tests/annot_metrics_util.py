"""Restatement of the annotated-box block of the per-step metrics (include/drn_wsod.h "per-step metrics"), shared by
tests/test_annot_metrics_cpu.py, tests/test_annot_metrics_gpu.py and the fixture's own check.  torch-CPU fp32 for the IoU - the
reference's own operations in its order - and int64 for every count.

What the reference computes and logs per iteration, for every head class:
  label_and_sample_proposals   projects/WSL/wsl/modeling/roi_heads/roi_heads.py:256-353   roi_head/num_{fg,bg,ig}_samples
  pairwise_iou                 detectron2/structures/boxes.py:329-361
  Matcher                      detectron2/modeling/matcher.py (allow_low_quality_matches=False)
  _sample_proposals            roi_heads.py:214-246 (returns before the sampling)
  WSDDNOutputs._log_accuracy   projects/WSL/wsl/modeling/roi_heads/fast_rcnn.py:213-235   fast_rcnn/{cls_accuracy,fg_cls_accuracy,
                                                                                           false_negative}"""
import numpy as np
import torch

NAMES = ("roi_head/num_fg_samples", "roi_head/num_bg_samples", "roi_head/num_ig_samples", "fast_rcnn/cls_accuracy",
         "fast_rcnn/fg_cls_accuracy", "fast_rcnn/false_negative")


def pairwise_iou(gt, props):
    """boxes.py:329-361, operation for operation: gt [G, 4], props [R, 4] fp32 -> iou [G, R] fp32"""
    gt, props = torch.as_tensor(gt, dtype=torch.float32), torch.as_tensor(props, dtype=torch.float32)
    area1 = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])           # Boxes.area(), boxes.py:188-196
    area2 = (props[:, 2] - props[:, 0]) * (props[:, 3] - props[:, 1])
    wh = torch.min(gt[:, None, 2:], props[:, 2:]) - torch.max(gt[:, None, :2], props[:, :2])
    wh.clamp_(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (area1[:, None] + area2 - inter), torch.zeros(1, dtype=inter.dtype))


def match(iou, thresholds, labels):
    """Matcher.__call__ (matcher.py) without low-quality matches: iou [G, R] -> (matched [R], matcher labels [R]).  The maximum's
    index on equal IoU is the LOWEST box index (the definition of include/drn_wsod.h), taken here with an explicit loop so that it
    does not rest on a library's tie rule."""
    G, R = iou.shape
    if G == 0:  # matcher.py: an empty matrix gives index 0 and labels[0] everywhere
        return np.zeros(R, dtype=np.int64), np.full(R, labels[0], dtype=np.int64)
    v = iou.numpy()
    best, idx = v[0].copy(), np.zeros(R, dtype=np.int64)
    for j in range(1, G):
        take = v[j] > best
        best[take], idx[take] = v[j][take], j
    thr = [-float("inf")] + [float(t) for t in thresholds] + [float("inf")]
    bt = torch.from_numpy(best)
    ml = np.ones(R, dtype=np.int64)
    for l, lo, hi in zip(labels, thr[:-1], thr[1:]):
        ml[((bt >= lo) & (bt < hi)).numpy()] = l  # (a python scalar against an fp32 tensor, as the reference compares)
    return idx, ml


def label_proposals(props, img_off, gt_boxes, gt_classes, gt_count, K, thresholds=(0.5,), labels=(0, 1)):
    """roi_heads.py:256-353 + :214-246 for every image -> (labels int64 [M], matched int64 [M], counts int64 [n_ig, n_bg, n_fg]
    summed over the images).  gt_boxes [n_img, max_gt, 4], gt_classes [n_img, max_gt], gt_count [n_img]."""
    props = np.asarray(props, dtype=np.float32).reshape(-1, 4)
    M = props.shape[0]
    out_l, out_m = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    counts = np.zeros(3, dtype=np.int64)
    for i in range(len(img_off) - 1):
        r0, r1 = int(img_off[i]), int(img_off[i + 1])
        G = int(gt_count[i])
        gb = np.asarray(gt_boxes[i], dtype=np.float32)[:G]
        gc = np.asarray(gt_classes[i]).astype(np.int64)[:G]
        idx, ml = match(pairwise_iou(gb.reshape(-1, 4), props[r0:r1]), thresholds, labels)
        if G > 0:
            cls = gc[idx].copy()
            cls[ml == 0] = K
            cls[ml == -1] = -1
        else:
            cls = np.full(r1 - r0, K, dtype=np.int64)
        out_l[r0:r1], out_m[r0:r1] = cls, idx
        n_ig, n_bg = int((cls == -1).sum()), int((cls == K).sum())
        counts += [n_ig, n_bg, cls.size - n_bg - n_ig]  # roi_heads.py:338-340
    return out_l, out_m, counts


def mil_counts(scores, labels, M):
    """fast_rcnn.py:213-235 over scores [>= M, C] and labels [>= M]: -> int64 [n_acc, n_fg_acc, n_fneg, n_fg] with the code's own
    bg_class_ind = C - 1 (for the MIL scores' C = K columns that is the LAST CLASS, not the background label K: restated as it is).
    np.argmax answers the FIRST maximal index, like torch.argmax."""
    x = np.asarray(scores, dtype=np.float32)[:M]
    g = np.asarray(labels).astype(np.int64)[:M]
    bg = x.shape[1] - 1
    p = x.argmax(axis=1).astype(np.int64) if M else np.zeros(0, dtype=np.int64)
    fg = (g >= 0) & (g < bg)
    return np.array([(p == g).sum(), (fg & (p == g)).sum(), (fg & (p == bg)).sum(), fg.sum()], dtype=np.int64)


def scalars(label_counts, mil, M, n_img):
    """the six un-suffixed scalars by the reference's names and omission rules (python-float ratios of integers)"""
    n_ig, n_bg, n_fg = (int(v) for v in label_counts)
    n_acc, n_fg_acc, n_fneg, mil_fg = (int(v) for v in mil)
    out = {"roi_head/num_fg_samples": n_fg / n_img, "roi_head/num_bg_samples": n_bg / n_img,
           "roi_head/num_ig_samples": n_ig / n_img}
    if M > 0:
        out["fast_rcnn/cls_accuracy"] = n_acc / M
        if mil_fg > 0:
            out["fast_rcnn/fg_cls_accuracy"] = n_fg_acc / mil_fg
            out["fast_rcnn/false_negative"] = n_fneg / mil_fg
    return out


def pack(boxes_per_image, classes_per_image, max_gt):
    """lists of [G_i, 4] boxes and [G_i] classes -> (gt_boxes fp32 [n, max_gt, 4], gt_classes int32 [n, max_gt], count int32 [n])"""
    n = len(boxes_per_image)
    gb = np.zeros((n, max_gt, 4), dtype=np.float32)
    gc = np.zeros((n, max_gt), dtype=np.int32)
    cnt = np.zeros(n, dtype=np.int32)
    for i, (b, c) in enumerate(zip(boxes_per_image, classes_per_image)):
        b = np.asarray(b, dtype=np.float32).reshape(-1, 4)
        gb[i, : len(b)], gc[i, : len(b)], cnt[i] = b, np.asarray(c, dtype=np.int32), len(b)
    return gb, gc, cnt
