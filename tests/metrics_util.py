"""int64 numpy restatement of the per-step metrics (include/drn_wsod.h, "per-step metrics"), shared by the metrics tests.

What the reference logs per refinement branch k and iteration:
  fast_rcnn/cls_accuracy_r{k}, fg_cls_accuracy_r{k}, false_negative_r{k}   projects/WSL/wsl/modeling/roi_heads/fast_rcnn.py:1098-1126
      pred = logits.argmax(dim=1); bg = K; fg = (gt >= 0) & (gt < bg)
      cls_accuracy = #(pred == gt) / gt.numel()                              (only if gt.numel() > 0)
      fg_cls_accuracy = #(pred[fg] == gt[fg]) / #fg, false_negative = #(pred[fg] == bg) / #fg   (only if #fg > 0)
  roi_head/num_{fg,bg,ig}_samples_r{k}                                      roi_heads.py:338-349, roi_heads_oicr.py:366-374
      mean over the images of #(gt in [0, K)), #(gt == K), #(gt == -1)
  every loss and total_loss = sum(loss_dict.values())                        detectron2/engine/train_loop.py:260-289"""
import numpy as np

COUNTERS = ("n_ig", "n_bg", "n_fg", "n_acc", "n_fg_acc", "n_fneg")


def head_counts(logits, col0s, K, labels, M):
    """-> int64 [nh, 6] in COUNTERS order.  logits: float32 [rows >= M, ld]; labels: nh int arrays of >= M entries.
    np.argmax answers the FIRST maximal index, like torch.argmax."""
    out = np.zeros((len(col0s), 6), dtype=np.int64)
    for k, c0 in enumerate(col0s):
        g = np.asarray(labels[k]).astype(np.int64)[:M]
        x = np.asarray(logits)[:M, c0: c0 + K + 1]
        p = x.argmax(axis=1).astype(np.int64) if M else np.zeros((0,), dtype=np.int64)
        fg = (g >= 0) & (g < K)
        out[k] = [(g == -1).sum(), (g == K).sum(), fg.sum(), (p == g).sum(), (fg & (p == g)).sum(), (fg & (p == K)).sum()]
    return out


def scalars(counts, M, n_img):
    """the logged scalars of one step's counts, by the reference's names and omission rules (python-float ratios of integers)"""
    out = {}
    for k, row in enumerate(np.asarray(counts).tolist()):
        c = dict(zip(COUNTERS, row))
        out["roi_head/num_fg_samples_r%d" % k] = c["n_fg"] / n_img
        out["roi_head/num_bg_samples_r%d" % k] = c["n_bg"] / n_img
        out["roi_head/num_ig_samples_r%d" % k] = c["n_ig"] / n_img
        if M > 0:
            out["fast_rcnn/cls_accuracy_r%d" % k] = c["n_acc"] / M
        if c["n_fg"] > 0:
            out["fast_rcnn/fg_cls_accuracy_r%d" % k] = c["n_fg_acc"] / c["n_fg"]
            out["fast_rcnn/false_negative_r%d" % k] = c["n_fneg"] / c["n_fg"]
    return out


def f32_bits(x):
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))
