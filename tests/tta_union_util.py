"""A numpy / oracle restatement of GeneralizedRCNNWithTTAUNION's merge (test_time_augmentation_union.py:228-264), shared by the
CPU test that pins it against the reference's golden and the GPU tests that compare ops.detect_union_batch with it.

union_rows: every pass's live detections mapped back to the original image (the package's `_apply_box`: the flip, then the
scale, each on the four corners in float32) and concatenated in pass order then detection order.
merge: the reference's own steps on those rows - a zero [n, K + 1] matrix with one score placed per row, then the oracle's
fast_rcnn_inference_single_image (finite-row filter, clip, threshold, row-major candidates, stable sort, batched NMS, top-k)."""
import numpy as np
import torch

import golden_util as G
from __graft_entry__ import load_package

load_package()
from drn_wsod_pytorch_amd.modeling.tta import _apply_box  # noqa: E402

O = G.O
CASES = [("avg", 100), ("avg", 12), ("def", 100), ("def", 12)]


def inverse_box(boxes, sx, sy, flip_w):
    """TransformList([Resize, HFlip?]).inverse().apply_box: HFlipTransform.inverse, then ResizeTransform.inverse; sx, sy as float32"""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    if flip_w is not None and flip_w >= 0:
        b = _apply_box(b, np.float32(1), np.float32(1), np.float32(flip_w))
    return _apply_box(b, np.float32(sx), np.float32(sy), None)


def union_rows(blk_boxes, blk_scores, blk_classes, counts, tfms):
    """padded blocks [B, T, 4] / [B, T] / [B, T], counts [B], tfms B x (sx, sy, flip_w) -> (boxes [n, 4] on the original image,
    scores [n], classes [n]); nothing beyond a block's count is looked at"""
    T = blk_scores.shape[1]
    ub, us, uc = [], [], []
    for b in range(blk_scores.shape[0]):
        n = min(max(int(counts[b]), 0), T)
        sx, sy, fw = tfms[b]
        with np.errstate(all="ignore"):
            ub.append(inverse_box(blk_boxes[b, :n], sx, sy, fw))
        us.append(np.asarray(blk_scores[b, :n], dtype=np.float32))
        uc.append(np.asarray(blk_classes[b, :n], dtype=np.int64))
    return np.concatenate(ub).reshape(-1, 4), np.concatenate(us), np.concatenate(uc)


def merge(ub, us, uc, shape_hw, K, nms_thresh, topk, score_thresh=1e-8):
    """-> (boxes [m, 4], scores [m], classes [m], rows [m]) as numpy; rows index the finite union rows"""
    n = us.shape[0]
    s2 = torch.zeros((n, K + 1), dtype=torch.float32)
    ok = (uc >= 0) & (uc < K)  # (the reference's classes always are; a row of another class has no non-zero entry)
    idx = torch.from_numpy(np.nonzero(ok)[0])
    s2[idx, torch.from_numpy(uc[ok])] = torch.from_numpy(us[ok])
    finite_score = torch.from_numpy(np.isfinite(us))
    s2[~finite_score, 0] = float("nan")  # a non-finite score outside 0 .. K-1 still makes its row non-finite
    rb, rs, rc, rr = O.fast_rcnn_inference_single_image(torch.from_numpy(np.ascontiguousarray(ub)), s2, shape_hw, score_thresh,
                                                        nms_thresh, topk)
    return rb.numpy(), rs.numpy(), rc.numpy(), rr.numpy()


def golden_blocks(d, tag, topk):
    """the golden's recorded per-pass detections of one run as padded blocks (slots beyond the count: zeros / class -1) with the
    passes' (sx, sy, flip_w), formed like the mappers form them"""
    pre = "%s_k%d_" % (tag, topk)
    A = int(d["n_aug"])
    H, W = d["image_u8"].shape[1:]
    bb = np.zeros((A, topk, 4), np.float32)
    bs = np.zeros((A, topk), np.float32)
    bc = np.full((A, topk), -1, np.int32)
    cnt = np.zeros((A,), np.int32)
    tfms = []
    for i in range(A):
        n = d[pre + "pass%d_scores" % i].shape[0]
        bb[i, :n], bs[i, :n], bc[i, :n], cnt[i] = d[pre + "pass%d_boxes" % i], d[pre + "pass%d_scores" % i], d[pre + "pass%d_classes" % i], n
        nh, nw = d["aug%d_image" % i].shape[1:]
        tfms.append((W * 1.0 / nw, H * 1.0 / nh, float(nw) if i % 2 == 1 else -1.0))  # plain and flipped image are adjacent
    return bb, bs, bc, cnt, tfms


def tta_cfg_opts(d, det_topk):
    return ["TEST.AUG.ENABLED", "True", "TEST.AUG.MIN_SIZES", str(tuple(int(x) for x in d["min_sizes"])), "TEST.AUG.MAX_SIZE",
            str(int(d["max_size"])), "TEST.AUG.FLIP", "True", "DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TEST", str(int(d["topk"])),
            "TEST.DETECTIONS_PER_IMAGE", str(int(det_topk))]
