"""Generated inputs for the NMS tests (tests/test_nms_gpu.py, tests/test_nms_cpu.py) and what the oracle says about them.

Boxes come in clusters so that suppression chains form: n // 8 cluster centres uniform in [0, 40 sqrt(n))^2, every box a random centre
plus a jitter uniform in +-6 with width and height uniform in 16 .. 32, uniform scores, uniform classes.  With K classes the n boxes
share the clusters and the field of n // K boxes: classes do not suppress each other, so n // 8 clusters for all K = 20 classes of
n = 129 boxes would leave 0.94 - 0.98 of them and no chain at all; sized per class, every class sees the density of the plain case.
A case is only worth
running when it can fail, so `checked_case` asserts on the ORACLE's result, before the device is asked, that
  * the kept share lies in [0.1, 0.9] (sizes from SHARE_FROM = 63 on: below that a share says little - one box is always kept), and
  * from n = 129 on at least one "revived" box exists: a kept box that overlaps an earlier box above the threshold, where that earlier
    box was itself suppressed - the box a kernel keeps wrongly dead when suppressed rows still suppress.
The oracle's answers are computed once per case and shared (lru_cache); nobody writes to them."""
import functools
import math

import numpy as np
import torch

from oracle import wsod_oracle as O

SHARE_FROM, REVIVED_FROM = 63, 129
PANEL = 512  # csrc/nms_shared.h drn_supp::PANEL: sorted rows per (mask, scan) launch pair


def generate(n, K=1, seed=0):
    """-> (boxes [n, 4] f32, scores [n] f32, classes [n] i64) as numpy arrays"""
    rs = np.random.RandomState(1000003 * seed + n)
    per_class = max(n // K, 1)  # clusters and field are sized for ONE class's boxes: every class sees the plain case's density
    nc = max(per_class // 8, 1)
    side = np.float32(40.0 * math.sqrt(per_class))
    centres = rs.uniform(0.0, side, (nc, 2)).astype(np.float32)
    c = centres[rs.randint(0, nc, n)] + rs.uniform(-6.0, 6.0, (n, 2)).astype(np.float32)
    wh = rs.uniform(16.0, 32.0, (n, 2)).astype(np.float32)
    half = wh * np.float32(0.5)
    boxes = np.concatenate([c - half, c + half], axis=1).astype(np.float32)
    scores = rs.uniform(0.0, 1.0, n).astype(np.float32)
    classes = rs.randint(0, K, n).astype(np.int64)
    return boxes.reshape(n, 4), scores, classes


def _iou_gt(a, b, thr):
    """[len(a), len(b)] bool: the oracle's float32 ratio inter / (area_a + area_b - inter) > thr"""
    aa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(np.float32(0), np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]))
    h = np.maximum(np.float32(0), np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]))
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (aa[:, None] + ab[None, :] - inter) > np.float32(thr)


def revived_count(boxes, scores, classes, keep, thr, prefix=4097):
    """kept boxes that an earlier SUPPRESSED box of their own class overlaps above thr, among the first `prefix` sorted positions
    (greedy NMS of a prefix of the sorted list is the prefix of the result, so a revived box there is one overall).  boxes are the
    boxes the suppression ran on (offset ones for the coordinate-offset form), classes None for plain nms."""
    n = len(scores)
    order = np.argsort(-scores.astype(np.float64), kind="stable")[:prefix]
    kept = np.zeros(n, bool)
    kept[np.asarray(keep, np.int64)] = True
    b, k = boxes[order], kept[order]
    over = np.triu(_iou_gt(b, b, thr), 1)  # [earlier, later]
    if classes is not None:
        c = classes[order]
        over &= c[:, None] == c[None, :]
    return int((over[~k].any(axis=0) & k).sum())


def offset_boxes(boxes, classes):
    """torchvision 0.6 batched_nms: boxes + idxs.to(boxes) * (boxes.max() + 1), float32"""
    mx = np.float32(boxes.max())
    return boxes + (classes.astype(np.float32) * (mx + np.float32(1)))[:, None]


@functools.lru_cache(maxsize=None)
def checked_case(n, thr, K=0, seed=0):
    """-> dict(boxes, scores, classes (torch, host), keep = the oracle's list): K = 0 plain nms, K >= 1 batched_nms with K classes.
    Asserts the kept share and the revived boxes on the oracle's result (module docstring)."""
    boxes, scores, classes = generate(n, max(K, 1), seed)
    tb, ts, tc = torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(classes)
    keep = O.nms(tb, ts, thr) if K == 0 else O.batched_nms(tb, ts, tc, thr)
    assert keep.dtype == torch.int64
    if n >= SHARE_FROM:
        share = len(keep) / n
        assert 0.1 <= share <= 0.9, "n = %d thr = %g K = %d: kept share %.3f - the case proves nothing" % (n, thr, K, share)
    if n >= REVIVED_FROM:
        if K == 0:
            rv = revived_count(boxes, scores, None, keep.numpy(), thr)
        elif n < 40000:
            rv = revived_count(offset_boxes(boxes, classes), scores, None, keep.numpy(), thr)
        else:
            rv = revived_count(boxes, scores, classes, keep.numpy(), thr)
        assert rv >= 1, "n = %d thr = %g K = %d: no revived box - the case proves nothing" % (n, thr, K)
    return dict(boxes=tb, scores=ts, classes=tc, keep=keep)


def candidate_set(R, K, seed=0, low=0.3):
    """an inference-tail input whose candidates are the generator's boxes: -> (boxes [R, 4 K] f32, scores [R, K + 1] f32, (h, w)).
    Class c of row r is box r * K + c of generate(R * K, K); a share `low` of the scores lies below the tests' score threshold 0.05;
    the image is 8 short of the largest coordinate, so the clip moves the outermost boxes on both sides; row 7 is not finite."""
    b, s, _ = generate(R * K, K, seed)
    rs = np.random.RandomState(77 + seed)
    s = np.where(rs.uniform(size=R * K) < low, np.float32(0.01) * s, np.float32(0.05) + np.float32(0.9) * s).astype(np.float32)
    side = float(np.ceil(b.max())) - 8.0
    boxes = torch.from_numpy(b.reshape(R, 4 * K).copy())
    boxes[7, 3] = float("nan")
    scores = torch.cat([torch.from_numpy(s.reshape(R, K).copy()), torch.zeros(R, 1)], dim=1)
    return boxes, scores, (side, side)
