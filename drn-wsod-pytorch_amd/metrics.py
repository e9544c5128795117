"""Per-step training metrics from a device-side ring (include/drn_wsod.h, "per-step metrics").

The reference floats every logged scalar on the host each iteration - one sync per scalar:
  every loss and total_loss                                 detectron2/engine/train_loop.py:260-289 (_write_metrics)
  fast_rcnn/{cls_accuracy,fg_cls_accuracy,false_negative}_r{k}   projects/WSL/wsl/modeling/roi_heads/fast_rcnn.py:1098-1126
  roi_head/num_{fg,bg,ig}_samples_r{k}                      roi_heads.py:338-349, roi_heads_oicr.py:366-374
Here the head engine issues two small launches behind the loss tail (drn_head_metrics, drn_metrics_record) that write ONE record
per step into a ring in device memory; MetricsRing.drain() copies state + ring to pinned host memory on the stream the heads run
on - stream-ordered behind every step issued so far, so it only ever sees complete records - and collect() decodes it once the
copy's event has completed.  No side stream, no host sync on the step.

The annotated-box block (enable_metrics(annotated=True)): the six UN-suffixed scalars every head class of the reference logs from
the annotated boxes - they feed no loss -
  roi_head/num_{fg,bg,ig}_samples                           roi_heads.py:256-353 (label_and_sample_proposals)
  fast_rcnn/{cls_accuracy,fg_cls_accuracy,false_negative}   fast_rcnn.py:213-235 (WSDDNOutputs / CSCOutputs._log_accuracy of the MIL scores)
from two more launches in front of the record (drn_label_proposals, drn_mil_metrics), published in the record's unused space.

More than one rank: every rank records its own losses and counts; the reference's cross-rank average of _write_metrics
(comm.gather + np.mean) is not built."""
import struct

import torch

from . import ops
from ._cabi import DrnError

_W = ops.METRICS_RECORD_WORDS
_LOSS0, _CNT0 = 4, 4 + ops.METRICS_MAX_LOSSES
_COUNTERS = ("n_ig", "n_bg", "n_fg", "n_acc", "n_fg_acc", "n_fneg")
_ANN0 = _CNT0 + ops.METRICS_COUNTERS * ops.METRICS_ANNOT_ROW  # the last head slot: the annotated-box block's six counters


def _f32(word):
    return struct.unpack("<f", struct.pack("<I", word & 0xFFFFFFFF))[0]


def decode_record(words, names, n_img):
    """One record (METRICS_RECORD_WORDS ints, the layout of include/drn_wsod.h) -> {name: python number}; the ONE place that knows
    the word order.  Every loss under its own name, total_loss = their Python-float sum in list order; per branch k
    roi_head/num_{fg,bg,ig}_samples_r{k} = n / n_img, fast_rcnn/cls_accuracy_r{k} = n_acc / M only if M > 0,
    fast_rcnn/fg_cls_accuracy_r{k} = n_fg_acc / n_fg and fast_rcnn/false_negative_r{k} = n_fneg / n_fg only if n_fg > 0.
    A record whose flag word says so carries the annotated-box block: the same six names without a suffix, the two foreground
    ratios over the MIL statistics' own foreground count (labels in [0, K - 1): fast_rcnn.py:219-221) and only if that is > 0."""
    n, nh, M = int(words[1]), int(words[2]), int(words[3])
    if len(names) != n:
        raise DrnError("metrics record holds %d losses, %d names are known (%s)" % (n, len(names), ", ".join(names)))
    out, total = {}, 0.0
    for i, name in enumerate(names):
        v = _f32(int(words[_LOSS0 + i]))
        out[name] = v
        total = total + v
    out["total_loss"] = total
    for k in range(nh):
        c = dict(zip(_COUNTERS, (int(words[_CNT0 + ops.METRICS_COUNTERS * k + j]) for j in range(ops.METRICS_COUNTERS))))
        out["roi_head/num_fg_samples_r%d" % k] = c["n_fg"] / n_img
        out["roi_head/num_bg_samples_r%d" % k] = c["n_bg"] / n_img
        out["roi_head/num_ig_samples_r%d" % k] = c["n_ig"] / n_img
        if M > 0:
            out["fast_rcnn/cls_accuracy_r%d" % k] = c["n_acc"] / M
        if c["n_fg"] > 0:
            out["fast_rcnn/fg_cls_accuracy_r%d" % k] = c["n_fg_acc"] / c["n_fg"]
            out["fast_rcnn/false_negative_r%d" % k] = c["n_fneg"] / c["n_fg"]
    if (int(words[ops.METRICS_ANNOT_WORD_FLAG]) & 0xFFFFFFFF) == ops.METRICS_ANNOT_FLAG:
        c = dict(zip(_COUNTERS, (int(words[_ANN0 + j]) for j in range(ops.METRICS_COUNTERS))))
        mil_fg = int(words[ops.METRICS_ANNOT_WORD_FG])
        out["roi_head/num_fg_samples"] = c["n_fg"] / n_img
        out["roi_head/num_bg_samples"] = c["n_bg"] / n_img
        out["roi_head/num_ig_samples"] = c["n_ig"] / n_img
        if M > 0:
            out["fast_rcnn/cls_accuracy"] = c["n_acc"] / M
            if mil_fg > 0:
                out["fast_rcnn/fg_cls_accuracy"] = c["n_fg_acc"] / mil_fg
                out["fast_rcnn/false_negative"] = c["n_fneg"] / mil_fg
    return out


class MetricsRing:
    """Owns the ring, its state, the counts scratch of drn_head_metrics and a pinned host copy.  names: the loss names in list
    order, n_img: images per step (both set by the head engine when it issues a record); iter0: the training iteration of
    record 0 (as LossGuard.iter0).  drain() / collect() are the host's two halves; collected: records handed out or given up so far."""

    def __init__(self, slots=256, device="cuda", annotated=False, max_gt=64):
        self.slots = int(slots)
        # the annotated-box block: off = no launch, buffer or record word differs from a ring without the option
        self.annotated, self.max_gt = bool(annotated), int(max_gt)
        self.annot_labels = self.annot_matched = None  # what drn_label_proposals wrote for the step issued last
        d = ops.metrics_ring(self.slots, device)
        self.buf, self.state, self.ring, self.counts = d["buf"], d["state"], d["ring"], d["counts"]
        self.host = torch.zeros_like(self.buf, device="cpu")
        if self.buf.is_cuda:
            self.host = self.host.pin_memory()
        self.names, self.n_img, self.iter0 = [], 1, 0
        self.collected = 0
        self._event = None

    # ---- device side: what the head engine calls behind its loss tail ----------------------------------------------
    def record(self, names, loss_list, n_img, M, logits=None, col0s=(), K=0, labels=(), annot=None):
        """the step's two launches on the current stream: label statistics of len(col0s) branches (none: losses only), then the
        record.  annot (the annotated-box block; dict(props, img_off, boxes, classes, count, thresholds, labels, scores, max_rows)):
        drn_label_proposals and drn_mil_metrics into the block's row of the scratch, in front of the record"""
        names = list(names)
        if self.names and names != self.names:
            raise DrnError("the loss list changed while metrics are recorded (%s -> %s): disable_metrics() and enable again"
                           % (", ".join(self.names), ", ".join(names)))
        self.names, self.n_img = names, int(n_img)
        nh = len(col0s)
        if nh:
            ops.head_metrics(logits, col0s, K, labels, M, self.counts)
        if annot is None:
            ops.metrics_record(loss_list, self.counts, nh, M, self.ring, self.state)
            return
        if nh > ops.METRICS_ANNOT_ROW:
            raise DrnError("the annotated-box block takes the record's last head slot: %d branches leave no room" % nh)
        if self.annot_labels is None or self.annot_labels.numel() != M:  # (static in a graphed step: allocated at its priming step)
            self.annot_labels = torch.empty((M,), dtype=torch.int32, device=self.counts.device)
            self.annot_matched = torch.empty((M,), dtype=torch.int32, device=self.counts.device)
        block = self.counts[ops.METRICS_ANNOT_ROW]
        ops.label_proposals(annot["props"], annot["img_off"], n_img, annot["boxes"], annot["classes"], annot["count"], K,
                            annot["thresholds"], annot["labels"], counts=block, max_rows=annot.get("max_rows"),
                            out=(self.annot_labels, self.annot_matched))
        ops.mil_metrics(annot["scores"], self.annot_labels, M, block)
        ops.metrics_record(loss_list, self.counts, nh, M, self.ring, self.state, annot=True)

    # ---- host side -------------------------------------------------------------------------------------------------------
    def drain(self):
        """non-blocking copy of state + ring to the pinned buffer on the CURRENT stream - the stream the heads run on - and an
        event behind it.  Stream order makes the copy see complete records only."""
        self.host.copy_(self.buf, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record()

    def collect(self, wait=False):
        """-> ([(iteration, {name: value}), ...], lost).  Decodes the last drain once its event has completed (wait=True:
        after synchronising THAT event only); ([], 0) while it has not, or when nothing was drained."""
        ev = self._event
        if ev is None:
            return [], 0
        if wait:
            ev.synchronize()
        elif not ev.query():
            return [], 0
        self._event = None
        return self.decode(self.host)

    def decode(self, host):
        """records `collected` .. count-1 of a host copy [4 + slots * words]: the ones the ring has overwritten (index < count -
        slots) and any slot whose two index words do not both equal the expected index count as lost - nothing is invented."""
        words = host.tolist()
        count, S = words[0], self.slots
        first = max(self.collected, count - S)
        lost = first - self.collected
        out = []
        for i in range(first, count):
            rec = words[4 + (i % S) * _W: 4 + (i % S + 1) * _W]
            if (rec[0] & 0xFFFFFFFF) != (i & 0xFFFFFFFF) or (rec[_W - 1] & 0xFFFFFFFF) != (i & 0xFFFFFFFF):
                lost += 1
                continue
            out.append((self.iter0 + i, decode_record(rec, self.names, self.n_img)))
        self.collected = max(self.collected, count)
        return out, lost
