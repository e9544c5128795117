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
(comm.gather + np.mean) is not built.

CscStats (CSCROIHeads.enable_csc_stats): the reference's `Statistic` log of the CSC weights (third_party/cpg_stats.py, csc.txt)
from a table one launch pair per training forward counts on the device (drn_csc_stats; include/drn_wsod.h, "CSC weight
statistics"); one stream-ordered copy per LOG_PERIOD, no per-step read."""
import math
import os
import struct

import numpy as np
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


_CSC_LINE = "----------------------------------------------"
_CSC_HEAD = "#class\tpred\t#roi\t#class\tpred\tpos\tneg\t#roi\t#pos\t%\t#neg\t%\t#zero\t%\tclass"


def decode_csc_stats(words, K):
    """one table of drn_csc_stats (csc_stats_words(K) int64 words, the layout of include/drn_wsod.h) -> {field: numpy array [K]
    (int64 counts, float64 sums), "steps": int, "num_img": int}; the ONE place that knows the word order"""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.int64))
    if w.shape != (ops.csc_stats_words(K),):
        raise DrnError("a CSC statistics table of %d classes has %d words, not %s" % (K, ops.csc_stats_words(K), w.shape))
    nh, ni = len(ops.CSC_STATS_HEAD), len(ops.CSC_STATS_INT)
    out = {name: int(w[j]) for j, name in enumerate(ops.CSC_STATS_HEAD)}
    for j, name in enumerate(ops.CSC_STATS_INT):
        out[name] = w[nh + j * K: nh + (j + 1) * K].copy()
    fp = w[nh + ni * K:].view(np.float64)
    for j, name in enumerate(ops.CSC_STATS_FP):
        out[name] = fp[j * K: (j + 1) * K].copy()
    return out


def format_csc_stats(table, iteration):
    """Statistic.LogIterStats (third_party/cpg_stats.py:99-199) of one period's table, character for character: the 4-decimal
    placeholder rows, int(a / b) truncation, csc_acm_label printed as a float, no newline behind the last row.  The acm row is
    the sum of the per-class rows (the reference adds both in the same statements)."""
    t = {k: ([float(x) for x in v] if isinstance(v, np.ndarray) else v) for k, v in table.items()}
    K = len(t["ori_label"])
    out = _CSC_LINE + str(iteration) + _CSC_LINE + "\n" + _CSC_HEAD + "\n"
    for c in range(K):
        n = t["ori_label"][c]
        if n > 0:
            out += "{}\t{:.5f}\t{}\t".format(int(n), t["ori_pred"][c] / n, int(t["ori_num_roi"][c] / n))
        else:
            out += "0\t0.0000\t0\t"
        n = t["csc_label"][c]
        if n > 0:
            roi = t["csc_num_roi"][c]
            out += "{}\t{:.5f}\t{:.5f}\t{:.5f}\t{}\t{}\t{:.5f}\t{}\t{:.5f}\t{}\t{:.5f}\t{}".format(
                int(n), t["csc_pred"][c] / n, t["csc_pred_pos"][c] / n, t["csc_pred_neg"][c] / n, int(roi / n),
                int(t["csc_roi_pos"][c] / n), 1.0 * t["csc_roi_pos"][c] / roi, int(t["csc_roi_neg"][c] / n),
                1.0 * t["csc_roi_neg"][c] / roi, int(t["csc_roi_zero"][c] / n), 1.0 * t["csc_roi_zero"][c] / roi, c)
        else:
            out += "0\t0.0000\t0.0000\t0.0000\t0\t0\t0.0000\t0\t0.0000\t0\t0.0000\t{}".format(c)
        out += "\n"
    a = {k: math.fsum(v) for k, v in t.items() if isinstance(v, list)}
    if a["ori_label"] > 0 and a["csc_label"] > 0:
        n, m, roi = a["ori_label"], a["csc_label"], a["csc_num_roi"]
        out += "{}\t{:.5f}\t{}\t{}\t{:.5f}\t{:.5f}\t{:.5f}\t{}\t{}\t{:.5f}\t{}\t{:.5f}\t{}\t{:.5f}\t{}".format(
            int(n), a["ori_pred"] / n, int(a["ori_num_roi"] / n), m, a["csc_pred"] / m, a["csc_pred_pos"] / m,
            a["csc_pred_neg"] / m, int(roi / m), int(a["csc_roi_pos"] / m), 1.0 * a["csc_roi_pos"] / roi,
            int(a["csc_roi_neg"] / m), 1.0 * a["csc_roi_neg"] / roi, int(a["csc_roi_zero"] / m), 1.0 * a["csc_roi_zero"] / roi,
            int(t["num_img"]))
    return out


class CscStats:
    """The device-side `Statistic` of one CSCROIHeads (made by enable_csc_stats; the head engine calls forward()).  Owns the
    table, the scratch of drn_csc_stats and a small pool of pinned host copies.  cur_iter counts training forwards from
    start_iter, as the reference's own counter does - one per micro-step of an ITER_SIZE window, also for a step the anomaly
    guard skips: the statistics describe the forward.  After the forward with cur_iter % period == 0 and cur_iter <= max_iter
    the table is drained: a non-blocking copy to pinned memory, a stream-ordered re-zero and an event, no host sync.  collect()
    decodes what has completed; with output_dir set every decoded block is appended to <output_dir>/<prefix>csc.txt.
    blocks: every (iteration, text) handed out so far."""

    def __init__(self, K, max_iter, period=320, output_dir=None, prefix="", start_iter=0, device="cuda"):
        if int(period) < 1:
            raise DrnError("enable_csc_stats(period=%r): a positive number of training forwards" % (period,))
        ops.csc_batch_limits(1, K)
        self.K, self.max_iter, self.period = int(K), int(max_iter), int(period)
        self.cur_iter = int(start_iter)
        self.path = None if output_dir is None else os.path.join(output_dir, prefix + "csc.txt")
        self.table = torch.zeros((ops.csc_stats_words(K),), dtype=torch.int64, device=device)
        self.scratch = torch.empty((ops.csc_stats_scratch_words(ops.CSC_MAX_IMAGES, K),), dtype=torch.int64, device=device)
        self.blocks = []
        self._pending, self._free = [], []  # drains under way (iteration, host copy, event); host copies to use again
        self._last = None                   # iteration of the last counted forward that no drain has taken yet

    # ---- device side: what the head engine calls once W is final -----------------------------------------------------------
    def forward(self, scores, W, img_off, n_img, onehot, slots, launch=True):
        """one training forward: the step's launch pair on the current stream (launch=False past CSC_MAX_ITER: W is None there
        and the reference prints nothing either), then the reference's LogIterStats rule"""
        if launch:
            ops.csc_stats(scores, W, img_off, n_img, onehot, slots, self.table, self.scratch)
        it = self._last = self.cur_iter
        self.cur_iter += 1
        if it % self.period == 0 and it <= self.max_iter:
            self.drain(it)
        elif self._pending:
            self.collect()

    # ---- host side -------------------------------------------------------------------------------------------------------
    def drain(self, iteration=None):
        """copy the table to pinned memory and re-zero it, both on the CURRENT stream - the one the heads run on, so the copy
        sees whole forwards only - and an event behind them.  The block is labelled `iteration` (default: the last forward)."""
        it = self._last if iteration is None else int(iteration)
        host = self._free.pop() if self._free else torch.zeros_like(self.table, device="cpu")
        if self.table.is_cuda and not host.is_pinned():
            host = host.pin_memory()
        host.copy_(self.table, non_blocking=True)
        self.table.zero_()
        ev = None
        if self.table.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
        self._pending.append((it, host, ev))
        self._last = None

    def collect(self, wait=False):
        """-> [(iteration, table), ...]: every drain whose copy has completed, oldest first (wait=True: after synchronising the
        drains' own events, nothing else).  table: decode_csc_stats' dict of numpy arrays.  Appends the blocks to csc.txt."""
        out = []
        while self._pending:
            it, host, ev = self._pending[0]
            if ev is not None:
                if wait:
                    ev.synchronize()
                elif not ev.query():
                    break
            self._pending.pop(0)
            out.append((it, decode_csc_stats(host.numpy(), self.K)))
            self._free.append(host)
        for it, table in out:
            text = self.format(table, it)
            self.blocks.append((it, text))
            if self.path is not None:
                os.makedirs(os.path.dirname(self.path) or ".", exist_ok=True)
                with open(self.path, "a") as f:
                    f.write(text + "\n")
        return out

    def flush(self):
        """drain what the forwards since the last drain have counted (a block labelled with the last forward's iteration; nothing
        when there was none) and wait for every copy under way -> collect(wait=True)"""
        if self._last is not None:
            self.drain()
        return self.collect(wait=True)

    format = staticmethod(format_csc_stats)
