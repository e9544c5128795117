"""PASCAL VOC detection evaluation (second half): turns the detector's / the TTA wrapper's outputs
into AP and CorLoc, behind the reference's names: `PascalVOCDetectionEvaluator`, `voc_ap`, `voc_eval`,
`voc_eval_corloc`, `parse_rec` (detectron2/evaluation/pascal_voc_evaluation.py:21-180, :182-234, :237-350, :353-447;
the CorLoc metric is this fork's addition for weakly supervised detection).

Same arithmetic, different plumbing: predictions stay in memory (the reference writes one text file per class and reads
it back); they still go through the reference's text quantisation (score %.3f, box %.1f after the +1 shift of
xmin / ymin, :58-66) because the ranking and the overlaps are computed on those rounded numbers.  Ground truth is read
from VOC XML files or handed over as {image_id: [(class name, difficult, [xmin, ymin, xmax, ymax])]}.
Pinned by tests/golden/voc_eval.npz (the reference's functions on a synthetic annotation set).
`PascalVOCDetectionEvaluator(..., device="cuda")` computes the same numbers on the device (ops.voc_match /
ops.voc_accumulate, csrc/voceval.hip): the quantisation by formula, ties in processing order.

COCO box AP: `COCOEvaluator` (detectron2/evaluation/coco_evaluation.py:33-306, bbox only) and `instances_to_coco_json`
(:308-367).  The reference hands its predictions to COCOeval_opt, whose two expensive stages are native C++
(detectron2/layers/csrc/cocoeval/cocoeval.cpp); here both run on the device (ops.coco_match / ops.coco_accumulate,
csrc/cocoeval.hip) and the predictions never leave it before the three result arrays are read back.  Pinned by
tests/golden/coco_eval.npz (the unmodified C++ on synthetic, tie-heavy annotation sets).

Box-proposal recall: `ProposalRecallEvaluator` / `evaluate_box_proposals`, the reference's box_proposals task
(coco_evaluation.py:200-237, :372-480: AR@k by area), matched on the device (ops.proposal_recall, csrc/proprecall.hip;
DESIGN 4.17); `COCOEvaluator` hands outputs that carry "proposals" to it.  Pinned by tests/golden/proposal_recall.npz."""
import contextlib
import json
import os
import xml.etree.ElementTree as ET
from collections import OrderedDict, defaultdict

import numpy as np

__all__ = ["PascalVOCDetectionEvaluator", "parse_rec", "voc_ap", "voc_eval", "voc_eval_corloc", "format_prediction",
           "COCOEvaluator", "instances_to_coco_json", "coco_params", "coco_summarize", "derive_coco_results",
           "inference_on_dataset", "inference_context", "DatasetEvaluators", "ProposalRecallEvaluator",
           "evaluate_box_proposals", "proposal_recall_key", "PROPOSAL_AREAS"]


# ---- the dataset loop (detectron2/evaluation/evaluator.py:64-200) ------------------------------------------------------

class DatasetEvaluators:
    """Several evaluators behind one reset() / process() / evaluate(): every call goes to each of them in turn; evaluate()
    merges their result dicts (a key that two of them return is an error; a None result - not the main process - adds
    nothing)."""

    def __init__(self, evaluators):
        self._evaluators = list(evaluators)

    def reset(self):
        for ev in self._evaluators:
            ev.reset()

    def process(self, inputs, outputs):
        for ev in self._evaluators:
            ev.process(inputs, outputs)

    def evaluate(self):
        merged = OrderedDict()
        for ev in self._evaluators:
            res = ev.evaluate()
            for key, val in (res or {}).items():
                assert key not in merged, "Different evaluators produce results with the same key {}".format(key)
                merged[key] = val
        return merged


@contextlib.contextmanager
def inference_context(model):
    """The model in eval mode inside the block, its previous mode afterwards - also when the block raises."""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


def inference_on_dataset(model, data_loader, evaluator):
    """evaluator.reset(); evaluator.process(inputs, model(inputs)) for every element of data_loader with the model in eval mode
    and without autograd; the result of evaluator.evaluate(), {} where that is None (not the main process).  evaluator=None
    only runs the model.  The reference's timing / ETA log lines are not rebuilt - they synchronise after every image.
    Whatever the model returns goes to process() as it is: a padded model (GeneralizedRCNNWithTTAAVG(padded=True), or a wrapper
    around model.inference(padded=True)) with a device evaluator makes a loop in which nothing between reset() and evaluate()
    reads the device, so the host prepares image i+1 while image i's kernels run."""
    import torch

    if evaluator is None:
        evaluator = DatasetEvaluators([])
    evaluator.reset()
    with inference_context(model), torch.no_grad():
        for inputs in data_loader:
            evaluator.process(inputs, model(inputs))
    results = evaluator.evaluate()
    return {} if results is None else results


def _is_padded(outputs):
    return hasattr(outputs, "to_outputs") and hasattr(outputs, "count")


def _padded_block(index, inputs, outputs):
    """process() of a DetectionBatch on the device path: the blocks are kept as they are (no read of the count)"""
    import torch

    if len(inputs) != len(outputs):
        raise ValueError("%d inputs for a DetectionBatch of %d images" % (len(inputs), len(outputs)))
    if outputs.boxes.dtype != torch.float32 or outputs.scores.dtype != torch.float32:
        raise TypeError("DetectionBatch blocks are float32, got %s / %s" % (outputs.boxes.dtype, outputs.scores.dtype))
    return ("padded", outputs.boxes, outputs.scores, outputs.classes, outputs.count, list(index))


def _entries_in_order(ev):
    """the per-image entries and the padded blocks of an evaluator, interleaved in processing order"""
    out, at = [], 0
    for pos, block in ev._padded:
        out += [("list", ev._boxes[k], ev._scores[k], ev._classes[k], ev._images[k]) for k in range(at, pos)]
        out.append(block)
        at = pos
    out += [("list", ev._boxes[k], ev._scores[k], ev._classes[k], ev._images[k]) for k in range(at, len(ev._boxes))]
    return out


def _pack_entries(entries, device):
    """The processed predictions in processing order, packed on the device: boxes [n, 4] f32, scores [n] f32, classes [n] i32,
    image index [n] i32.  `entries` mixes ("list", boxes, scores, classes, image) of one image each and padded blocks
    ("padded", boxes, scores, classes, count, images); each run of consecutive padded blocks is packed by ONE
    ops.detections_compact and costs one 4-byte read of its n."""
    import torch

    from . import ops

    parts, i = [], 0
    while i < len(entries):
        j = i
        while j < len(entries) and entries[j][0] == entries[i][0]:
            j += 1
        run = entries[i:j]
        if run[0][0] == "list":
            counts = torch.tensor([e[1].shape[0] for e in run])
            img = torch.repeat_interleave(torch.tensor([e[4] for e in run], dtype=torch.int32), counts).to(device)
            parts.append((torch.cat([e[1].float().reshape(-1, 4) for e in run]), torch.cat([e[2].float() for e in run]),
                          torch.cat([e[3] for e in run]).to(torch.int32), img))
        else:
            topk = max(e[2].shape[1] for e in run)

            def pad(t, fill):  # blocks of different capacity (evaluations that mix models): widen to the largest
                if t.shape[1] == topk:
                    return t
                wide = t.new_full((t.shape[0], topk) + tuple(t.shape[2:]), fill)
                wide[:, : t.shape[1]] = t
                return wide

            images = torch.tensor([v for e in run for v in e[5]], dtype=torch.int32).to(device, non_blocking=True)
            ob, os_, oc, oi, n = ops.detections_compact(torch.cat([pad(e[1], 0) for e in run]), torch.cat([pad(e[2], 0) for e in run]),
                                                        torch.cat([pad(e[3], -1) for e in run]).to(torch.int32),
                                                        torch.cat([e[4] for e in run]).to(torch.int32), images)
            n = int(n.item())  # the one extra read of evaluate()
            parts.append((ob[:n], os_[:n], oc[:n], oi[:n]))
        i = j
    if len(parts) == 1:
        return parts[0]
    return tuple(torch.cat([p[k] for p in parts]) for k in range(4))


def parse_rec(filename):
    """VOC XML -> [(name, difficult, [xmin, ymin, xmax, ymax])]"""
    out = []
    for obj in ET.parse(filename).findall("object"):
        bb = obj.find("bndbox")
        out.append((obj.find("name").text, int(obj.find("difficult").text),
                    [int(bb.find(k).text) for k in ("xmin", "ymin", "xmax", "ymax")]))
    return out


def format_prediction(image_id, score, box):
    """the line PascalVOCDetectionEvaluator.process writes (:58-66): 1-based xmin / ymin, 3 / 1 decimals"""
    xmin, ymin, xmax, ymax = box
    xmin += 1
    ymin += 1
    return f"{image_id} {score:.3f} {xmin:.1f} {ymin:.1f} {xmax:.1f} {ymax:.1f}"


def voc_ap(rec, prec, use_07_metric=False):
    if use_07_metric:  # 11-point interpolation of VOC07
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap = ap + p / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def _class_gt(annos, classname):
    gt, npos, npos_im = {}, 0, 0
    for iid, objs in annos.items():
        R = [o for o in objs if o[0] == classname]
        difficult = np.array([o[1] for o in R]).astype(bool)
        gt[iid] = {"bbox": np.array([o[2] for o in R]), "difficult": difficult, "det": [False] * len(R)}
        npos += int(sum(~difficult))
        if len(R) > 0:
            npos_im += min(1, int(sum(~difficult)))
    return gt, npos, npos_im


def _ranked(lines):
    split = [x.strip().split(" ") for x in lines]
    ids = [x[0] for x in split]
    conf = np.array([float(x[1]) for x in split])
    BB = np.array([[float(z) for z in x[2:]] for x in split]).reshape(-1, 4)
    order = np.argsort(-conf)
    return [ids[k] for k in order], BB[order, :]


def _max_overlap(bb, BBGT):
    """VOC devkit IoU with the +1 pixel convention; (-inf, -1) when the image has no box of the class"""
    if BBGT.size == 0:
        return -np.inf, -1
    iw = np.maximum(np.minimum(BBGT[:, 2], bb[2]) - np.maximum(BBGT[:, 0], bb[0]) + 1.0, 0.0)
    ih = np.maximum(np.minimum(BBGT[:, 3], bb[3]) - np.maximum(BBGT[:, 1], bb[1]) + 1.0, 0.0)
    inters = iw * ih
    uni = ((bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + (BBGT[:, 2] - BBGT[:, 0] + 1.0) * (BBGT[:, 3] - BBGT[:, 1] + 1.0)
           - inters)
    ov = inters / uni
    return np.max(ov), int(np.argmax(ov))


def voc_eval(lines, annos, classname, ovthresh=0.5, use_07_metric=False):
    """lines: prediction lines of this class (format_prediction); annos: {image_id: [(name, difficult, bbox)]}.
    Returns (rec, prec, ap) like the reference's voc_eval (:237-350)."""
    gt, npos, _ = _class_gt(annos, classname)
    ids, BB = _ranked(lines)
    nd = len(ids)
    tp, fp = np.zeros(nd), np.zeros(nd)
    for d in range(nd):
        R = gt[ids[d]]
        ovmax, jmax = _max_overlap(BB[d, :].astype(float), R["bbox"].astype(float))
        if ovmax > ovthresh:
            if not R["difficult"][jmax]:
                if not R["det"][jmax]:
                    tp[d] = 1.0
                    R["det"][jmax] = 1
                else:
                    fp[d] = 1.0
        else:
            fp[d] = 1.0
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    rec = tp / float(npos) if npos > 0 else np.zeros_like(tp)  # no object of this class anywhere: recall 0, AP 0
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap(rec, prec, use_07_metric)


def voc_eval_corloc(lines, annos, classname, ovthresh=0.5, use_07_metric=False):
    """CorLoc (:353-447): fraction of images containing the class whose top-ranked detection of that class hits"""
    gt, _, npos_im = _class_gt(annos, classname)
    if len(lines) == 0 or npos_im == 0:  # (the reference divides by zero for a class that no image contains)
        return 0.0
    ids, BB = _ranked(lines)
    hit, miss = [], []
    for d in range(len(ids)):
        if ids[d] in hit or ids[d] in miss:
            continue
        R = gt[ids[d]]
        if all(R["difficult"]):
            continue
        ovmax, _ = _max_overlap(BB[d, :].astype(float), R["bbox"].astype(float))
        (hit if ovmax > ovthresh else miss).append(ids[d])
    return 1.0 * len(hit) / npos_im


class PascalVOCDetectionEvaluator:
    """reset() / process(inputs, outputs) / evaluate() like the reference's evaluator.  `annotations` is either the
    dict described above or None, in which case `dirname/Annotations/{id}.xml` of the ids listed in
    `dirname/ImageSets/Main/{split}.txt` are parsed.

    `device=None` is the host path: process() copies every image's predictions to the host and formats the reference's
    text lines, evaluate() runs voc_eval / voc_eval_corloc.  With a device ("cuda") the evaluator stays on it: process()
    keeps the prediction tensors and never synchronises; evaluate() concatenates them, uploads the ground truth, runs
    ops.voc_match / ops.voc_accumulate (csrc/voceval.hip) and reads `ap` / `corloc` back, its only synchronisation.  The
    device path differs from the host path in what it defines and what it refuses:
      * equal quantised ("%.3f") scores of a class rank in processing order - process() call order, then row order
        (the line order of the reference's per-class file).  The host path's np.argsort is not stable, so on ties its
        result is not a function of its inputs; without ties the two paths agree bit for bit (area AP: to summation order);
      * boxes and scores must be float32 or narrower (fp64 raises TypeError: the exact quantisation needs a 24-bit
        significand) and finite - the inference tail never emits a non-finite score, its `score > thresh` drops NaN;
      * predicted classes must lie in [0, len(class_names));
      * an unknown image_id raises ValueError in process() (host path: KeyError in evaluate());
      * at most ops.VOC_MAX_GT ground-truth boxes per (image, class): evaluate() raises DrnError beyond.
    `gather`: host path: callable(list-per-class dict) -> list of such dicts (one per rank); device path: callable(dict of
    this rank's host arrays) -> list of such dicts in rank order; both: None on every process but the main one."""

    def __init__(self, class_names, dirname=None, split="test", year=2007, annotations=None, gather=None, device=None):
        assert year in (2007, 2012), year
        self._class_names, self._is_2007 = list(class_names), year == 2007
        if annotations is None:
            with open(os.path.join(dirname, "ImageSets", "Main", split + ".txt")) as f:
                ids = [x.strip() for x in f.readlines()]
            annotations = {i: parse_rec(os.path.join(dirname, "Annotations", i + ".xml")) for i in ids}
        self._annos = annotations
        self._gather = gather  # None = single process
        self._device, self._mark = device, None
        if device is not None:
            self._index_ground_truth()
        self.reset()

    def _index_ground_truth(self):
        """ground truth grouped by (image, class) pair - images in annotation-dict order, annotation order inside a pair -
        with the pairs' offsets, and per class npos / npos_im as _class_gt counts them"""
        self._img_ids = list(self._annos)
        self._img_index = {iid: i for i, iid in enumerate(self._img_ids)}
        cls_index = {name: k for k, name in enumerate(self._class_names)}
        I, K = len(self._img_ids), len(self._class_names)
        objs = [(i * K + cls_index[o[0]], o[1], o[2]) for i, iid in enumerate(self._img_ids) for o in self._annos[iid]
                if o[0] in cls_index]
        pair = np.array([o[0] for o in objs], np.int64)
        o = np.argsort(pair, kind="stable")
        diff = np.array([1 if objs[j][1] else 0 for j in o], np.uint8)
        count = np.bincount(pair, minlength=I * K)
        easy = np.bincount(pair[o], weights=1 - diff.astype(np.float64), minlength=I * K).astype(np.int64).reshape(I, K)
        self._gt = dict(box=np.array([objs[j][2] for j in o], np.float64).reshape(-1, 4), diff=diff,
                        off=np.concatenate([[0], np.cumsum(count)]).astype(np.int32),
                        npos=easy.sum(0).astype(np.int32), npos_im=(easy > 0).sum(0).astype(np.int32))

    def reset(self):
        self._predictions = defaultdict(list)
        self._boxes, self._scores, self._classes, self._images = [], [], [], []
        self._padded = []  # (number of per-image entries in front of it, padded block): DetectionBatch outputs, device path

    def process(self, inputs, outputs):
        """outputs: a list of {"instances": Instances} or a structures.DetectionBatch (both may be mixed in one evaluation;
        processing order defines the tie order either way).  On the device path a DetectionBatch is kept as padded blocks
        without a read of its count; evaluate() packs them with ops.detections_compact, which costs one extra 4-byte read
        of n per run of consecutive padded blocks.  The host path converts it with to_outputs()."""
        if self._device is not None:
            return self._process_device(inputs, outputs)
        if _is_padded(outputs):
            outputs = outputs.to_outputs()
        for inp, out in zip(inputs, outputs):
            inst = out["instances"]
            boxes = inst.pred_boxes.tensor.detach().cpu().numpy()
            for box, score, cls in zip(boxes, inst.scores.tolist(), inst.pred_classes.tolist()):
                self._predictions[cls].append(format_prediction(inp["image_id"], score, box))

    def _process_device(self, inputs, outputs):
        import torch

        narrow = (torch.float32, torch.float16, torch.bfloat16)
        if _is_padded(outputs):
            for inp in inputs:
                if inp["image_id"] not in self._img_index:
                    raise ValueError("image_id %r is not in the annotations" % (inp["image_id"],))
            self._padded.append((len(self._boxes), _padded_block([self._img_index[inp["image_id"]] for inp in inputs],
                                                                 inputs, outputs)))
            return
        for inp, out in zip(inputs, outputs):
            if inp["image_id"] not in self._img_index:
                raise ValueError("image_id %r is not in the annotations" % (inp["image_id"],))
            inst = out["instances"]
            box, score = inst.pred_boxes.tensor.detach(), inst.scores.detach()
            if box.dtype not in narrow or score.dtype not in narrow:
                raise TypeError("PascalVOCDetectionEvaluator(device=...): boxes and scores must be float32 or narrower, got "
                                "%s / %s" % (box.dtype, score.dtype))
            self._boxes.append(box)
            self._scores.append(score)
            self._classes.append(inst.pred_classes.detach())
            self._images.append(self._img_index[inp["image_id"]])

    def evaluate(self):
        if self._device is not None:
            return self._evaluate_device()
        parts = self._gather(self._predictions) if self._gather is not None else [self._predictions]
        if parts is None:
            return None  # not the main process
        preds = defaultdict(list)
        for part in parts:
            for c, lines in part.items():
                preds[c].extend(lines)
        aps, cls_ = defaultdict(list), defaultdict(list)
        for ci, name in enumerate(self._class_names):
            lines = preds.get(ci, [])
            for thr in range(50, 100, 5):
                ap = voc_eval(lines, self._annos, name, thr / 100.0, self._is_2007)[2] if lines else 0.0
                aps[thr].append(ap * 100)
                cls_[thr].append(voc_eval_corloc(lines, self._annos, name, thr / 100.0, self._is_2007) * 100)
        return self._results(aps, cls_)

    def _results(self, aps, cls_):
        ret = OrderedDict()
        m = {t: np.mean(x) for t, x in aps.items()}
        ret["bbox"] = {"AP": np.mean(list(m.values())), "AP50": m[50], "AP75": m[75]}
        m = {t: np.mean(x) for t, x in cls_.items()}
        ret["bbox CorLoc"] = {"CL": np.mean(list(m.values())), "CL50": m[50], "CL75": m[75]}
        ret["per_class"] = {"AP50": dict(zip(self._class_names, aps[50])), "CL50": dict(zip(self._class_names, cls_[50]))}
        return ret

    def _local(self):
        """this rank's predictions, concatenated on the device in processing order: boxes [n, 4] f32 XYXY, scores [n] f32
        (both widened exactly), classes, image index"""
        import torch

        if self._padded:
            return _pack_entries(_entries_in_order(self), self._padded[0][1][1].device)
        dev = self._boxes[0].device if self._boxes else torch.device(self._device)
        if not self._boxes:
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            return z((0, 4), torch.float32), z((0,), torch.float32), z((0,), torch.int32), z((0,), torch.int32)
        counts = torch.tensor([b.shape[0] for b in self._boxes])
        img = torch.repeat_interleave(torch.tensor(self._images, dtype=torch.int32), counts).to(dev)
        return (torch.cat([b.float().reshape(-1, 4) for b in self._boxes]), torch.cat([s.float() for s in self._scores]),
                torch.cat(self._classes).to(torch.int32), img)

    def _evaluate_device(self):
        import torch

        from . import ops
        from ._cabi import DrnError

        box, score, cls, img = self._local()
        if self._gather is not None:
            parts = self._gather({"boxes": box.cpu().numpy(), "scores": score.cpu().numpy(), "classes": cls.cpu().numpy(),
                                  "images": img.cpu().numpy()})
            if parts is None:
                return None  # not the main process
            dev = torch.device(self._device)
            up = lambda k, dt: torch.from_numpy(np.concatenate([np.asarray(p[k]) for p in parts])).to(dt).to(dev)
            box, score = up("boxes", torch.float32).reshape(-1, 4), up("scores", torch.float32)
            cls, img = up("classes", torch.int32), up("images", torch.int32)
        dev = box.device
        K, gt = len(self._class_names), self._gt
        ngt = np.diff(gt["off"])
        max_gt = int(ngt.max()) if ngt.size else 0
        if max_gt > ops.VOC_MAX_GT:
            worst = int(ngt.argmax())
            raise DrnError("PascalVOCDetectionEvaluator: image %s / class %s has %d ground-truth boxes; the device matcher "
                           "holds at most %d per (image, class) pair" % (self._img_ids[worst // K],
                                                                         self._class_names[worst % K], max_gt, ops.VOC_MAX_GT))
        thrs = list(range(50, 100, 5))
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
        iou_thr = t(np.array([thr / 100.0 for thr in thrs], np.float64), torch.float64)
        rec_thr = t(np.arange(0.0, 1.1, 0.1), torch.float64)  # voc_ap's own expression: not i / 10
        margs = (box.contiguous(), score.contiguous(), (img * K + cls).contiguous(), t(gt["box"], torch.float64),
                 t(gt["diff"], torch.uint8), t(gt["off"], torch.int32), K, max_gt, iou_thr)
        npos, npos_im = t(gt["npos"], torch.int32), t(gt["npos_im"], torch.int32)
        mark = self._mark or (lambda name: None)  # tools/voc_eval_bench.py records a HIP event per stage here
        mark("start")
        m = ops.voc_match(*margs, stages=1)
        mark("quantise + rank")
        ops.voc_match(*margs, stages=2, out=m)
        mark("match")
        acc = ops.voc_accumulate(m["tp"], m["fp"], m["cls_off"], m["hit"], npos, npos_im, len(thrs), rec_thr, self._is_2007)
        mark("accumulate")
        ap, corloc = acc["ap"].cpu().numpy(), acc["corloc"].cpu().numpy()  # the only sync
        mark("read-back")
        aps = {thr: [ap[ti, k] * 100 for k in range(K)] for ti, thr in enumerate(thrs)}
        cls_ = {thr: [corloc[ti, k] * 100 for k in range(K)] for ti, thr in enumerate(thrs)}
        return self._results(aps, cls_)


# ---- COCO box AP ------------------------------------------------------------------------------------------------------

def coco_params():
    """pycocotools' Params for iouType = 'bbox' (cocoeval.py), to the letter, in fp64: IoU thresholds, recall thresholds,
    maxDets, area ranges.  The kernels hard-code none of them."""
    return dict(iouThrs=np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
                recThrs=np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
                maxDets=[1, 10, 100],
                areaRng=[[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]])


def coco_summarize(precision, recall, params=None):
    """the 12 `stats` of pycocotools' COCOeval.summarize: the mean over the entries > -1, -1 if there are none"""
    p = params or coco_params()
    iou, last = np.asarray(p["iouThrs"]), len(p["maxDets"]) - 1

    def one(ap, thr=None, a=0, m=last):
        s = precision if ap else recall
        if thr is not None:
            s = s[np.where(thr == iou)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))

    return np.array([one(1), one(1, .5), one(1, .75), one(1, a=1), one(1, a=2), one(1, a=3), one(0, m=0), one(0, m=1),
                     one(0), one(0, a=1), one(0, a=2), one(0, a=3)])


def derive_coco_results(stats, precision, class_names=None):
    """COCOEvaluator._derive_coco_results for 'bbox' (coco_evaluation.py:239-306): x 100, NaN for -1, per-category AP"""
    metrics = ["AP", "AP50", "AP75", "APs", "APm", "APl"]
    results = {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(metrics)}
    if class_names is None or len(class_names) <= 1:
        return results
    assert len(class_names) == precision.shape[2]
    for idx, name in enumerate(class_names):
        pr = precision[:, :, idx, 0, -1]  # area range "all", the largest maxDets
        pr = pr[pr > -1]
        results["AP-" + "{}".format(name)] = float(np.mean(pr) * 100) if pr.size else float("nan")
    return results


def instances_to_coco_json(instances, img_id):
    """coco_evaluation.py:308-367 for boxes: [{"image_id", "category_id" (the contiguous class), "bbox" (XYWH, converted in
    float32), "score"}] for writing result files"""
    if len(instances) == 0:
        return []
    b = instances.pred_boxes.tensor.detach().cpu().numpy().astype(np.float32)
    xywh = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).tolist()
    scores, classes = instances.scores.tolist(), instances.pred_classes.tolist()
    return [{"image_id": img_id, "category_id": classes[k], "bbox": xywh[k], "score": scores[k]} for k in range(len(scores))]


class COCOEvaluator:
    """reset() / process(inputs, outputs) / evaluate() like the reference's COCOEvaluator, box AP only (useCats = 1).

    `annotations`: a COCO-format dict or the path of a json file; `images[*].id`, `categories[*].{id, name}` and
    `annotations[*].{image_id, category_id, bbox, area, iscrowd}` are used.  Every image of the file counts, with or
    without detections.  The predicted contiguous class c stands for the c-th smallest dataset category id (detectron2's
    thing_dataset_id_to_contiguous_id); `class_names` defaults to the categories' names in that order.
    `gather`: callable(per-rank dict of host arrays) -> list of such dicts on the main process, None elsewhere.

    process() keeps the predictions as device tensors and never synchronises; evaluate() concatenates them, converts the
    boxes XYXY -> XYWH in float32 (coco_evaluation.py:323-325) and widens them to fp64, uploads the ground truth once,
    runs order -> match -> order -> accumulate on the device and reads `precision` / `recall` / `scores` back."""

    def __init__(self, annotations, class_names=None, gather=None, device="cuda"):
        if not isinstance(annotations, dict):
            with open(annotations) as f:
                annotations = json.load(f)
        self._img_ids = sorted(int(im["id"]) for im in annotations["images"])
        cats = sorted(annotations["categories"], key=lambda c: int(c["id"]))
        self._cat_ids = [int(c["id"]) for c in cats]
        self._class_names = list(class_names) if class_names is not None else [str(c.get("name", c["id"])) for c in cats]
        self._img_index = {iid: i for i, iid in enumerate(self._img_ids)}
        cat_index = {cid: k for k, cid in enumerate(self._cat_ids)}
        I, K = len(self._img_ids), len(self._cat_ids)
        anns = [a for a in annotations["annotations"] if int(a["image_id"]) in self._img_index
                and int(a["category_id"]) in cat_index]
        pair = np.array([self._img_index[int(a["image_id"])] * K + cat_index[int(a["category_id"])] for a in anns], np.int64)
        o = np.argsort(pair, kind="stable")  # grouped by (image, category); annotation order inside a pair
        self._gt = dict(
            box=np.array([anns[j]["bbox"] for j in o], np.float64).reshape(-1, 4),
            area=np.array([anns[j]["area"] for j in o], np.float64),
            crowd=np.array([1 if anns[j].get("iscrowd", 0) else 0 for j in o], np.uint8),
            off=np.concatenate([[0], np.cumsum(np.bincount(pair, minlength=I * K))]).astype(np.int32))
        self._gather, self._device = gather, device
        self._annotations = annotations  # for the box_proposals task, indexed when the first such output arrives
        self.params = coco_params()
        self.stats, self.eval, self._mark = None, None, None
        self.reset()

    def reset(self):
        self._boxes, self._scores, self._classes, self._images = [], [], [], []
        self._padded = []  # (number of per-image entries in front of it, padded block): DetectionBatch outputs
        self._proposals = None  # the ProposalRecallEvaluator of outputs that carry "proposals"

    def process(self, inputs, outputs):
        """outputs: a list of {"instances": Instances} or a structures.DetectionBatch, which is kept as padded blocks without
        a read of its count (both may be mixed; evaluate() packs the blocks with ops.detections_compact at the price of one
        extra 4-byte read of n per run of consecutive padded blocks)."""
        if _is_padded(outputs):
            for inp in inputs:
                if int(inp["image_id"]) not in self._img_index:
                    raise ValueError("image_id %r is not in the annotation file" % (inp["image_id"],))
            self._padded.append((len(self._boxes), _padded_block([self._img_index[int(inp["image_id"])] for inp in inputs],
                                                                 inputs, outputs)))
            return
        for inp, out in zip(inputs, outputs):
            iid = int(inp["image_id"])
            if iid not in self._img_index:
                raise ValueError("image_id %r is not in the annotation file" % (inp["image_id"],))
            if "proposals" in out:  # coco_evaluation.py:119-120: the box_proposals task
                if self._proposals is None:
                    self._proposals = ProposalRecallEvaluator(self._annotations, gather=self._gather, device=self._device)
                self._proposals.process([inp], [out])
                if "instances" not in out:
                    continue
            inst = out["instances"]
            self._boxes.append(inst.pred_boxes.tensor.detach())
            self._scores.append(inst.scores.detach())
            self._classes.append(inst.pred_classes.detach())
            self._images.append(self._img_index[iid])

    def _local(self):
        """this rank's predictions, concatenated on the device: boxes [n, 4] f32 XYXY, scores [n] f32, classes, image index"""
        import torch

        if self._padded:
            return _pack_entries(_entries_in_order(self), self._padded[0][1][1].device)
        dev = self._boxes[0].device if self._boxes else torch.device(self._device)
        if not self._boxes:
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            return z((0, 4), torch.float32), z((0,), torch.float32), z((0,), torch.int32), z((0,), torch.int32)
        counts = torch.tensor([b.shape[0] for b in self._boxes])
        img = torch.repeat_interleave(torch.tensor(self._images, dtype=torch.int32), counts).to(dev)
        return (torch.cat(self._boxes).float().reshape(-1, 4), torch.cat(self._scores).float(),
                torch.cat(self._classes).to(torch.int32), img)

    def evaluate(self):
        """OrderedDict(bbox=...) as ever; when outputs with "proposals" were processed, box_proposals comes in front
        (coco_evaluation.py:145-148) and bbox is there if any "instances" were processed too."""
        if self._proposals is None:
            return self._evaluate_instances()
        res = self._proposals.evaluate()
        if self._boxes or self._padded:
            bbox = self._evaluate_instances()
            if res is not None and bbox is not None:
                res.update(bbox)
        return res

    def _evaluate_instances(self):
        import torch

        from . import ops
        from ._cabi import DrnError

        box, score, cls, img = self._local()
        if self._gather is not None:
            parts = self._gather({"boxes": box.cpu().numpy(), "scores": score.cpu().numpy(), "classes": cls.cpu().numpy(),
                                  "images": img.cpu().numpy()})
            if parts is None:
                return None  # not the main process
            dev = torch.device(self._device)
            up = lambda k, dt: torch.from_numpy(np.concatenate([np.asarray(p[k]) for p in parts])).to(dt).to(dev)
            box, score = up("boxes", torch.float32).reshape(-1, 4), up("scores", torch.float32)
            cls, img = up("classes", torch.int32), up("images", torch.int32)
        dev = box.device
        I, K, gt, p = len(self._img_ids), len(self._cat_ids), self._gt, self.params
        ngt = np.diff(gt["off"])
        max_gt = int(ngt.max()) if ngt.size else 0
        if max_gt > ops.COCO_MAX_GT:
            worst = int(ngt.argmax())
            raise DrnError("COCOEvaluator: image %d / category %d has %d ground-truth boxes; the device matcher holds at most "
                           "%d per (image, category) pair" % (self._img_ids[worst // K], self._cat_ids[worst % K], max_gt,
                                                              ops.COCO_MAX_GT))
        # coco_evaluation.py:323-325: XYXY -> XYWH in float32; the json round trip then makes python floats (fp64) of them
        xywh = torch.stack([box[:, 0], box[:, 1], box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]], 1).double().contiguous()
        pair = (img * K + cls).contiguous()
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
        iou_thr, rec_thr = t(p["iouThrs"], torch.float64), t(p["recThrs"], torch.float64)
        area = t(np.array(p["areaRng"], np.float64), torch.float64)
        max_dets = t(np.array(p["maxDets"], np.int32), torch.int32)
        mark = self._mark or (lambda name: None)  # tools/coco_eval_bench.py records a HIP event per stage here
        margs = (xywh, score.contiguous(), pair, t(gt["box"], torch.float64), t(gt["area"], torch.float64),
                 t(gt["crowd"], torch.uint8), t(gt["off"], torch.int32), K, max_gt, iou_thr, area)
        mark("start")
        m = ops.coco_match(*margs, max_det=int(p["maxDets"][-1]), stages=1)
        mark("sort (image, category)")
        ops.coco_match(*margs, max_det=int(p["maxDets"][-1]), stages=2, out=m)
        mark("match")
        aargs = (m["s_score"], m["s_cat"], m["s_rank"], m["dm"], m["di"], m["npig"], I, K, iou_thr.shape[0], max_dets, rec_thr)
        acc = ops.coco_accumulate(*aargs, stages=1)
        mark("sort (category)")
        ops.coco_accumulate(*aargs, stages=2, out=acc)
        mark("accumulate")
        precision, recall, scores = (acc[k].cpu().numpy() for k in ("precision", "recall", "scores"))  # the only sync
        mark("read-back")
        self.eval = {"params": p, "counts": [int(v) for v in precision.shape], "precision": precision, "recall": recall,
                     "scores": scores}
        self.stats = coco_summarize(precision, recall, p)
        return OrderedDict(bbox=derive_coco_results(self.stats, precision, self._class_names))


# ---- box-proposal recall (AR@k by area) -----------------------------------------------------------------------------------

# coco_evaluation.py:380-399, to the letter
PROPOSAL_AREAS = OrderedDict([("all", [0 ** 2, 1e5 ** 2]), ("small", [0 ** 2, 32 ** 2]), ("medium", [32 ** 2, 96 ** 2]),
                              ("large", [96 ** 2, 1e5 ** 2]), ("96-128", [96 ** 2, 128 ** 2]), ("128-256", [128 ** 2, 256 ** 2]),
                              ("256-512", [256 ** 2, 512 ** 2]), ("512-inf", [512 ** 2, 1e5 ** 2])])
_AREA_SUFFIX = {"all": "", "small": "s", "medium": "m", "large": "l"}  # :230; the other four: "[name]"


def proposal_recall_key(area, limit):
    """the reference's result key (:234): AR@100, ARs@100, ...; AR[96-128]@100 for the areas it never reports; @all = no cut"""
    return "AR%s@%s" % (_AREA_SUFFIX.get(area, "[%s]" % area), "all" if limit is None else "%d" % limit)


def _xywh_to_xyxy_f32(bbox):
    """BoxMode.convert of a python list (boxes.py:63,111-113): float32, one addition per far corner"""
    b = np.asarray(bbox, np.float32).reshape(-1, 4)
    return np.stack([b[:, 0], b[:, 1], b[:, 2] + b[:, 0], b[:, 3] + b[:, 1]], 1).astype(np.float32)


def _id_key(v):
    return v if isinstance(v, str) else int(v)


class ProposalRecallEvaluator:
    """The box_proposals task of the reference's COCOEvaluator (coco_evaluation.py:200-237 over _evaluate_box_proposals,
    :372-480): average recall of the proposals an output carries, per (area range, limit) pair, matched on the device
    (ops.proposal_recall, csrc/proprecall.hip).

    `annotations`: a COCO-format dict or the path of a json file; `images[*].id` and `annotations[*].{image_id, bbox, area,
    iscrowd}` are used (every category; crowd annotations are left out, :418).  `from_dataset_dicts` takes detectron2-format
    dicts instead.  `limits`: cuts of the per-image proposal list (None = all), `areas`: names of PROPOSAL_AREAS.
    `gather`: callable(per-rank dict of host arrays) -> list of such dicts on the main process, None elsewhere.

    process() keeps `outputs[i]["proposals"]` (`proposal_boxes` / `objectness_logits`, on the device or on the host) and
    never synchronises.  Only processed images take part, each as often as it was processed.  evaluate() uploads their
    ground truth once, runs every pair in one launch chain and reads back once; it returns
    OrderedDict(box_proposals={"AR@100": ..., "ARs@100": ..., ...}) with float(ar * 100) in the reference's key order, and
    leaves the reference's dict of every pair (ar, recalls, thresholds, gt_overlaps sorted, num_pos; CPU tensors, formed from
    the device's overlaps with the reference's torch expressions) in `self.results[(area, limit)]` and the device's integer
    counts in `self.counts[(area, limit)]`.  This package's definitions: equal logits keep their input order; among equal
    IoUs the first proposal and the first box win; a NaN logit is undefined.  An unknown image_id raises ValueError in
    process(); more than ops.PROPOSAL_MAX_GT boxes in an image or more than ops.PROPOSAL_MAX_PER_IMAGE proposals after the
    cut raise DrnError in evaluate() before anything is uploaded."""

    def __init__(self, annotations, limits=(100, 1000), areas=("all", "small", "medium", "large"), gather=None, device="cuda",
                 thresholds=None):
        if not isinstance(annotations, dict):
            with open(annotations) as f:
                annotations = json.load(f)
        per = OrderedDict((_id_key(im["id"]), []) for im in annotations["images"])
        for a in annotations["annotations"]:
            if a.get("iscrowd", 0) == 0 and _id_key(a["image_id"]) in per:
                per[_id_key(a["image_id"])].append(a)
        self._setup([(iid, _xywh_to_xyxy_f32([a["bbox"] for a in anns]), np.array([a["area"] for a in anns], np.float32))
                     for iid, anns in per.items()], limits, areas, gather, device, thresholds)

    @classmethod
    def from_dataset_dicts(cls, dataset_dicts, limits=(100, 1000), areas=("all", "small", "medium", "large"), gather=None,
                           device="cuda", thresholds=None):
        """detectron2-format dicts ({"image_id", "annotations": [{"bbox", "bbox_mode", "iscrowd"?, "area"?}]}), so that VOC
        works.  An annotation without "area" counts with w * h of its XYWH box in float32 (this package's definition)."""
        from .data import BoxMode

        records = []
        for r in dataset_dicts:
            boxes, areas_ = [], []
            for a in r.get("annotations", []):
                if a.get("iscrowd", 0) != 0:
                    continue
                mode = int(a.get("bbox_mode", BoxMode.XYXY_ABS))
                b = np.asarray(a["bbox"], np.float32).reshape(4)
                if mode == int(BoxMode.XYWH_ABS):
                    xyxy, wh = _xywh_to_xyxy_f32(b)[0], (b[2], b[3])
                elif mode == int(BoxMode.XYXY_ABS):
                    xyxy, wh = b, (b[2] - b[0], b[3] - b[1])
                else:
                    raise ValueError("bbox_mode %r is not supported" % (a["bbox_mode"],))
                boxes.append(xyxy)
                areas_.append(np.float32(a["area"]) if "area" in a else np.float32(wh[0]) * np.float32(wh[1]))
            records.append((_id_key(r["image_id"]), np.array(boxes, np.float32).reshape(-1, 4), np.array(areas_, np.float32)))
        self = cls.__new__(cls)
        self._setup(records, limits, areas, gather, device, thresholds)
        return self

    def _setup(self, records, limits, areas, gather, device, thresholds):
        for a in areas:
            assert a in PROPOSAL_AREAS, "Unknown area range: {}".format(a)
        self._limits = [None if l is None else int(l) for l in limits]
        assert self._limits and areas and all(l is None or l > 0 for l in self._limits)
        self._areas = list(areas)
        self._gt = {iid: (box, area) for iid, box, area in records}
        self._gather, self._device, self._thresholds, self._mark = gather, device, thresholds, None
        self.results, self.counts = None, None
        self.reset()

    def reset(self):
        self._boxes, self._logits, self._images = [], [], []

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            iid = _id_key(inp["image_id"])
            if iid not in self._gt:
                raise ValueError("image_id %r is not in the annotations" % (inp["image_id"],))
            prop = out["proposals"]
            self._boxes.append(prop.proposal_boxes.tensor.detach())
            self._logits.append(prop.objectness_logits.detach())
            self._images.append(iid)

    def process_proposal_file(self, proposal_file):
        """Feeds in a proposal file in the format data.load_proposals_into_dataset reads (a pickle, or the dict it holds:
        ids | indexes, boxes, objectness_logits | scores, bbox_mode?): the entries whose id is in the annotations, in file
        order, as host tensors.  Returns how many were fed."""
        import pickle

        import torch

        from .data import BoxMode

        proposals = proposal_file
        if not isinstance(proposals, dict):
            with open(proposal_file, "rb") as f:
                proposals = pickle.load(f, encoding="latin1")
        ids = proposals["ids"] if "ids" in proposals else proposals["indexes"]
        logits = proposals["objectness_logits"] if "objectness_logits" in proposals else proposals["scores"]
        mode = int(proposals["bbox_mode"]) if "bbox_mode" in proposals else int(BoxMode.XYXY_ABS)
        by_str = {str(k): k for k in self._gt}
        fed = 0
        for k, i in enumerate(ids):
            if str(i) not in by_str:
                continue
            boxes = np.asarray(proposals["boxes"][k], np.float32).reshape(-1, 4)
            if mode != int(BoxMode.XYXY_ABS):
                boxes = np.asarray(BoxMode.convert(boxes, mode, BoxMode.XYXY_ABS), np.float32)
            self._boxes.append(torch.from_numpy(np.ascontiguousarray(boxes)))
            self._logits.append(torch.from_numpy(np.ascontiguousarray(np.asarray(logits[k], np.float32).reshape(-1))))
            self._images.append(by_str[str(i)])
            fed += 1
        return fed

    def _refuse_over_cap(self, images, counts):
        from . import ops
        from ._cabi import DrnError

        for iid in images:
            if len(self._gt[iid][1]) > ops.PROPOSAL_MAX_GT:
                raise DrnError("ProposalRecallEvaluator: image %r has %d ground-truth boxes; the device matcher holds at most "
                               "%d per image" % (iid, len(self._gt[iid][1]), ops.PROPOSAL_MAX_GT))
        cut = None if None in self._limits else max(self._limits)
        kept = [c if cut is None else min(c, cut) for c in counts]
        if kept and max(kept) > ops.PROPOSAL_MAX_PER_IMAGE:
            worst = int(np.argmax(kept))
            raise DrnError("ProposalRecallEvaluator: image %r has %d proposals after the cut; the device matcher holds at most "
                           "%d per image" % (images[worst], kept[worst], ops.PROPOSAL_MAX_PER_IMAGE))
        return max(kept) if kept else 0

    def evaluate(self):
        import torch

        images, counts = list(self._images), [int(b.shape[0]) for b in self._boxes]
        if self._gather is None:
            max_prop = self._refuse_over_cap(images, counts)  # before anything is uploaded
        from . import ops

        dev = torch.device(self._device)
        mark = self._mark or (lambda name: None)  # tools/proposal_recall_bench.py records a HIP event per stage here
        mark("start")
        box = logit = None  # (an evaluation without a processed image touches no device)
        if self._gather is not None:
            host = lambda ts, shape: (torch.cat([t.float().reshape(shape).cpu() for t in ts]).numpy() if ts
                                      else np.zeros((0,) + shape[1:], np.float32))
            parts = self._gather({"boxes": host(self._boxes, (-1, 4)), "logits": host(self._logits, (-1,)),
                                  "counts": np.array(counts, np.int64), "images": images})
            if parts is None:
                return None  # not the main process
            images = [i for p in parts for i in p["images"]]
            counts = [int(c) for p in parts for c in np.asarray(p["counts"])]
            max_prop = self._refuse_over_cap(images, counts)
            if images:
                box = torch.from_numpy(np.concatenate([np.asarray(p["boxes"], np.float32).reshape(-1, 4) for p in parts])).to(dev)
                logit = torch.from_numpy(np.concatenate([np.asarray(p["logits"], np.float32).reshape(-1) for p in parts])).to(dev)
        elif self._boxes:
            # host-resident proposals (a proposal file) go up in one copy, device-resident ones stay where they are
            up = ((lambda t: t) if not any(b.is_cuda or s.is_cuda for b, s in zip(self._boxes, self._logits))
                  else (lambda t: t.to(dev, non_blocking=True)))
            box = torch.cat([up(b).float().reshape(-1, 4) for b in self._boxes]).to(dev).contiguous()
            logit = torch.cat([up(s).float().reshape(-1) for s in self._logits]).to(dev).contiguous()
        thr = (torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32) if self._thresholds is None
               else torch.as_tensor(self._thresholds, dtype=torch.float32).reshape(-1).cpu())  # :465-467
        A, L, T, I = len(self._areas), len(self._limits), int(thr.shape[0]), len(images)
        if I > 0:
            gt_box = np.concatenate([self._gt[i][0] for i in images]).astype(np.float32).reshape(-1, 4)
            gt_area = np.concatenate([self._gt[i][1] for i in images]).astype(np.float32)
            ngt = [len(self._gt[i][1]) for i in images]
            t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev, non_blocking=True)
            off = lambda n: np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
            args = (box, logit, t(off(counts), torch.int32), t(gt_box, torch.float32), t(gt_area, torch.float32),
                    t(off(ngt), torch.int32), t(np.array([PROPOSAL_AREAS[a] for a in self._areas], np.float32), torch.float32),
                    t(np.array([0 if l is None else l for l in self._limits], np.int32), torch.int32), thr.to(dev),
                    max(ngt), max_prop)
            mark("upload")
            m = ops.proposal_recall(*args, stages=1)
            mark("order")
            ops.proposal_recall(*args, stages=2, out=m)
            mark("match")
            G = gt_area.shape[0]
            flat = torch.cat([m["counts"].reshape(-1).view(torch.int32), m["num_pos"].view(torch.int32),
                              m["overlaps"].reshape(-1).view(torch.int32)]).cpu()  # one copy, the only sync
            mark("read-back")
            nc = 2 * A * L * T
            cnt = flat[:nc].view(torch.int64).reshape(A, L, T)
            num_pos = flat[nc: nc + 2 * A].view(torch.int64)
            overlaps = flat[nc + 2 * A:].view(torch.float32).reshape(A, L, G)
        else:
            overlaps, cnt, num_pos = torch.zeros(A, L, 0), torch.zeros(A, L, T, dtype=torch.int64), torch.zeros(A, dtype=torch.int64)
        self.results, self.counts, res = OrderedDict(), OrderedDict(), OrderedDict()
        for l, limit in enumerate(self._limits):
            for a, area in enumerate(self._areas):
                ov = overlaps[a, l]
                gt_overlaps, _ = torch.sort(ov[ov >= 0])  # :460-463 (-1 = not an entry)
                n = int(num_pos[a])
                recalls = torch.zeros_like(thr)
                for i, tv in enumerate(thr):  # :468-473
                    recalls[i] = (gt_overlaps >= tv).float().sum() / float(n)
                ar = recalls.mean()
                self.results[(area, limit)] = {"ar": ar, "recalls": recalls, "thresholds": thr, "gt_overlaps": gt_overlaps,
                                               "num_pos": n}
                self.counts[(area, limit)] = cnt[a, l].clone()
                res[proposal_recall_key(area, limit)] = float(ar.item() * 100)
        return OrderedDict(box_proposals=res)


def evaluate_box_proposals(proposals, ground_truth, thresholds=None, area="all", limit=None, device="cuda"):
    """_evaluate_box_proposals (coco_evaluation.py:372-480) on the device.  `proposals`: the reference's dataset_predictions,
    [{"image_id", "proposals": Instances}]; `ground_truth`: a COCO-format dict or json path (in the place of coco_api), a list
    of detectron2-format dataset dicts, or a ProposalRecallEvaluator's annotations in any form that class takes.  Returns the
    reference's dict - ar, recalls, thresholds, gt_overlaps (sorted), num_pos - as CPU tensors (num_pos: int)."""
    make = ProposalRecallEvaluator.from_dataset_dicts if isinstance(ground_truth, (list, tuple)) else ProposalRecallEvaluator
    ev = make(ground_truth, limits=(limit,), areas=(area,), device=device, thresholds=thresholds)
    ev.process(proposals, proposals)
    ev.evaluate()
    return ev.results[(area, limit)]
