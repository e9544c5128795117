"""Test-time augmentation of the WSL detector, behind the reference's names:
`DatasetMapperTTAAVG` and `GeneralizedRCNNWithTTAAVG` (projects/WSL/wsl/modeling/test_time_augmentation_avg.py:68-137,
:139-321) with the transforms they drive - ResizeShortestEdge (detectron2/data/transforms/augmentation_impl.py:155-175),
ResizeTransform (detectron2/data/transforms/transform.py:83-134), fvcore's HFlipTransform.

Split of work: the mapper (image resize through PIL for uint8 images exactly like the reference, flip, proposal boxes
scaled / flipped / clipped / filtered / top-k) is host-side data preparation, as in the reference.  Everything after it
stays on the GPU: one `model.inference` per augmentation, `drn_tta_accumulate` maps each augmentation's [R, 4K]
predictions back to the original image and folds them into the running box / score averages (the reference copies
them to the host and back for this), and `drn_detect_topk` runs the final score-threshold / NMS / top-k."""
import copy
import logging

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import ops
from .._cabi import DrnError
from ..structures import Boxes, DetectionBatch, Instances
from .roi_heads import padded_detections

__all__ = ["DatasetMapperTTAAVG", "GeneralizedRCNNWithTTAAVG", "DatasetMapperTTAUNION", "GeneralizedRCNNWithTTAUNION",
           "resize_shortest_edge_shape"]

VECTORISED_MAPPER = True  # tools: False = the per-augmentation mapper (its proposals are uploaded inside each pass)


def resize_shortest_edge_shape(h, w, size, max_size):
    """ResizeShortestEdge.get_transform, augmentation_impl.py:164-174"""
    scale = size * 1.0 / min(h, w)
    if h < w:
        newh, neww = size, scale * w
    else:
        newh, neww = scale * h, size
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh = newh * scale
        neww = neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def _resize_image(img_hwc, new_h, new_w):
    """ResizeTransform.apply_image, transform.py:101-122"""
    if img_hwc.dtype == np.uint8:
        try:
            from PIL import Image
        except ImportError as e:  # the reference has the same dependency for uint8 images
            raise DrnError("PIL is needed to resize uint8 images like the reference does") from e
        return np.asarray(Image.fromarray(img_hwc).resize((new_w, new_h), Image.BILINEAR))
    t = torch.from_numpy(np.ascontiguousarray(img_hwc)).permute(2, 0, 1)[None]
    t = F.interpolate(t, (new_h, new_w), mode="bilinear", align_corners=False)
    return t[0].permute(1, 2, 0).numpy()


def _apply_box(boxes, sx, sy, flip_w):
    """Transform.apply_box through [ResizeTransform, HFlipTransform?]: corners in float32, then their bounding box"""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    idx = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
    c = b[:, idx].reshape(-1, 2).copy()
    c[:, 0] = c[:, 0] * sx
    c[:, 1] = c[:, 1] * sy
    if flip_w is not None:
        c[:, 0] = flip_w - c[:, 0]
    c = c.reshape(-1, 4, 2)
    # (element-wise minima / maxima of the four corners: ndarray.min(axis=1) over the short middle axis took 3 ms per call on the
    # GPU box's host - 97 of the 101 ms of a 16-augmentation mapper call; same values, min / max are exact)
    lo = np.minimum(np.minimum(c[:, 0], c[:, 1]), np.minimum(c[:, 2], c[:, 3]))
    hi = np.maximum(np.maximum(c[:, 0], c[:, 1]), np.maximum(c[:, 2], c[:, 3]))
    return np.concatenate((lo, hi), axis=1)


class DatasetMapperTTAAVG:
    """test_time_augmentation_avg.py:68-137: dataset dict -> list of augmented dataset dicts (len(min_sizes) x
    (2 if flip else 1)); each carries "tta" = (sx, sy, flip_w) of the INVERSE box transform instead of a TransformList."""

    def __init__(self, cfg, device=None):
        # device (round 5): resize + flip of uint8 images run on that device (drn_resize_bilinear_u8: Pillow's integer
        # BILINEAR resample restated - bit-identical images) instead of 8 PIL resizes on the host per image, which took
        # ~0.4 s of a 0.41-s TTA call (tools/tta_bench.py, profiles/r5_20_tta.txt); None = the host path
        self.device = device
        self.min_sizes = cfg.TEST.AUG.MIN_SIZES
        self.max_size = cfg.TEST.AUG.MAX_SIZE
        self.flip = cfg.TEST.AUG.FLIP
        self.image_format = cfg.INPUT.FORMAT
        self.proposal_topk = cfg.DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TEST if cfg.MODEL.LOAD_PROPOSALS else None

    def __call__(self, dataset_dict):
        img = dataset_dict["image"]
        if self.device is not None and img.dtype == torch.uint8 and VECTORISED_MAPPER:
            return self._augmented_device(dataset_dict)
        return list(self._augmented(dataset_dict))

    def _augmented_device(self, dataset_dict):
        """The device path in one sweep: the image goes up once and is resized / flipped there (drn_resize_bilinear_u8); the proposal
        transform of ALL augmentations (transform_proposals, :27-65: scale, flip, bounding box of the corners, clip, drop empty boxes,
        top-k) is ONE set of float32 numpy operations on an [A, R, 4] block - the same operations on the same values as _apply_box
        / Boxes.clip / Boxes.nonempty per augmentation, so the same bits - written into a pinned staging buffer and uploaded in ONE
        asynchronous copy; each augmentation's Instances holds views of it.  (Per augmentation this was ~30 small numpy / torch calls
        and a pageable H2D copy inside its pass, which waits for the stream's queued work: 16-40 ms of host time per image on the GPU
        boxes' hosts, more than the 16 device passes take - profiles/r5_56_tta_batch.txt.)"""
        img = dataset_dict["image"].detach().cpu().permute(1, 2, 0).numpy()
        h, w = img.shape[:2]
        if (dataset_dict["height"], dataset_dict["width"]) != (h, w):
            raise DrnError("TTA on an already resized input (pre_tfm of the reference) is off this path")
        src = torch.from_numpy(np.ascontiguousarray(img)).to(self.device, non_blocking=True)  # [H, W, 3] uint8, once
        augs = [(resize_shortest_edge_shape(h, w, size, self.max_size), fl) for size in self.min_sizes
                for fl in ([False, True] if self.flip else [False])]
        out = []
        for (nh, nw), fl in augs:
            dic = {k: v for k, v in dataset_dict.items() if k not in ("image", "proposals")}
            dic["image"] = ops.resize_bilinear_u8(src, nh, nw, flip=fl)  # fp32 [3, nh, nw] of the same bytes
            dic["tta"] = (w * 1.0 / nw, h * 1.0 / nh, float(nw) if fl else -1.0)
            out.append(dic)
        if self.proposal_topk is None:
            return out
        prop = dataset_dict["proposals"]
        b = prop.proposal_boxes.tensor.detach().cpu().numpy().astype(np.float32, copy=False).reshape(-1, 4)
        logit = prop.objectness_logits.detach().cpu().numpy()
        A, R = len(augs), b.shape[0]
        f32 = np.float32
        sx = np.array([nw * 1.0 / w for (nh, nw), _ in augs], dtype=np.float64).astype(f32).reshape(A, 1, 1)
        sy = np.array([nh * 1.0 / h for (nh, nw), _ in augs], dtype=np.float64).astype(f32).reshape(A, 1, 1)
        cx = b[:, [0, 2, 0, 2]][None] * sx  # [A, R, 4] corner xs (x0, x1, x0, x1), float32 x float32 like `c[:, 0] * sx`
        cy = b[:, [1, 1, 3, 3]][None] * sy
        flipped = np.array([fl for _, fl in augs])
        fw = np.array([nw for (nh, nw), _ in augs], dtype=f32).reshape(A, 1, 1)
        if flipped.any():
            cx[flipped] = fw[flipped] - cx[flipped]
        x0, x1 = cx.min(axis=2), cx.max(axis=2)  # (min / max are exact: any order)
        y0, y1 = cy.min(axis=2), cy.max(axis=2)
        fh = np.array([nh for (nh, nw), _ in augs], dtype=f32).reshape(A, 1)
        fw = fw.reshape(A, 1)
        x0, x1 = np.minimum(np.maximum(x0, f32(0)), fw), np.minimum(np.maximum(x1, f32(0)), fw)  # Boxes.clip
        y0, y1 = np.minimum(np.maximum(y0, f32(0)), fh), np.minimum(np.maximum(y1, f32(0)), fh)
        keep = ((x1 - x0) > 0) & ((y1 - y0) > 0)  # Boxes.nonempty(threshold=0)
        boxes = np.stack((x0, y0, x1, y1), axis=2)  # [A, R, 4]
        k = self.proposal_topk
        cnt = [min(int(keep[a].sum()), k) for a in range(A)]
        n = sum(cnt)
        if getattr(self, "_pin", None) is None or self._pin.shape[0] < 5 * n:
            self._pin = torch.empty((max(5 * n, 1),), dtype=torch.float32).pin_memory()
            self._pin_ev = None
        if self._pin_ev is not None:
            self._pin_ev.synchronize()  # the previous call's copy has left the staging buffer (normally long done)
        pin = self._pin.numpy()
        hb, hl = pin[: 4 * n].reshape(n, 4), pin[4 * n: 5 * n]  # [all boxes | all logits]: every device view below is contiguous
        o = 0
        for a in range(A):
            c = cnt[a]
            if keep[a].all():
                hb[o: o + c] = boxes[a, :c]
                hl[o: o + c] = logit[:c]
            else:
                hb[o: o + c] = boxes[a][keep[a]][:c]
                hl[o: o + c] = logit[keep[a]][:c]
            o += c
        dev = self._pin[: 5 * n].to(self.device, non_blocking=True)
        self._pin_ev = torch.cuda.Event()
        self._pin_ev.record()
        db, dl = dev[: 4 * n].view(n, 4), dev[4 * n: 5 * n]
        o = 0
        for a, ((nh, nw), _) in enumerate(augs):
            p = Instances((nh, nw))
            p.proposal_boxes = Boxes(db[o: o + cnt[a]])
            p.objectness_logits = dl[o: o + cnt[a]]
            out[a]["proposals"] = p
            o += cnt[a]
        return out

    def _augmented(self, dataset_dict):
        img = dataset_dict["image"].detach().cpu().permute(1, 2, 0).numpy()
        h, w = img.shape[:2]
        if (dataset_dict["height"], dataset_dict["width"]) != (h, w):
            raise DrnError("TTA on an already resized input (pre_tfm of the reference) is off this path")
        on_dev = self.device is not None and img.dtype == np.uint8
        if on_dev:
            src = torch.from_numpy(np.ascontiguousarray(img)).to(self.device, non_blocking=True)  # [H, W, 3] uint8, once
        for size in self.min_sizes:
            nh, nw = resize_shortest_edge_shape(h, w, size, self.max_size)
            rimg = None if on_dev else _resize_image(np.copy(img), nh, nw)
            for flipped in ([False, True] if self.flip else [False]):
                dic = {k: v for k, v in dataset_dict.items() if k not in ("image", "proposals")}
                if on_dev:
                    dic["image"] = ops.resize_bilinear_u8(src, nh, nw, flip=flipped)  # fp32 [3, nh, nw] of the same bytes
                else:
                    im = np.flip(rimg, axis=1) if flipped else rimg
                    dic["image"] = torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1)))
                dic["tta"] = (w * 1.0 / nw, h * 1.0 / nh, float(nw) if flipped else -1.0)
                if self.proposal_topk is not None:
                    # transform_proposals (:27-65)
                    prop = dataset_dict["proposals"]
                    boxes = _apply_box(prop.proposal_boxes.tensor.detach().cpu().numpy(), nw * 1.0 / w, nh * 1.0 / h,
                                       nw if flipped else None)
                    boxes = Boxes(torch.from_numpy(boxes))
                    logits = prop.objectness_logits.detach().cpu()
                    boxes.clip((nh, nw))
                    keep = boxes.nonempty(threshold=0)
                    boxes, logits = boxes[keep], logits[keep]
                    p = Instances((nh, nw))
                    p.proposal_boxes = boxes[: self.proposal_topk]
                    p.objectness_logits = logits[: self.proposal_topk]
                    dic["proposals"] = p
                yield dic


class DatasetMapperTTAUNION(DatasetMapperTTAAVG):
    """test_time_augmentation_union.py:27-82: the AVG mapper's augmented images (the same code path: host PIL, or
    drn_resize_bilinear_u8 on `device`) and the same "tta" = (sx, sy, flip_w) key - but, restated as the reference has it,
    dataset_dict["proposals"] is NOT transformed: with MODEL.LOAD_PROPOSALS every augmentation gets the ORIGINAL image's
    proposals unchanged (the object itself, untouched), whatever the size or flip of its image (the reference's constructor
    assertion against it is disabled, :109-111).  That is the reference's default for GeneralizedRCNNWithTTAUNION and is kept as
    the default here; it is warned about once.  GeneralizedRCNNWithTTAUNION(cfg, model, tta_mapper=DatasetMapperTTAAVG(cfg,
    device=...)) is the combination whose proposals follow their images."""

    _warned = False

    def __init__(self, cfg, device=None):
        super().__init__(cfg, device=device)
        self.load_proposals = bool(cfg.MODEL.LOAD_PROPOSALS)
        self.proposal_topk = None  # the AVG code path then leaves "proposals" out: they are passed through below

    def __call__(self, dataset_dict):
        out = super().__call__(dataset_dict)
        if "proposals" in dataset_dict:
            if self.load_proposals and not DatasetMapperTTAUNION._warned:
                DatasetMapperTTAUNION._warned = True
                logging.warning("DatasetMapperTTAUNION leaves precomputed proposals in the ORIGINAL image's coordinates for every "
                                "augmentation, as the reference does (test_time_augmentation_union.py:27-82); pass "
                                "tta_mapper=DatasetMapperTTAAVG(cfg, device=...) for proposals that follow their images")
            for dic in out:
                dic["proposals"] = dataset_dict["proposals"]
        return out


class GeneralizedRCNNWithTTAAVG(nn.Module):
    """test_time_augmentation_avg.py:139-321 (box branch; masks / keypoints are off the WSL path)."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=1, padded=False):
        """padded=True: __call__ returns a DetectionBatch (one image per input, the merge through the batched tail with N = 1)
        instead of a list of dicts, and reads nothing back from the device."""
        super().__init__()
        from .rcnn import GeneralizedRCNNWSL

        model = getattr(model, "module", model)
        assert isinstance(model, GeneralizedRCNNWSL), \
            "TTA is only supported on GeneralizedRCNNWSL. Got a model of type {}".format(type(model))
        self.cfg = cfg.clone()
        assert not self.cfg.MODEL.KEYPOINT_ON, "TTA for keypoint is not supported yet"
        if self.cfg.MODEL.MASK_ON:
            raise DrnError("mask heads are off the DRN-WSOD path")
        if batch_size < 1:
            raise DrnError("batch_size must be >= 1")
        self.model = model
        self.tta_mapper = tta_mapper if tta_mapper is not None else DatasetMapperTTAAVG(cfg, device=model.device)
        self.batch_size = batch_size
        self.padded = bool(padded)

    def __call__(self, batched_inputs):
        out = []
        for x in batched_inputs:
            if "image" not in x:
                raise DrnError("reading images from file_name is the data loader's job (off this path)")
            ret = copy.copy(x)
            if "height" not in ret and "width" not in ret:
                ret["height"], ret["width"] = x["image"].shape[1], x["image"].shape[2]
            out.append(self._inference_one_image(ret))
        if self.padded:
            if len(out) == 1:
                return out[0]
            cat = lambda name: torch.cat([getattr(b, name) for b in out])
            return DetectionBatch(cat("boxes"), cat("scores"), cat("classes"), cat("count"),
                                  [b.image_sizes[0] for b in out], out[0].topk, rows=cat("rows"))
        return out

    def _get_augmented_boxes(self, augmented_inputs):
        """:269-294, on the device: running means of the back-transformed boxes and of the scores"""
        acc_b = acc_s = None
        n = len(augmented_inputs)
        heads = self.model.roi_heads
        # _batch_inference (:200-225): consecutive augmentations in groups of `batch_size` through ONE model.inference (the mapper
        # emits each size's plain and flipped image next to each other, so batch_size = 2 batches same-size pairs: one conv chain
        # per pair); the averages are accumulated per augmentation in the mapper's order either way
        prev, heads.scores_only = heads.scores_only, True
        try:
            for g0 in range(0, n, self.batch_size):
                group = augmented_inputs[g0: g0 + self.batch_size]
                # the per-pass detections are never used here (the reference computes and drops them): skip the inference tail
                _, scores, boxes = self.model.inference([{k: v for k, v in inp.items() if k != "tta"} for inp in group],
                                                        do_postprocess=False)
                for j, inp in enumerate(group):
                    i = g0 + j
                    sx, sy, flip_w = inp["tta"]
                    b, s = boxes[j][0].contiguous(), scores[j][0].contiguous()
                    if acc_b is None:
                        acc_b, acc_s = torch.empty_like(b), torch.empty_like(s)
                    elif acc_b.shape != b.shape:
                        raise DrnError("augmentations kept different numbers of proposals (%s vs %s): the averages are "
                                       "undefined (the reference fails in torch.cat here)" % (tuple(acc_b.shape), tuple(b.shape)))
                    ops.tta_accumulate(b, s, acc_b, acc_s, np.float32(sx), np.float32(sy), flip_w, i == 0, n if i == n - 1 else 0)
        finally:
            heads.scores_only = prev
        return acc_b, acc_s

    def _inference_one_image(self, input):
        orig_shape = (input["height"], input["width"])
        with torch.no_grad():
            # (queueing each augmentation's pass while the host prepares the next one was built and measured: 261 vs 86 ms per
            # image - the host work between the launches stretches the dependent chain; all augmentations first, then the passes)
            augmented_inputs = self.tta_mapper(input)
            all_boxes, all_scores = self._get_augmented_boxes(augmented_inputs)
            # _merge_detections (:296-309) = fast_rcnn_inference_single_image on the averages
            if self.padded:  # the same tail, padded and without the read of the count (merged instances are not postprocessed)
                return padded_detections(all_boxes, all_scores, [all_scores.shape[0]], [orig_shape], None,
                                         self.cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST, self.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST,
                                         self.cfg.TEST.DETECTIONS_PER_IMAGE)
            ob, os_, oc, _ = ops.detect_topk(all_boxes, all_scores, orig_shape, self.cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST,
                                             self.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, self.cfg.TEST.DETECTIONS_PER_IMAGE)
        r = Instances(orig_shape)
        r.pred_boxes = Boxes(ob)
        r.scores = os_
        r.pred_classes = oc
        return {"instances": r}


class GeneralizedRCNNWithTTAUNION(GeneralizedRCNNWithTTAAVG):
    """test_time_augmentation_union.py:85-264 (box branch): every augmentation's OWN detections (threshold / NMS / top-k per pass),
    mapped back to the original image, concatenated in augmentation order then detection order, and merged by one more
    threshold (1e-8) / NMS / top-k over the union.  Unlike the AVG form the augmentations may keep different numbers of
    proposals.  On the device this is two launch chains per image whatever the number of augmentations: ONE batched tail over
    the passes as "images" (padded_detections) and ONE drn_detect_union_batch; the reference runs a tail per pass, moves every
    pass's boxes to the host and back, and fills its [n, K+1] score matrix one element at a time.

    tta_mapper defaults to DatasetMapperTTAUNION as in the reference - which leaves precomputed proposals untransformed, see its
    docstring; DatasetMapperTTAAVG is accepted as well.  padded=True: __call__ returns a DetectionBatch on the original image
    sizes and reads nothing back; otherwise the reference's list of {"instances": ...}, at one read of the count per image."""

    MERGE_SCORE_THRESH = 1e-8  # :259

    def __init__(self, cfg, model, tta_mapper=None, batch_size=1, padded=False):
        inner = getattr(model, "module", model)
        if tta_mapper is None:
            tta_mapper = DatasetMapperTTAUNION(cfg, device=getattr(inner, "device", None))
        super().__init__(cfg, model, tta_mapper=tta_mapper, batch_size=batch_size, padded=padded)

    def _get_augmented_detections(self, augmented_inputs):
        """_batch_inference + the per-pass tails (:146-170, :228-230): a DetectionBatch with one block per augmentation, in the
        augmented images' coordinates, and the passes' (sx, sy, flip_w)"""
        heads = self.model.roi_heads
        all_b, all_s, nper, sizes = [], [], [], []
        # the passes deliver scores / boxes alone; their tails then run in ONE chain instead of one per pass
        prev, heads.scores_only = heads.scores_only, True
        try:
            for g0 in range(0, len(augmented_inputs), self.batch_size):
                group = augmented_inputs[g0: g0 + self.batch_size]
                _, scores, boxes = self.model.inference([{k: v for k, v in inp.items() if k != "tta"} for inp in group],
                                                        do_postprocess=False)
                for j, inp in enumerate(group):
                    all_b.append(boxes[j][0])
                    all_s.append(scores[j][0])
                    nper.append(int(scores[j][0].shape[0]))
                    # a pass clips to its proposals' image size (fast_rcnn.py: image_shapes = [x.image_size for x in proposals]):
                    # the augmented image's under DatasetMapperTTAAVG, the original image's under DatasetMapperTTAUNION
                    sizes.append(tuple(inp["proposals"].image_size) if "proposals" in inp else tuple(inp["image"].shape[1:]))
        finally:
            heads.scores_only = prev
        det = padded_detections(torch.cat(all_b).contiguous(), torch.cat(all_s).contiguous(), nper, sizes, None,
                                self.cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST, self.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST,
                                self.cfg.TEST.DETECTIONS_PER_IMAGE)
        return det, [inp["tta"] for inp in augmented_inputs]

    def _merge_detections(self, det, tfms, orig_shape):
        """:246-264 with the back-transform of :236-239 inside: ops.detect_union_batch on the passes' blocks"""
        return ops.detect_union_batch(det.boxes, det.scores, det.classes, det.count, [0, len(det)], tfms, [orig_shape],
                                      num_classes=self.cfg.MODEL.ROI_HEADS.NUM_CLASSES, score_thresh=self.MERGE_SCORE_THRESH,
                                      nms_thresh=self.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST,
                                      topk=self.cfg.TEST.DETECTIONS_PER_IMAGE)

    def _inference_one_image(self, input):
        orig_shape = (input["height"], input["width"])
        with torch.no_grad():
            augmented_inputs = self.tta_mapper(input)
            det, tfms = self._get_augmented_detections(augmented_inputs)
            ob, os_, oc, orow, cnt = self._merge_detections(det, tfms, orig_shape)
        merged = DetectionBatch(ob, os_, oc, cnt, [orig_shape], self.cfg.TEST.DETECTIONS_PER_IMAGE, rows=orow)
        if self.padded:
            return merged
        return merged.to_outputs()[0]  # (merged instances are not postprocessed, :220-221)
