"""ROI heads of the DRN-WSOD / OICR path behind the reference's names and constructor arguments:

  ROIPooler                    detectron2/modeling/poolers.py:99-246
  Matcher                      detectron2/modeling/matcher.py:8-126
  Box2BoxTransform             detectron2/modeling/box_regression.py:17-110
  DiscriminativeAdaptionNeck   projects/WSL/wsl/modeling/roi_heads/box_head.py:14-103
  WSDDNOutputLayers            projects/WSL/wsl/modeling/roi_heads/fast_rcnn.py:396-700
  OICROutputLayers             projects/WSL/wsl/modeling/roi_heads/fast_rcnn.py:1267-1594
  ROIHeads / OICRROIHeads / WSDDNROIHeads
                               projects/WSL/wsl/modeling/roi_heads/{roi_heads.py:156-353, roi_heads_oicr.py:33-567,
                               roi_heads_wsddn.py}

Same module tree => same state_dict keys (roi_heads.box_head.fc1.weight, roi_heads.box_predictor.cls.weight,
roi_heads.box_refinery_0.cls_score.weight, ...).  The arithmetic does not run module by module: OICRROIHeads
drives one fused schedule of HIP kernels (`_HeadEngine`, modeling/head_engine.py) — ROIPool fused with the objectness
scaling writes the fc6 operand, three MFMA GEMM groups (fc6, fc7, all predictor Linears concatenated), the MIL/OICR
kernels, and an explicit backward (dW/dX GEMMs) that writes gradients straight into a flat fp32 arena shared with the
fused SGD kernel and the gradient all-reduce.  No host synchronisation happens inside a step."""
import inspect
import math
from typing import List

import torch
from torch import nn

from .. import compute_dtype, ops
from .._cabi import DrnError
from ..config import configurable
from ..events import get_event_storage, has_event_storage
from ..layers import Linear, ROIAlign, RoIPool, ShapeSpec, to_nhwc
from ..registry import ROI_BOX_HEAD_REGISTRY, ROI_HEADS_REGISTRY
from ..structures import Boxes, DetectionBatch, Instances
# (re-exported: roi_heads._HeadEngine / _TrainFn and the dropout-seed rule still resolve here)
from .head_engine import DROP_COUNTER_STEP, FC7_SEED_OFFSET, _HeadEngine, _TrainFn, dropout_seeds  # noqa: F401


def padded_detections(boxes, scores, nper, image_sizes, output_sizes, score_thresh, nms_thresh, topk):
    """The batched inference tail (ops.detect_topk_batch) on the rows of len(nper) images, as a DetectionBatch: raw (in
    `image_sizes` coordinates) when output_sizes is None, else after detector_postprocess to `output_sizes`.  Batches beyond
    the entry's limits are chunked here: the launch count then depends on the number of chunks alone.  No host read."""
    K = scores.shape[1] - 1
    chunks, lo, n_img = [], 0, len(nper)
    while lo < n_img:
        hi = lo + 1
        while (hi < n_img and hi - lo < ops.DETECT_MAX_IMAGES
               and sum(nper[lo: hi + 1]) * K <= ops.DETECT_BATCH_MAX_ENTRIES):
            hi += 1
        chunks.append((lo, hi))
        lo = hi
    parts, r0 = [], 0
    for lo, hi in chunks:
        rows = sum(nper[lo:hi])
        off = [0]
        for n in nper[lo:hi]:
            off.append(off[-1] + n)
        parts.append(ops.detect_topk_batch(boxes[r0: r0 + rows], scores[r0: r0 + rows], off, image_sizes[lo:hi],
                                           None if output_sizes is None else output_sizes[lo:hi],
                                           score_thresh=score_thresh, nms_thresh=nms_thresh, topk=topk))
        r0 += rows
    ob, os_, oc, orow, cnt = parts[0] if len(parts) == 1 else (torch.cat(t) for t in zip(*parts))
    return DetectionBatch(ob, os_, oc, cnt, image_sizes if output_sizes is None else output_sizes, topk, rows=orow)


# ------------------------------------------------------------------------------------------------
class Matcher:
    """The reference's constructor checks (matcher.py:24-59) and __call__ (matcher.py:61-103) without low-quality matches.  The
    training path does not come through here: its matching (column arg-max over GT + threshold labelling) runs inside
    drn_oicr_targets / drn_label_proposals; __call__ is the same rule as a stand-alone device op (ops.match)."""

    def __init__(self, thresholds: List[float], labels: List[int], allow_low_quality_matches: bool = False):
        thresholds = thresholds[:]
        assert thresholds[0] > 0
        thresholds.insert(0, -float("inf"))
        thresholds.append(float("inf"))
        assert all(low <= high for (low, high) in zip(thresholds[:-1], thresholds[1:]))
        assert all(l in [-1, 0, 1] for l in labels)
        assert len(labels) == len(thresholds) - 1
        if allow_low_quality_matches:
            raise DrnError("allow_low_quality_matches is off the OICR path (roi_heads.py:207-211 passes False)")
        self.thresholds = thresholds
        self.labels = labels
        self.allow_low_quality_matches = allow_low_quality_matches

    def __call__(self, match_quality_matrix):
        """[N, M] qualities (N ground-truth rows, M predictions) -> (matches [M] int64, match_labels [M] int8)"""
        return ops.match(match_quality_matrix, self.thresholds[1:-1], self.labels)


class Box2BoxTransform:
    """box_regression.py:17-110 (weights + scale clamp; apply_deltas executes drn_apply_deltas)."""

    def __init__(self, weights, scale_clamp: float = math.log(1000.0 / 16)):
        self.weights = tuple(weights)
        self.scale_clamp = scale_clamp

    def apply_deltas(self, deltas, boxes):
        k = deltas.shape[1] // 4
        return ops.apply_deltas(deltas.float().contiguous(), boxes.float().contiguous(), k, self.weights)


def convert_boxes_to_pooler_format(box_lists: List[Boxes]):
    """poolers.py:62-96 -> [M,5] (batch index, x0, y0, x1, y1)."""
    return torch.cat([torch.cat((torch.full((len(b), 1), float(i), dtype=b.tensor.dtype, device=b.tensor.device),
                                 b.tensor), dim=1) for i, b in enumerate(box_lists)], dim=0)


class ROIPooler(nn.Module):
    """poolers.py:99-246, single feature level (the only case on this path)."""

    def __init__(self, output_size, scales, sampling_ratio, pooler_type, canonical_box_size=224, canonical_level=4):
        super().__init__()
        if isinstance(output_size, int):
            output_size = (output_size, output_size)
        assert len(output_size) == 2 and output_size[0] == output_size[1]
        self.output_size = output_size
        if len(scales) != 1:
            raise DrnError("multi-level (FPN) pooling is off the DRN-WSOD path")
        self.pooler_type, self.sampling_ratio, self.scales = pooler_type, sampling_ratio, tuple(scales)
        if pooler_type == "ROIAlign":
            self.level_poolers = nn.ModuleList(ROIAlign(output_size, s, sampling_ratio, aligned=False) for s in scales)
        elif pooler_type == "ROIAlignV2":
            self.level_poolers = nn.ModuleList(ROIAlign(output_size, s, sampling_ratio, aligned=True) for s in scales)
        elif pooler_type == "ROIPool":
            self.level_poolers = nn.ModuleList(RoIPool(output_size, spatial_scale=s) for s in scales)
        else:
            raise ValueError("Unknown pooler type: {}".format(pooler_type))
        min_level = -(math.log2(scales[0]))
        assert math.isclose(min_level, int(min_level)), "Featuremap stride is not power of 2!"

    def kernel_args(self):
        mode = 0 if self.pooler_type == "ROIPool" else 1
        return dict(P=self.output_size[0], scale=self.scales[0], mode=mode, sampling_ratio=self.sampling_ratio,
                    aligned=self.pooler_type == "ROIAlignV2")

    def forward(self, x: List[torch.Tensor], box_lists: List[Boxes]):
        assert isinstance(x, list) and isinstance(box_lists, list), "Arguments to pooler must be lists"
        assert len(x) == 1 and len(box_lists) == x[0].size(0)
        return self.level_poolers[0](x[0], convert_boxes_to_pooler_format(box_lists))


# ------------------------------------------------------------------------------------------------
@ROI_BOX_HEAD_REGISTRY.register()
class DiscriminativeAdaptionNeck(nn.Module):
    """box_head.py:14-103: flatten -> fc1 -> ReLU -> dropout(0.5) -> fc2 -> ReLU -> dropout(0.5)."""

    @configurable
    def __init__(self, input_shape: ShapeSpec, *, conv_dims: List[int], fc_dims: List[int], conv_norm=""):
        super().__init__()
        assert len(conv_dims) + len(fc_dims) > 0
        if len(conv_dims):
            raise DrnError("DAN conv layers (NUM_CONV > 0) are not used by any DRN-WSOD config")
        self._output_size = (input_shape.channels, input_shape.height, input_shape.width)
        self.conv_norm_relus = []
        self.fcs = []
        for k, fc_dim in enumerate(fc_dims):
            size = self._output_size if isinstance(self._output_size, int) else int(
                self._output_size[0] * self._output_size[1] * self._output_size[2])
            fc = Linear(size, fc_dim)
            self.add_module("fc{}".format(k + 1), fc)
            self.fcs.append(fc)
            self._output_size = fc_dim
        for layer in self.fcs:
            torch.nn.init.normal_(layer.weight, std=0.005)
            torch.nn.init.constant_(layer.bias, 0.1)
        self.dropout_p = 0.5          # box_head.py:90 hard-codes p=0.5
        self.dropout_masks = None     # test hook: explicit [M, fc_dim] multiplier masks

    @classmethod
    def from_config(cls, cfg, input_shape):
        return {"input_shape": input_shape, "conv_dims": [cfg.MODEL.ROI_BOX_HEAD.CONV_DIM] * cfg.MODEL.ROI_BOX_HEAD.NUM_CONV,
                "fc_dims": cfg.MODEL.ROI_BOX_HEAD.DAN_DIM, "conv_norm": cfg.MODEL.ROI_BOX_HEAD.NORM}

    @property
    def output_shape(self):
        o = self._output_size
        return ShapeSpec(channels=o) if isinstance(o, int) else ShapeSpec(channels=o[0], height=o[1], width=o[2])

    def forward(self, x):
        raise DrnError("DiscriminativeAdaptionNeck runs inside the fused OICRROIHeads schedule; call the ROI heads")


@ROI_BOX_HEAD_REGISTRY.register()
class FastRCNNConvFCHead(nn.Module):
    """detectron2/modeling/roi_heads/box_head.py:23-95 as wsddn_R_50_DC5_1x.yaml configures it (NUM_CONV 0, NUM_FC 2):
    flatten -> fc1 -> ReLU -> fc2 -> ReLU.  The same two-Linear neck as DiscriminativeAdaptionNeck WITHOUT dropout, so it runs
    on the same head engine, which reads `dropout_p` (0 here) and `dropout_masks`."""

    @configurable
    def __init__(self, input_shape: ShapeSpec, *, conv_dims: List[int], fc_dims: List[int], conv_norm=""):
        super().__init__()
        assert len(conv_dims) + len(fc_dims) > 0
        if len(conv_dims):
            raise DrnError("MODEL.ROI_BOX_HEAD.NUM_CONV = %d: conv layers in the box head are not built (no shipped "
                           "WSL recipe sets them)" % len(conv_dims))
        if conv_norm:
            raise DrnError("MODEL.ROI_BOX_HEAD.NORM = '%s': the box head has no conv layers to normalise" % conv_norm)
        if len(fc_dims) != 2:
            raise DrnError("MODEL.ROI_BOX_HEAD.NUM_FC = %d: the head engine runs the two-layer neck (fc1, fc2)" % len(fc_dims))
        self._output_size = (input_shape.channels, input_shape.height, input_shape.width)
        self.conv_norm_relus = []
        self.fcs = []
        for k, fc_dim in enumerate(fc_dims):
            size = self._output_size if isinstance(self._output_size, int) else int(
                self._output_size[0] * self._output_size[1] * self._output_size[2])
            fc = Linear(size, fc_dim)
            self.add_module("fc{}".format(k + 1), fc)
            self.fcs.append(fc)
            self._output_size = fc_dim
        for layer in self.fcs:  # fvcore.nn.weight_init.c2_xavier_fill
            torch.nn.init.kaiming_uniform_(layer.weight, a=1)
            torch.nn.init.constant_(layer.bias, 0)
        self.dropout_p = 0.0          # box_head.py:95-96: relu only
        self.dropout_masks = None

    @classmethod
    def from_config(cls, cfg, input_shape):
        return {"input_shape": input_shape, "conv_dims": [cfg.MODEL.ROI_BOX_HEAD.CONV_DIM] * cfg.MODEL.ROI_BOX_HEAD.NUM_CONV,
                "fc_dims": [cfg.MODEL.ROI_BOX_HEAD.FC_DIM] * cfg.MODEL.ROI_BOX_HEAD.NUM_FC,
                "conv_norm": cfg.MODEL.ROI_BOX_HEAD.NORM}

    @property
    def output_shape(self):
        o = self._output_size
        return ShapeSpec(channels=o) if isinstance(o, int) else ShapeSpec(channels=o[0], height=o[1], width=o[2])

    def forward(self, x):
        raise DrnError("FastRCNNConvFCHead runs inside the fused ROI-heads schedule; call the ROI heads")


def build_box_head(cfg, input_shape):
    return ROI_BOX_HEAD_REGISTRY.get(cfg.MODEL.ROI_BOX_HEAD.NAME)(cfg, input_shape)


class _OutputLayersBase(nn.Module):
    def _common(self, box2box_transform, test_score_thresh, test_nms_thresh, test_topk_per_image, smooth_l1_beta,
                box_reg_loss_type, loss_weight, mean_loss):
        self.box2box_transform = box2box_transform
        self.smooth_l1_beta = smooth_l1_beta
        self.test_score_thresh = test_score_thresh
        self.test_nms_thresh = test_nms_thresh
        self.test_topk_per_image = test_topk_per_image
        self.box_reg_loss_type = box_reg_loss_type
        if isinstance(loss_weight, float):
            loss_weight = {"loss_cls": loss_weight, "loss_box_reg": loss_weight}
        self.loss_weight = loss_weight
        self.mean_loss = mean_loss

    @staticmethod
    def _cfg_common(cfg):
        return {
            "box2box_transform": Box2BoxTransform(weights=cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS),
            "num_classes": cfg.MODEL.ROI_HEADS.NUM_CLASSES,
            "cls_agnostic_bbox_reg": cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG,
            "smooth_l1_beta": cfg.MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA,
            "test_score_thresh": cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST,
            "test_nms_thresh": cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST,
            "test_topk_per_image": cfg.TEST.DETECTIONS_PER_IMAGE,
            "box_reg_loss_type": cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE,
            "loss_weight": {"loss_box_reg": cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_WEIGHT},
            "mean_loss": cfg.WSL.MEAN_LOSS,
        }


class WSDDNOutputLayers(_OutputLayersBase):
    """fast_rcnn.py:396-700: `cls` and `det` Linear(input, K), Xavier-uniform, zero bias."""

    @configurable
    def __init__(self, input_shape, *, box2box_transform, num_classes, test_score_thresh=0.0, test_nms_thresh=0.5,
                 test_topk_per_image=100, cls_agnostic_bbox_reg=False, smooth_l1_beta=0.0,
                 box_reg_loss_type="smooth_l1", loss_weight=1.0, mean_loss=True):
        super().__init__()
        if isinstance(input_shape, int):
            input_shape = ShapeSpec(channels=input_shape)
        input_size = input_shape.channels * (input_shape.width or 1) * (input_shape.height or 1)
        self.num_bbox_reg_classes = 1 if cls_agnostic_bbox_reg else num_classes
        self.box_dim = len(box2box_transform.weights)
        self.num_classes = num_classes
        self.cls = Linear(input_size, num_classes)
        self.det = Linear(input_size, num_classes)
        nn.init.xavier_uniform_(self.cls.weight)
        nn.init.xavier_uniform_(self.det.weight)
        for l in [self.cls, self.det]:
            nn.init.constant_(l.bias, 0)
        self._common(box2box_transform, test_score_thresh, test_nms_thresh, test_topk_per_image, smooth_l1_beta,
                     box_reg_loss_type, loss_weight, mean_loss)

    @classmethod
    def from_config(cls, cfg, input_shape):
        d = cls._cfg_common(cfg)
        d["input_shape"] = input_shape
        return d


class OICROutputLayers(_OutputLayersBase):
    """fast_rcnn.py:1267-1594: `cls_score` Linear(input, K+1) (std 0.01) and `bbox_pred` Linear(input, 4K)
    (std 0.001; only used when WSL.REFINE_REG[k])."""

    @configurable
    def __init__(self, input_shape, *, box2box_transform, num_classes, test_score_thresh=0.0, test_nms_thresh=0.5,
                 test_topk_per_image=100, cls_agnostic_bbox_reg=False, smooth_l1_beta=0.0,
                 box_reg_loss_type="smooth_l1", loss_weight=1.0, mean_loss=True, refine_k=None, refine_reg=False):
        super().__init__()
        if isinstance(input_shape, int):
            input_shape = ShapeSpec(channels=input_shape)
        input_size = input_shape.channels * (input_shape.width or 1) * (input_shape.height or 1)
        if cls_agnostic_bbox_reg:
            raise DrnError("class-agnostic box regression is not used by any DRN-WSOD config")
        regresses = refine_reg  # cfg.WSL.REFINE_REG (one flag per branch) or this branch's flag
        if isinstance(regresses, (list, tuple)):
            regresses = regresses[refine_k] if refine_k is not None else any(regresses)
        if regresses:
            # drn_box_reg_loss computes the class-specific L1 loss (smooth-L1 with beta = 0) with weight 1, as every shipped
            # config does (fast_rcnn.py:1146-1211); any other setting would train with the wrong loss
            lw = loss_weight.get("loss_box_reg", 1.0) if isinstance(loss_weight, dict) else loss_weight
            if box_reg_loss_type != "smooth_l1":
                raise DrnError("BBOX_REG_LOSS_TYPE %r is not on the built path (only smooth_l1)" % (box_reg_loss_type,))
            if smooth_l1_beta != 0.0:
                raise DrnError("SMOOTH_L1_BETA %r is not on the built path (the box loss is L1: beta = 0)" % (smooth_l1_beta,))
            if lw != 1.0:
                raise DrnError("BBOX_REG_LOSS_WEIGHT %r is not on the built path (weight 1)" % (lw,))
        self.num_classes = num_classes
        self.cls_score = Linear(input_size, num_classes + 1)
        self.num_bbox_reg_classes = num_classes
        self.box_dim = len(box2box_transform.weights)
        self.bbox_pred = Linear(input_size, self.num_bbox_reg_classes * self.box_dim)
        nn.init.normal_(self.cls_score.weight, std=0.01)
        nn.init.normal_(self.bbox_pred.weight, std=0.001)
        for l in [self.cls_score, self.bbox_pred]:
            nn.init.constant_(l.bias, 0)
        self._common(box2box_transform, test_score_thresh, test_nms_thresh, test_topk_per_image, smooth_l1_beta,
                     box_reg_loss_type, loss_weight, mean_loss)
        self.refine_k = refine_k
        self.refine_reg = refine_reg

    @classmethod
    def from_config(cls, cfg, input_shape, refine_k):
        d = cls._cfg_common(cfg)
        d.update(input_shape=input_shape, refine_reg=cfg.WSL.REFINE_REG, refine_k=refine_k)
        return d


# ------------------------------------------------------------------------------------------------
class ROIHeads(nn.Module):
    """roi_heads.py:156-212 (constructor / from_config)."""

    @configurable
    def __init__(self, *, num_classes, batch_size_per_image, positive_fraction, proposal_matcher,
                 proposal_append_gt=True):
        super().__init__()
        self.batch_size_per_image = batch_size_per_image
        self.positive_fraction = positive_fraction
        self.num_classes = num_classes
        self.proposal_matcher = proposal_matcher
        self.proposal_append_gt = proposal_append_gt

    @classmethod
    def from_config(cls, cfg):
        return {
            "batch_size_per_image": cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE,
            "positive_fraction": cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION,
            "num_classes": cfg.MODEL.ROI_HEADS.NUM_CLASSES,
            "proposal_append_gt": cfg.MODEL.ROI_HEADS.PROPOSAL_APPEND_GT,
            "proposal_matcher": Matcher(cfg.MODEL.ROI_HEADS.IOU_THRESHOLDS, cfg.MODEL.ROI_HEADS.IOU_LABELS,
                                        allow_low_quality_matches=False),
        }


def pack_annotated(targets, max_gt, setter="enable_metrics(max_gt=%d)"):
    """the annotated boxes of a step, packed on the host for the label upload: int32 words [boxes fp32 n_img * max_gt * 4 |
    classes n_img * max_gt | counts n_img] (views: annotated_views).  Feeds the un-suffixed logging scalars of the metrics ring
    (roi_heads.py:256-353) and the box regression of a regressing PCL branch.  More than max_gt boxes in an image: DrnError - the
    length is known here, without a sync (`setter`: the call that sized the block, for the message)."""
    n_img = len(targets)
    words = torch.zeros((annotated_words(n_img, max_gt),), dtype=torch.int32)
    v = annotated_views(words, n_img, max_gt)
    for i, t in enumerate(targets):
        b = t.gt_boxes.tensor.detach().cpu().to(torch.float32).reshape(-1, 4)
        c = t.gt_classes.detach().cpu().reshape(-1)
        if b.shape[0] != c.shape[0]:
            raise DrnError("image %d: %d annotated boxes, %d classes" % (i, b.shape[0], c.shape[0]))
        if b.shape[0] > max_gt:
            raise DrnError("image %d has %d annotated boxes, %s holds at most %d: enable with a larger "
                           "max_gt" % (i, b.shape[0], setter % max_gt, max_gt))
        v["ann_boxes"][i, : b.shape[0]] = b
        v["ann_classes"][i, : c.shape[0]] = c.to(torch.int32)
        v["ann_count"][i] = b.shape[0]
    return words


def annotated_words(n_img, max_gt):
    return n_img * max_gt * 5 + n_img


def annotated_views(words, n_img, max_gt):
    """the three tensors of pack_annotated's word block, as views (host or device)"""
    nb = n_img * max_gt * 4
    return dict(ann_boxes=words[:nb].view(torch.float32).view(n_img, max_gt, 4),
                ann_classes=words[nb: nb + n_img * max_gt].view(n_img, max_gt), ann_count=words[nb + n_img * max_gt:])


def get_image_level_gt(targets, num_classes):
    """roi_heads.py:137-153.  `unique(sorted=True)` of a handful of ints: done on the host copy of the labels
    (they arrive from the data loader on the host), so no device sync is introduced."""
    if targets is None:
        return None, None, None
    ints = [torch.unique(t.gt_classes.detach().cpu(), sorted=True).to(torch.int64) for t in targets]
    oh = torch.zeros((len(ints), num_classes), dtype=torch.float32)
    for i, g in enumerate(ints):
        oh[i, g] = 1
    return ints, ints, oh


@ROI_HEADS_REGISTRY.register()
class OICRROIHeads(ROIHeads):
    """roi_heads_oicr.py:33-567."""

    refine_mode = "oicr"  # how the refinement branches are trained ("pcl": PCLROIHeads); the head engine picks its loss tail by it
    csc_head = False      # CSCROIHeads

    @configurable
    def __init__(self, *, box_in_features, box_pooler, box_head, box_predictor, mask_in_features=None,
                 mask_pooler=None, mask_head=None, keypoint_in_features=None, keypoint_pooler=None,
                 keypoint_head=None, train_on_pred_boxes=False, output_dir=None, vis_test=False, vis_period=0,
                 refine_K=4, refine_reg=(False, False, False, False), box_refinery=(None, None, None, None),
                 cls_agnostic_bbox_reg=False, **kwargs):
        super().__init__(**kwargs)
        if mask_in_features is not None or keypoint_in_features is not None or train_on_pred_boxes:
            raise DrnError("mask / keypoint heads and train_on_pred_boxes are off the DRN-WSOD path")
        self.in_features = self.box_in_features = box_in_features
        self.box_pooler = box_pooler
        self.box_head = box_head
        self.box_predictor = box_predictor
        self.mask_on = self.keypoint_on = False
        self.train_on_pred_boxes = train_on_pred_boxes
        self.iter = self.iter_test = self.epoch_test = 0
        self.output_dir, self.vis_test, self.vis_period = output_dir, vis_test, vis_period
        self.refine_K = refine_K
        self.refine_reg = list(refine_reg)
        self.box_refinery = list(box_refinery)
        for k in range(self.refine_K):
            self.add_module("box_refinery_{}".format(k), self.box_refinery[k])
        self.cls_agnostic_bbox_reg = cls_agnostic_bbox_reg
        self._props = None       # (rois, contiguous proposal boxes) of the last _gather_inputs / prefetch (_take_props)
        self._zero_oh = None     # cached zero label matrix of the WSDDN inference scores
        self._prefetched = None  # what prefetch_pooled() returned for the batch of this forward
        self.scores_only = False  # GeneralizedRCNNWithTTAAVG: inference returns all_scores / all_boxes alone
        self.padded_tail = None   # GeneralizedRCNNWSL.inference(padded=True): a dict while the batched tail is asked for
        self._engine = _HeadEngine(self)

    @classmethod
    def from_config(cls, cfg, input_shape):
        ret = super().from_config(cfg)
        ret["train_on_pred_boxes"] = cfg.MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES
        if inspect.ismethod(cls._init_box_head):
            ret.update(cls._init_box_head(cfg, input_shape))
        return ret

    _refine_from_cfg = True

    @classmethod
    def _init_box_head(cls, cfg, input_shape):
        in_features = cfg.MODEL.ROI_HEADS.IN_FEATURES
        pooler_resolution = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
        pooler_scales = tuple(1.0 / input_shape[k].stride for k in in_features)
        in_channels = [input_shape[f].channels for f in in_features]
        assert len(set(in_channels)) == 1, in_channels
        in_channels = in_channels[0]
        box_pooler = ROIPooler(output_size=pooler_resolution, scales=pooler_scales,
                               sampling_ratio=cfg.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO,
                               pooler_type=cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE)
        box_head = build_box_head(cfg, ShapeSpec(channels=in_channels, height=pooler_resolution, width=pooler_resolution))
        box_predictor = WSDDNOutputLayers(cfg, box_head.output_shape)
        refine_K = cfg.WSL.REFINE_NUM if cls._refine_from_cfg else 0
        box_refinery = [OICROutputLayers(cfg, box_head.output_shape, k) for k in range(refine_K)]
        return {"box_in_features": in_features, "box_pooler": box_pooler, "box_head": box_head,
                "box_predictor": box_predictor, "output_dir": cfg.OUTPUT_DIR, "vis_test": cfg.WSL.VIS_TEST,
                "vis_period": cfg.VIS_PERIOD, "refine_K": refine_K, "refine_reg": cfg.WSL.REFINE_REG,
                "box_refinery": box_refinery, "cls_agnostic_bbox_reg": cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG}

    # ---- helpers --------------------------------------------------------------------------------------
    def _gather_inputs(self, features, proposals):
        feat = features[self.box_in_features[0]]
        nhwc = feat.permute(0, 2, 3, 1)
        if not nhwc.is_contiguous() or nhwc.dtype != compute_dtype():
            nhwc = to_nhwc(feat, compute_dtype())
        self._props = None
        if len(proposals) == 1:
            # one image (every shipped config trains and tests with one image per GPU): rois, logits and the boxes' contiguous
            # copy in ONE launch instead of torch.full + two torch.cat + three copies in front of every forward
            b, l = proposals[0].proposal_boxes.tensor, proposals[0].objectness_logits
            if (b.is_cuda and b.dtype == torch.float32 and b.dim() == 2 and b.is_contiguous() and l is not None and l.is_cuda and
                    l.device == b.device and l.dtype == torch.float32 and l.dim() == 1 and l.shape[0] == b.shape[0] and
                    l.is_contiguous()):
                rois, obj, props = ops.stage_rois(b, l, 0.0)
                self._props = (rois, props)  # (tied to THIS rois tensor: a prefetch of a later batch may gather in between)
                return nhwc, rois, obj
        rois = convert_boxes_to_pooler_format([p.proposal_boxes for p in proposals]).float().contiguous()
        obj = torch.cat([p.objectness_logits for p in proposals], dim=0).float().contiguous()
        return nhwc, rois, obj

    def _take_props(self, rois):
        """the proposal boxes as a contiguous [M, 4] tensor: the copy _gather_inputs made in its staging launch, else a slice copy"""
        p, self._props = self._props, None
        return p[1] if p is not None and p[0] is rois and p[1] is not None else rois[:, 1:].contiguous()

    def _zero_onehot(self, n_img, K, dev):
        z = self._zero_oh
        if z is None or z.shape != (n_img, K) or z.device != dev:
            z = self._zero_oh = torch.zeros((n_img, K), dtype=torch.float32, device=dev)
        return z

    def enable_metrics(self, slots=256, annotated=False, max_gt=64):
        """Record every training step's losses and, for OICR branches, label statistics into a device-side ring of `slots`
        records (metrics.MetricsRing, returned): two small launches behind the loss tail, no host sync.  A graphed step freezes
        its launch sequence when it is primed, so this has to come first: enable_metrics() -> build / prime the graphed step.
        annotated=True (any head class): two more launches label the proposals against the ANNOTATED boxes of targets[i].gt_boxes /
        gt_classes (at most max_gt per image) and record the reference's six un-suffixed scalars, roi_head/num_{fg,bg,ig}_samples
        and fast_rcnn/{cls_accuracy,fg_cls_accuracy,false_negative}; the boxes travel in the step's label upload."""
        from .. import ops
        from ..metrics import MetricsRing

        if annotated:
            if self.proposal_append_gt:
                raise DrnError("enable_metrics(annotated=True) with MODEL.ROI_HEADS.PROPOSAL_APPEND_GT = True: appending the "
                               "annotated boxes to the proposals is not built (every shipped recipe sets it False)")
            if not 1 <= int(max_gt) <= ops.LABEL_MAX_GT:
                raise DrnError("enable_metrics(max_gt=%d): 1 .. %d annotated boxes per image are built" % (max_gt, ops.LABEL_MAX_GT))
            if self.refine_mode != "pcl" and self.refine_K > ops.METRICS_ANNOT_ROW:
                raise DrnError("enable_metrics(annotated=True) with %d OICR branches: the block takes the record's last head slot, "
                               "at most %d branches leave room" % (self.refine_K, ops.METRICS_ANNOT_ROW))

        eng = self._engine
        owner = eng.captured_by
        if owner is not None and owner() is not None:
            raise DrnError("enable_metrics() after a graphed step was primed: its captured launches would never record.  Order: "
                           "enable_metrics(), then create and prime the GraphedTrainStep / GraphedFullStep")
        eng.ensure(next(self.parameters()).device)
        eng.metrics = MetricsRing(slots, eng.arena_w.device, annotated, max_gt)
        return eng.metrics

    def _annot_capacity(self):
        """annotated boxes per image that a training step's label upload carries; 0 = none.  The metrics ring's annotated-box block
        sizes it (enable_metrics(annotated=True, max_gt=)); PCLROIHeads with a regressing branch needs the block as well."""
        ring = self._engine.metrics
        return ring.max_gt if ring is not None and ring.annotated else 0

    def _annot_setter(self):
        return "enable_metrics(max_gt=%d)"

    def disable_metrics(self):
        """back to the launch sequence without metrics (eager steps at once; a primed graphed step keeps what it captured)"""
        self._engine.metrics = None

    def prefetch_pooled(self, features, proposals):
        """pool a FUTURE batch's proposals (on whatever stream is current) into the engine's spare buffer set"""
        if self._engine.kshard is not None:
            return None  # K-sharded fc6: the operand is built from every rank's features inside the forward
        nhwc, rois, obj = self._gather_inputs(features, proposals)
        return dict(rois=rois, obj=obj, props=self._take_props(rois),
                    pooled=self._engine.pool(nhwc, rois, obj, self.training, prefetch=True))

    def forward(self, images, features, proposals, targets=None, prefetched=None):
        """roi_heads_oicr.py:248-291."""
        self.images = images
        self._prefetched = prefetched
        if self.training:
            assert targets
            losses = self._forward_box(features, proposals, targets)
            self.iter += 1
            if self.iter_test > 0:
                self.epoch_test += 1
            self.iter_test = 0
            return proposals, losses
        pred_instances, all_scores, all_boxes = self._forward_box(features, proposals, None)
        self.iter_test += 1
        return pred_instances, {}, all_scores, all_boxes

    def _forward_box(self, features, proposals, targets):
        """roi_heads_oicr.py:320-421."""
        pre = self._prefetched
        self._prefetched = None
        if pre is not None:
            nhwc, rois, obj, pooled = None, pre["rois"], pre["obj"], pre["pooled"]
            self._props = (rois, pre.get("props"))
        else:
            nhwc, rois, obj = self._gather_inputs(features, proposals)
            pooled = None
        dev = rois.device
        nper = [len(p) for p in proposals]
        n_img = len(proposals)
        K = self.num_classes
        if self.training:
            ints, _, oh = get_image_level_gt(targets, K)
            self.gt_classes_img_int, self.gt_classes_img_oh = ints, oh
            gmax = max(1, max(len(g) for g in ints))
            gcl = torch.zeros((n_img, gmax), dtype=torch.int32)
            for i, g in enumerate(ints):
                gcl[i, : len(g)] = g.to(torch.int32)
            off = torch.tensor([0] + list(torch.tensor(nper).cumsum(0).tolist()), dtype=torch.int32)
            gt = dict(onehot=oh.to(dev, non_blocking=True), classes=gcl.to(dev, non_blocking=True),
                      count=torch.tensor([len(g) for g in ints], dtype=torch.int32).to(dev, non_blocking=True),
                      props=self._take_props(rois), max_rows=max(nper), rows=nper)
            cap = self._annot_capacity()
            if cap:  # the annotated boxes (metrics ring and / or a regressing PCL branch: ONE block), packed on the host
                words = pack_annotated(targets, cap, self._annot_setter()).to(dev, non_blocking=True)
                gt.update(annotated_views(words, n_img, cap))
            losses, state = self._engine.forward(nhwc, rois, obj, True, off.to(dev, non_blocking=True), n_img, gt,
                                                 pooled=pooled)
            self.pred_class_img_logits = state["aux"]["img_scores"]
            self._last_state = state
            if has_event_storage():  # kept as device scalars: no sync (the reference syncs 3x here)
                st = get_event_storage()
                o1 = obj + 1
                st.put_scalar("proposals/objectness_logits+1 mean", o1.mean())
                st.put_scalar("proposals/objectness_logits+1 max", o1.max())
                st.put_scalar("proposals/objectness_logits+1 min", o1.min())
            return losses
        w, col = self._engine.forward(nhwc, rois, obj, False, pooled=pooled)
        heads = [k for k in range(self.refine_K)]
        props = self._take_props(rois)
        last = self.box_refinery[-1] if self.refine_K else self.box_predictor
        if self.refine_K == 0:
            # WSDDNROIHeads (roi_heads_wsddn.py:305-309 -> WSDDNOutputLayers.inference, fast_rcnn.py:587-608): the MIL
            # scores with a zero background column, zero deltas
            off = torch.tensor([0] + list(torch.tensor(nper).cumsum(0).tolist()), dtype=torch.int32).to(dev)
            zeros = self._zero_onehot(n_img, K, dev)
            sc, _, _ = ops.wsddn_fwd_bwd(w["logits"], col["cls"], col["det"], K, off, n_img, zeros, max_rows=max(nper))
            probs = torch.zeros((sc.shape[0], K + 1), dtype=torch.float32, device=dev)
            probs[:, :K].copy_(sc)
            boxes = ops.apply_deltas(None, props, K, last.box2box_transform.weights)
        elif self.refine_mode == "pcl":
            # roi_heads_pcl.py:342-349 -> inference(pcl_bg=True): the mean softmax of ALL branches, background rotated to the last
            # column, and the decode of the mean of ALL branches' deltas - a non-regressing branch contributes zeros
            # (fast_rcnn.py:1377-1386), so the regressing branches' deltas are divided by REFINE_NUM; the boxes stay in true
            # class order (fast_rcnn.py:1465).  Not OICR's rule below (last branch, undivided).
            probs = ops.mean_softmax(w["logits"], [col["r%d" % k] for k in heads], K + 1, bg_first=True)
            reg = [k for k in heads if self.refine_reg[k]]
            if reg:
                boxes = ops.apply_deltas_mean(w["logits"], [col["b%d" % k] for k in reg], self.refine_K, props, K,
                                              last.box2box_transform.weights)
            else:
                boxes = ops.apply_deltas(None, props, K, last.box2box_transform.weights)
        elif self.refine_reg[-1]:
            probs, _ = ops.softmax_ce(w["logits"], col["r%d" % heads[-1]], K + 1)
            boxes = ops.apply_deltas(w["logits"], props, K, last.box2box_transform.weights, col0=col["b%d" % heads[-1]])
        else:
            probs = ops.mean_softmax(w["logits"], [col["r%d" % k] for k in heads], K + 1,
                                     bg_first=self.refine_mode == "pcl")
            boxes = ops.apply_deltas(None, props, K, last.box2box_transform.weights)
        results, all_scores, all_boxes = [], [], []
        if self.scores_only:
            # GeneralizedRCNNWithTTAAVG's per-augmentation passes use all_scores / all_boxes alone
            # (test_time_augmentation_avg.py:269-294 drops the first return value): no threshold / sort / NMS per pass
            for s, b in zip(probs.split(nper), boxes.split(nper)):
                all_scores.append(s.unsqueeze(0))
                all_boxes.append(b.unsqueeze(0))
            return None, all_scores, all_boxes
        if self.padded_tail is not None:
            # GeneralizedRCNNWSL.inference(padded=True): ONE launch chain for all images, no host read; the value holds the
            # output sizes of detector_postprocess (applied on the device) or None for the raw tail
            results = padded_detections(boxes, probs, nper, [p.image_size for p in proposals],
                                        self.padded_tail.get("output_sizes"), last.test_score_thresh, last.test_nms_thresh,
                                        last.test_topk_per_image)
            for s, b in zip(probs.split(nper), boxes.split(nper)):
                all_scores.append(s.unsqueeze(0))
                all_boxes.append(b.unsqueeze(0))
            return results, all_scores, all_boxes
        for p, s, b in zip(proposals, probs.split(nper), boxes.split(nper)):
            if 1 <= last.test_topk_per_image <= 1024:
                ob, os_, oc, _ = ops.detect_topk(b, s, p.image_size, last.test_score_thresh, last.test_nms_thresh,
                                                 last.test_topk_per_image)
            else:  # negative = every detection (fast_rcnn.py:65,133), or more than the one-wave kernel's 1024: the uncapped tail
                ob, os_, oc, _ = ops.detect_all(b, s, p.image_size, last.test_score_thresh, last.test_nms_thresh,
                                                last.test_topk_per_image)
            r = Instances(p.image_size)
            r.pred_boxes = Boxes(ob)
            r.scores = os_
            r.pred_classes = oc
            results.append(r)
            all_scores.append(s.unsqueeze(0))
            all_boxes.append(b.unsqueeze(0))
        return results, all_scores, all_boxes


@ROI_HEADS_REGISTRY.register()
class PCLROIHeads(OICRROIHeads):
    """roi_heads_pcl.py:28-349: the same trunk, neck, MIL head and K+1-way refinement branches as OICR; the branches
    are trained with the proposal-cluster loss (fast_rcnn.py:1725-1745) instead of the pseudo-GT cross entropy, keep
    the background in column 0, and are averaged with `pcl_bg` at test time (roi_heads_pcl.py:341-349).  The reference
    runs the clustering in numpy / scikit-learn and the loss in C++ on the host; here both stay on the device
    (csrc/pcl.hip)."""

    refine_mode = "pcl"
    ANNOT_MAX_GT = 64    # annotated boxes per image of a regressing branch's label upload, unless set_annotated_capacity() says else
    _annot_cap = None    # what set_annotated_capacity() set

    @property
    def regresses(self):
        """a branch with WSL.REFINE_REG (the reg/pcl_* recipes): box regression onto the ANNOTATED boxes"""
        return any(self.refine_reg[: self.refine_K])

    def set_annotated_capacity(self, max_gt):
        """Annotated boxes per image that the label upload of a regressing head holds (default ANNOT_MAX_GT = 64; an image with more
        raises DrnError on the host).  ONE RULE: with the metrics ring's annotated-box block on (enable_metrics(annotated=True,
        max_gt=)) the ring's max_gt is the capacity - the regression and the ring read one block, uploaded once - and a capacity
        set here that differs from it is refused; without the block the capacity set here (else the default) holds.  A graphed
        step lays its label buffer out when it is primed, so this has to come first."""
        from .. import ops

        if not 1 <= int(max_gt) <= ops.LABEL_MAX_GT:
            raise DrnError("set_annotated_capacity(%d): 1 .. %d annotated boxes per image are built" % (max_gt, ops.LABEL_MAX_GT))
        owner = self._engine.captured_by
        if int(max_gt) != self._annot_capacity_quiet() and owner is not None and owner() is not None:
            raise DrnError("set_annotated_capacity() after a graphed step was primed: its label buffer is laid out.  Order: "
                           "set_annotated_capacity(), then create and prime the GraphedTrainStep / GraphedFullStep")
        self._annot_cap = int(max_gt)
        self._annot_capacity()  # (refuses a contradiction with the ring at once)
        return self

    def _annot_capacity_quiet(self):
        try:
            return self._annot_capacity()
        except DrnError:
            return -1

    def _annot_capacity(self):
        ring_gt = super()._annot_capacity()
        if not self.regresses:
            return ring_gt
        if self.proposal_append_gt:
            raise DrnError("PCLROIHeads with a regressing branch and MODEL.ROI_HEADS.PROPOSAL_APPEND_GT = True: appending the "
                           "annotated boxes to the proposals is not built (every shipped reg/pcl recipe sets it False)")
        if ring_gt:
            if self._annot_cap is not None and self._annot_cap != ring_gt:
                raise DrnError("set_annotated_capacity(%d) contradicts enable_metrics(annotated=True, max_gt=%d): with the "
                               "annotated-box block on, the ring's max_gt is the capacity" % (self._annot_cap, ring_gt))
            return ring_gt
        return self._annot_cap if self._annot_cap is not None else self.ANNOT_MAX_GT

    def _annot_setter(self):
        ring = self._engine.metrics
        if ring is not None and ring.annotated:
            return "enable_metrics(max_gt=%d)"
        return "PCLROIHeads.set_annotated_capacity(%d)"

    @property
    def image_batches(self):
        return bool(self._engine.pcl_image_batches)

    def enable_image_batches(self, on=True):
        """Train on batches of images (off by default: like the reference, a step with more than one image is refused).  On:
        every image is clustered on its own, all of them in one (branch, image) launch; loss_cls_r{k} is the mean over the images
        of the single-image loss - what a data-parallel job with one image per rank optimises - and _last_state["aux"]["targets"]
        holds the per-image target dicts (include/drn_wsod.h, "PCL refinement on image batches"; at most ops.PCL_MAX_IMAGES
        images of at most 4096 proposals).  A graphed step freezes its launch sequence when it is primed, so this has to come
        first: enable_image_batches() -> build / prime the GraphedTrainStep."""
        eng = self._engine
        owner = eng.captured_by
        if bool(on) != self.image_batches and owner is not None and owner() is not None:
            raise DrnError("enable_image_batches() after a graphed step was primed: its captured launches are the other path's.  "
                           "Order: enable_image_batches(), then create and prime the GraphedTrainStep / GraphedFullStep")
        eng.pcl_image_batches = bool(on)
        return self


@ROI_HEADS_REGISTRY.register()
class WSDDNROIHeads(OICRROIHeads):
    """roi_heads_wsddn.py: the MIL head alone (no refinement branches); inference scores are the MIL scores
    (WSDDNOutputLayers.inference, fast_rcnn.py:587-608)."""

    _refine_from_cfg = False


def csc_slot_schedule(labelled, img_scores, tau):
    """The image-gradient passes of one CSC step on an image batch (pure host function; include/drn_wsod.h, "CSC on image
    batches").  labelled[i]: the labelled classes of image i; img_scores[i][c]: its image-level scores; tau: the threshold a
    class has to reach to get a map.  ->
      active  per image the ascending labelled classes with score >= tau
      slots   S = max_i |active[i]| rows of one class per image: slots[j][i] = active[i][j], or -1 where image i has fewer
              (one d/dx pass over the whole batch per row)
      pairs   every (image, labelled class), active or not: a labelled class below tau keeps a zero map and still goes through
              the weights op, as in the reference"""
    labelled = [sorted({int(c) for c in L}) for L in labelled]
    active = [[c for c in L if img_scores[i][c] >= tau] for i, L in enumerate(labelled)]
    n_slots = max([len(a) for a in active] or [0])
    slots = [[a[j] if j < len(a) else -1 for a in active] for j in range(n_slots)]
    pairs = [(i, c) for i, L in enumerate(labelled) for c in L]
    return dict(active=active, slots=slots, pairs=pairs)


@ROI_HEADS_REGISTRY.register()
class CSCROIHeads(OICRROIHeads):
    """roi_heads_csc.py:40-551: the WSDDN MIL head trained with two image-level BCE losses on CSC-weighted score sums.
    Per labelled class whose image score reaches `tau`, the gradient of the summed class score w.r.t. the (normalised)
    input image gives a saliency map (`_forward_cpg`: here the d/dx half of the explicit backward through the predictor,
    fc7, fc6, RoIPool and EVERY trunk layer down to the pixels); the map, thresholded and summed into a table, scores
    each proposal by its frame / context contrast (CSCPool) and becomes the signed weight W (csc.hip).  After
    WSL.CSC_MAX_ITER iterations W_pos = 1, W_neg = 0.  Inference is WSDDN's.  Debug dumps (`_save_mask`) are the
    reference's control plane and are not rebuilt; its `Statistic` log (csc.txt) is enable_csc_stats()."""

    _refine_from_cfg = False
    csc_head = True

    @configurable
    def __init__(self, *, csc_max_iter=35000, **kwargs):
        super().__init__(**kwargs)
        self.csc_max_iter = csc_max_iter
        self.tau, self.fg_threshold, self.bg_threshold = 0.7, 0.1, 0.005  # roi_heads_csc.py:107-109
        self.context_scale, self.area_sqrt = 1.8, True  # :110-118 (mass / density thresholds are unused by the op)
        self.image_grad_fn = None  # set by GeneralizedRCNNWSL: feature-map gradient -> image gradient (NHWC)
        self._image_batches = False  # enable_image_batches()
        # what the last training forward built maps for: the active classes of the one image (a list), the CscBatchPlan of an
        # image batch, None past CSC_MAX_ITER.  Read by the weight statistics (enable_csc_stats), which are handed the decision.
        self._csc_sched = None

    @classmethod
    def from_config(cls, cfg, input_shape):
        ret = super().from_config(cfg, input_shape)
        ret["csc_max_iter"] = cfg.WSL.CSC_MAX_ITER
        return ret

    def prefetch_pooled(self, features, proposals):
        raise DrnError("the CSC head differentiates through RoIPool and the trunk: no prefetched operands")

    def enable_csc_stats(self, period=320, output_dir=None, prefix="", start_iter=0):
        """Record the reference's CSC weight statistics (`Statistic`, third_party/cpg_stats.py, driven from CSCOutputs.csc_loss,
        fast_rcnn.py:910-918) on the device: per labelled class how many proposals W marks positive / negative / leaves at zero
        and how the score mass splits between them.  Every training forward up to WSL.CSC_MAX_ITER adds to a table in device
        memory (drn_csc_stats: two small launches once W is final, nothing is read back); after every `period`-th forward - the
        reference's LOG_PERIOD = 1280 / 4 - the table is copied to pinned memory on the heads' stream and re-zeroed, and the
        decoded block is appended to <output_dir>/<prefix>csc.txt (output_dir None: kept in CscStats.blocks only).  start_iter:
        the training-forward count the log continues from (a resumed job).  Returns the metrics.CscStats.  Off by default:
        without this call no launch, buffer or upload of a step changes.  Every rank writes its own file."""
        from ..metrics import CscStats

        eng = self._engine
        eng.ensure(next(self.parameters()).device)
        eng.csc_stats = CscStats(self.num_classes, self.csc_max_iter, period, output_dir, prefix, start_iter, eng.arena_w.device)
        return eng.csc_stats

    def disable_csc_stats(self):
        """back to the launch sequence without the statistics; what was drained stays collectable on the returned object"""
        eng = self._engine
        st, eng.csc_stats = eng.csc_stats, None
        return st

    def _csc_weights(self, eng, w, col, scores, rowsm, M, dtype, fg, masks, drop_p):
        """roi_heads_csc.py:423-510 (_forward_cpg + _forward_csc). Returns (W [M, K] or None past CSC_MAX_ITER, cpgs)."""
        K = self.num_classes
        self._csc_sched = None
        if self.iter > self.csc_max_iter:
            return None, None
        if self.image_grad_fn is None:
            raise DrnError("CSCROIHeads needs the meta-architecture's image-gradient pass (GeneralizedRCNNWSL with cpg)")
        H, Wd = self.images.image_sizes[0]
        if tuple(self.images.nhwc.shape[1:3]) != (H, Wd):
            raise DrnError("CSC maps are image-sized: the padded batch tensor must equal the image (one image per step)")
        dev = scores.device
        labelled = [int(c) for c in self.gt_classes_img_int[0].tolist()]
        # the reference branches on the image score per class on the host too (roi_heads_csc.py:445): one read of K floats
        img = scores.sum(dim=0).tolist()
        cpgs = torch.zeros((K, H, Wd), dtype=torch.float32, device=dev)
        W = torch.ones((M, K), dtype=torch.float32, device=dev)
        table = torch.empty((H, Wd), dtype=torch.float32, device=dev)
        first = True
        self._csc_sched = [c for c in labelled if img[c] >= self.tau]  # the classes this step builds a map for
        for c in labelled:
            if img[c] >= self.tau:
                ops.csc_loss(w["logits"], col["cls"], col["det"], K, scores, rowsm, None, None,
                             self.box_predictor.mean_loss, dlogits=w["dlogits"], seed_class=c)
                dfeat = eng.input_gradient(w, M, dtype, fg, masks, drop_p, refresh_w1t=first)
                first = False
                ops.csc_cpg(self.image_grad_fn(dfeat), 3, out=cpgs[c])
            # (a labelled class below tau keeps a zero map and still goes through the op, as in the reference)
            ops.csc_weights(cpgs[c], self.fg_threshold, fg["rois"], scores, c, self.area_sqrt, self.context_scale, W, table)
        return W, cpgs

    @property
    def image_batches(self):
        return self._image_batches

    def enable_image_batches(self, on=True):
        """Train on batches of images (off by default: like the reference, a step with more than one image is refused).  On:
        every image gets the maps of its own labelled classes from its own crop of the batch's image gradient - slot j of the
        step carries the j-th active class of EVERY image through one d/dx pass, so a step costs max_i |active_i| passes
        instead of their sum; loss_cls_pos / loss_cls_neg are the mean over the images of the single-image losses - what a
        data-parallel job with one image per rank optimises - and _last_state["aux"]["cpgs"] is a list of [K, H_i, W_i] maps
        (include/drn_wsod.h, "CSC on image batches"; at most ops.CSC_MAX_IMAGES images).  Graphed steps stay refused."""
        self._image_batches = bool(on)
        return self

    def _csc_weights_batch(self, eng, s, scores, rowsm):
        """_csc_weights for the n_img images of an opted-in step -> (W [M, K] or None past CSC_MAX_ITER, list of maps or None)"""
        K, n, w, col = self.num_classes, s.n_img, s.w, s.col
        sizes = [(int(hw[0]), int(hw[1])) for hw in self.images.image_sizes]
        ops.csc_batch_limits(n, K, sizes)
        self._csc_sched = None
        if self.iter > self.csc_max_iter:
            return None, None
        if self.image_grad_fn is None:
            raise DrnError("CSCROIHeads needs the meta-architecture's image-gradient pass (GeneralizedRCNNWSL with cpg)")
        if len(sizes) != n or self.images.nhwc.shape[0] != n:
            raise DrnError("CSC image batch: %d images for %d proposal lists" % (len(sizes), n))
        dev = scores.device
        # the one host read of the step: n * K image scores, each image's the column sum the single-image head reads
        bounds = [0]
        for r in s.gt["rows"]:
            bounds.append(bounds[-1] + r)
        img = torch.stack([scores[a:b].sum(dim=0) for a, b in zip(bounds[:-1], bounds[1:])]).tolist()
        sched = csc_slot_schedule([g.tolist() for g in self.gt_classes_img_int], img, self.tau)
        plan = self._csc_sched = ops.CscBatchPlan(sizes, K, sched["slots"], sched["pairs"], dev)  # (the one upload)
        flat, cpgs = plan.new_maps(dev)
        W = torch.ones((s.M, K), dtype=torch.float32, device=dev)
        for j in range(len(plan.slots)):
            ops.csc_seed_batch(w["logits"], col["cls"], col["det"], K, scores, rowsm, s.img_off, n, plan.d_slots[j], w["dlogits"])
            dfeat = eng.input_gradient(w, s.M, s.dtype, s.fg, s.masks, s.drop_p, refresh_w1t=j == 0)
            ops.csc_cpg_batch(self.image_grad_fn(dfeat), 3, plan, j, flat)
        ops.csc_weights_batch(flat, plan, self.fg_threshold, s.fg["rois"], s.img_off, scores, self.area_sqrt,
                              self.context_scale, W)
        return W, cpgs


def build_roi_heads(cfg, input_shape):
    return ROI_HEADS_REGISTRY.get(cfg.MODEL.ROI_HEADS.NAME)(cfg, input_shape)
