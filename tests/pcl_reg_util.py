"""CPU restatement of the reg/pcl recipes (PCLROIHeads with WSL.REFINE_REG branches), composed of existing oracle pieces - nothing
under oracle/ changes:

  training   roi_heads_pcl.py:227-334: the proposals are labelled against the ANNOTATED boxes (O.label_proposals), every branch gets
             the proposal-cluster loss (pcl_oracle.pcl_refine_loss through O._PclLossFn) on the previous branch's probabilities,
             and a branch with REFINE_REG adds loss_box_reg_r{k} = O.oicr_box_reg_loss of its deltas against
             O.get_deltas(proposal, matched ANNOTATED box) - PCL never relabels against pseudo ground truth.  The regression feeds
             nothing back into the clustering.
  inference  roi_heads_pcl.py:342-349: mean softmax over ALL branches, background rotated to the last column; boxes =
             O.apply_deltas(mean over ALL branches of their deltas, proposals), where a non-regressing branch contributes zeros -
             with flags [F, F, F, T] the regressing branch's deltas divided by 4.  The boxes are not rotated.

The kernel-level functions (annot_box_reg, mean_deltas) take tensors of any float dtype and are what tests/test_pcl_reg_gpu.py runs in
fp64 on the kernels' fp32 inputs; the labelling is always done in fp32, torch's own arithmetic (annot_metrics_util.label_proposals),
because the labels are defined by fp32 IoUs.  The model flow runs in the oracle's dtype.
tests/golden/gen_golden_pcl_reg.py holds this restatement against the unmodified reference."""
import numpy as np
import torch
import torch.nn.functional as F

import annot_metrics_util as AU
import golden_util as G

O = G.O

NAME = "model_pcl_reg_r50c4_tiny"
YAML = "PascalVOC-Detection/reg/pcl_WSR_50_DC5_1x.yaml"
REG_YAMLS = tuple("PascalVOC-Detection/reg/pcl_%s_DC5_1x.yaml" % a for a in ("V_16", "WSR_18", "WSR_50", "WSR_101"))


def ocfg():
    """the fixture's oracle config: model_pcl_r50c4_tiny's plus REFINE_NUM 4 / REFINE_REG [F, F, F, T] (a fresh object per call)"""
    return O.OracleCfg(arch="wsr50", out_feature="res4", res5_dilation=1, heads="pcl", refine_num=4,
                       refine_reg=(False, False, False, True), dropout=0.0, **G.TINY)


# ------------------------------------------------------------------------------------------------------------------ kernel level
def annot_box_reg(logits, col0s, K, props, img_off, gt_boxes, gt_classes, gt_count, thresholds, match_labels, weights,
                  loss_scale=1.0):
    """include/drn_wsod.h drn_annot_box_reg in the dtype of `logits` (fp64 in the tests).  logits [M, ld], props [M, 4] (the fp32
    values, any dtype), gt_boxes [n_img, max_gt, 4] / gt_classes / gt_count as packed (AU.pack).
    -> dict(loss [n_heads] (python floats), labels, matched (int64 [M]), absdiff [n_heads][M, 4] (|pred - target| on fg rows, else
    0), sign [n_heads][M, 4], grad_scale [M] (1 / M_i / n_img * loss_scale as exact fp32 products), terms (sum |.| in fp64))."""
    props32 = np.asarray(props, dtype=np.float32)
    gb32, gc, cnt = np.asarray(gt_boxes, dtype=np.float32), np.asarray(gt_classes), np.asarray(gt_count)
    labels, matched, _ = AU.label_proposals(props32, img_off, gb32, gc, cnt, K, thresholds, match_labels)
    labels, matched = np.asarray(labels, dtype=np.int64), np.asarray(matched, dtype=np.int64)
    M, n_img, dt = props32.shape[0], len(img_off) - 1, logits.dtype
    lab_t = torch.from_numpy(labels)
    img_of = np.zeros(M, dtype=np.int64)
    for i in range(n_img):
        img_of[img_off[i]: img_off[i + 1]] = i
    tgt_boxes = torch.from_numpy(gb32[img_of, matched]).to(dt)  # the matched annotated box of every row
    p_t = torch.from_numpy(props32).to(dt)
    fg = (lab_t >= 0) & (lab_t < K)
    tgt = torch.zeros((M, 4), dtype=dt)
    if fg.any():
        tgt[fg] = O.get_deltas(p_t[fg], tgt_boxes[fg], weights)
    out = dict(labels=labels, matched=matched, fg=fg.numpy(), target=tgt, loss=[], absdiff=[], sign=[], terms=[])
    gs = np.zeros(M, dtype=np.float32)
    for i in range(n_img):
        mi = img_off[i + 1] - img_off[i]
        if mi:
            gs[img_off[i]: img_off[i + 1]] = (np.float32(1.0) / np.float32(mi) * (np.float32(1.0) / np.float32(n_img)) *
                                             np.float32(loss_scale))
    out["grad_scale"] = gs
    cls = torch.where(fg, lab_t, torch.zeros_like(lab_t))
    for c0 in col0s:
        cols = c0 + 4 * cls[:, None] + torch.arange(4)
        pred = torch.gather(logits, 1, cols)
        diff = torch.where(fg[:, None], pred - tgt, torch.zeros_like(pred))
        per_img = []
        for i in range(n_img):
            a, b = int(img_off[i]), int(img_off[i + 1])
            if b > a:
                lab_i, pr_i = lab_t[a:b], logits[a:b, c0: c0 + 4 * K]
                if bool(fg[a:b].any()):  # (O.oicr_box_reg_loss is the reference's statement of the per-image loss)
                    per_img.append(float(O.oicr_box_reg_loss(pr_i, lab_i, p_t[a:b], tgt_boxes[a:b], K, _W(weights))))
                else:
                    per_img.append(0.0)
            else:
                per_img.append(0.0)
        out["loss"].append(sum(per_img) / n_img)
        out["per_image"] = per_img
        out["absdiff"].append(diff.abs())
        out["sign"].append(torch.sign(diff))
        out["terms"].append(float(diff.abs().double().sum()))
    return out


class _W:
    """the one field O.oicr_box_reg_loss reads of its config"""

    def __init__(self, weights):
        self.bbox_weights = tuple(weights)


def mean_deltas(logits, col0s, K, n_total):
    """the fp32 mean drn_apply_deltas_mean decodes, computed by torch: ((+0 + d_k0) + d_k1 + ...) / n_total"""
    d = torch.zeros((logits.shape[0], 4 * K), dtype=torch.float32)
    for c0 in col0s:
        d = d + logits[:, c0: c0 + 4 * K]
    return d / torch.tensor(float(n_total), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------------------- model level
def roi_heads_train(p, feat, prop_boxes, objectness, gt_classes_list, gt_boxes_list, cfg, dropout_masks=None, return_aux=False):
    """roi_heads_pcl.py:227-334 with WSL.REFINE_REG branches; O.roi_heads_train's PCL flow plus the annotated-box labelling and
    the box regression loss.  One image per step (third_party/pcl.py:94)."""
    K = cfg.num_classes
    assert len(prop_boxes) == 1
    nper = [len(b) for b in prop_boxes]
    _, gt_oh = O.get_image_level_gt(gt_classes_list, K)
    pooled = O.pool_features(feat, prop_boxes, cfg)
    obn = torch.cat([o + 1 for o in objectness], dim=0)
    pooled = O._q(pooled * obn.view(-1, 1, 1, 1), cfg)
    x = O.dan_forward(p, pooled, cfg, True, dropout_masks)
    scores = O.wsddn_scores(p, x, nper, cfg=cfg)
    losses = {"loss_cls": O.wsddn_loss(scores, nper, gt_oh, cfg.mean_loss)}
    # roi_heads_pcl.py:233-235: labels against the ANNOTATED boxes, true class indexing (background K, ignore -1)
    gc, matched, gb = O.label_proposals(prop_boxes[0], gt_boxes_list[0], gt_classes_list[0], K, cfg)
    aux = {"scores": scores, "labels": gc, "matched": matched, "gt_boxes": gb, "pcl": [], "logits": [], "deltas": {}}
    last = scores.detach().numpy()
    for k in range(cfg.refine_num):
        pre = "roi_heads.box_refinery_%d." % k
        logits = O._head_linear(x, p[pre + "cls_score.weight"], p[pre + "cls_score.bias"], cfg)
        loss, tg, probs = O._PclLossFn.apply(logits, prop_boxes[0].numpy(), last, gt_oh[0].numpy())
        losses["loss_cls_r%d" % k] = loss
        if cfg.refine_reg[k]:
            deltas = O._head_linear(x, p[pre + "bbox_pred.weight"], p[pre + "bbox_pred.bias"], cfg)
            losses["loss_box_reg_r%d" % k] = O.oicr_box_reg_loss(deltas, gc, prop_boxes[0], gb, K, cfg)
            aux["deltas"][k] = deltas
        aux["logits"].append(logits)
        aux["pcl"].append(tg)
        last = probs  # (pcl_loss() clusters the proposals, never refined boxes: no feedback from the regression)
    return (losses, aux) if return_aux else losses


def model_train_losses(p, batch, cfg, dropout_masks=None, return_aux=False):
    x, _ = O.preprocess_image([b["image"] for b in batch], cfg)
    feat = O.backbone_forward(p, x, cfg)
    return roi_heads_train(p, feat, [b["proposal_boxes"] for b in batch], [b["objectness_logits"] for b in batch],
                           [b["gt_classes"] for b in batch], [b["gt_boxes"] for b in batch], cfg, dropout_masks, return_aux)


def train_step(p, batch, cfg, opt, dropout_masks=None, freeze_at=5, return_aux=False):
    """O.train_step around this module's losses: fwd, sum of losses, bwd, SGD step -> (losses, grads[, aux])"""
    names = O.trainable_names(p, cfg, freeze_at)
    leaves = {n: p[n].detach().clone().requires_grad_(True) for n in names}
    q = dict(p)
    q.update(leaves)
    losses, aux = model_train_losses(q, batch, cfg, dropout_masks, True)
    total = sum(losses.values())
    gl = torch.autograd.grad(total, [leaves[n] for n in names], allow_unused=True)
    grads = {n: (g if g is not None else torch.zeros_like(p[n])) for n, g in zip(names, gl)}
    opt.step(p, grads)
    out = {k: float(v.detach()) for k, v in losses.items()}
    return (out, grads, aux) if return_aux else (out, grads)


def model_inference(p, batch, cfg, rule="pcl"):
    """rcnn.py:199-240 + roi_heads_pcl.py:342-349.  rule: "pcl" (the reference's: mean of all branches' deltas, zeros for the
    non-regressing ones), or one of the two WRONG rules the golden must tell apart - "last" (OICR's: the last branch undivided),
    "all_layers" (the mean over all bbox_pred layers, used or not)."""
    x, sizes = O.preprocess_image([b["image"] for b in batch], cfg)
    feat = O.backbone_forward(p, x, cfg)
    prop_boxes = [b["proposal_boxes"] for b in batch]
    K = cfg.num_classes
    nper = [len(b) for b in prop_boxes]
    pooled = O.pool_features(feat, prop_boxes, cfg)
    obn = torch.cat([b["objectness_logits"] + 1 for b in batch], dim=0)
    x = O.dan_forward(p, pooled * obn.view(-1, 1, 1, 1), cfg, False)
    props_cat = torch.cat(prop_boxes, dim=0)
    probs, deltas = None, torch.zeros(x.shape[0], 4 * K)
    for k in range(cfg.refine_num):
        pre = "roi_heads.box_refinery_%d." % k
        pk = F.softmax(F.linear(x, p[pre + "cls_score.weight"], p[pre + "cls_score.bias"]), dim=-1)
        probs = pk if probs is None else probs + pk
        dk = O._head_linear(x, p[pre + "bbox_pred.weight"], p[pre + "bbox_pred.bias"], cfg)
        if rule == "all_layers" or (rule == "pcl" and cfg.refine_reg[k]):
            deltas = deltas + dk
        elif rule == "last" and k == cfg.refine_num - 1:
            deltas = dk * cfg.refine_num  # (divided again below: the branch's deltas as they are)
    probs = probs / cfg.refine_num
    deltas = deltas / cfg.refine_num
    probs = torch.cat((probs[:, 1:], probs[:, :1]), dim=1)  # pcl_bg; the boxes stay in true class order (fast_rcnn.py:1465)
    boxes = O.apply_deltas(deltas, props_cat, cfg.bbox_weights)
    res = []
    for b, s, sz in zip(boxes.split(nper), probs.split(nper), sizes):
        res.append(O.fast_rcnn_inference_single_image(b, s, sz, cfg.score_thresh, cfg.nms_thresh, cfg.topk))
    return res, list(probs.split(nper)), list(boxes.split(nper))


def scale_bbox_pred(p, factor, cfg):
    """the inference record's parameters: the bbox_pred WEIGHTS of all branches times `factor` (a dict of the same tensors else)"""
    q = dict(p)
    for k in range(cfg.refine_num):
        n = "roi_heads.box_refinery_%d.bbox_pred.weight" % k
        q[n] = p[n] * factor
    return q


# ------------------------------------------------------------------------------------------------- inputs of the kernel-level tests
KERNEL_M, KERNEL_K, KERNEL_NIMG, KERNEL_MAX_GT, KERNEL_HEADS = (1, 255, 256, 257, 513), (1, 4, 20), (1, 3), (1, 64, 256), (1, 3)
KERNEL_THR = (((0.5,), (0, 1)), ((0.1, 0.5), (-1, 0, 1)))
GRAD_RULE = 1e-5  # a foreground entry is checked exactly when its fp64 |pred - target| exceeds GRAD_RULE * max(1, |target|)


def kernel_case(M, K, n_img, max_gt, n_heads, seed=0):
    """Inputs of one kernel-level case, fp32, built on the CPU from a fixed seed.  n_img = 3: image 0 has ONE row, image 1 has no
    annotated box, image 2 the rest (unequal row counts; M = 1 leaves images 1 and 2 without rows).  Every coordinate is a multiple
    of 1/4 below 512, so widths, heights and centres are exact in fp32 and an fp32 target is within a few ulp of the fp64 one - far
    inside GRAD_RULE; roughly 60 % of the rows are shifted copies of an annotated box (foreground at 0.5), some exact copies (IoU 1),
    and with two or more boxes box 1 duplicates box 0 under another class (the lowest-index tie rule).  Logits: N(0, 2) in the
    heads' delta columns of a wider row, NaN everywhere else.
    -> dict(logits [M + 1, ld], col0s, ld, props [M, 4], img_off, rows, gt_boxes, gt_classes, gt_count)"""
    rs = np.random.RandomState(seed + 7919 * M + 131 * K + 17 * n_img + max_gt + 3 * n_heads)
    rows = [M] if n_img == 1 else [1, (M - 1) // 3, M - 1 - (M - 1) // 3]
    img_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    q = lambda a: np.round(np.asarray(a) * 4.0) / 4.0
    boxes_pi, cls_pi = [], []
    props = np.zeros((M, 4), dtype=np.float32)
    for i in range(n_img):
        G = 0 if (n_img == 3 and i == 1) else (max_gt if i == n_img - 1 else int(rs.randint(1, max_gt + 1)))
        xy = q(rs.uniform(0, 380, (G, 2)))
        wh = q(rs.uniform(16, 120, (G, 2)))
        gb = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        gc = rs.randint(0, K, G).astype(np.int32)
        if G >= 2:
            gb[1] = gb[0]
            gc[1] = (gc[0] + 1) % K  # (K = 1: the same class - the tie still shows in `matched`)
        boxes_pi.append(gb)
        cls_pi.append(gc)
        for r in range(int(img_off[i]), int(img_off[i + 1])):
            u = rs.rand()
            if G and u < 0.6:
                g = gb[rs.randint(0, G)]
                w, h = g[2] - g[0], g[3] - g[1]
                j = q(rs.uniform(-1, 1, 4) * np.array([w, h, w, h]) / 8.0) if u > 0.05 else np.zeros(4)
                props[r] = np.clip(g + j, 0, 511.75)
            else:
                xy1 = q(rs.uniform(0, 380, 2))
                props[r] = np.concatenate([xy1, xy1 + q(rs.uniform(8, 120, 2))])
    gt_boxes, gt_classes, gt_count = AU.pack(boxes_pi, cls_pi, max_gt)
    pad = 3
    ld = pad + n_heads * (4 * K + 2) + 5
    col0s = [pad + h * (4 * K + 2) for h in range(n_heads)]
    logits = torch.full((M + 1, ld), float("nan"))
    for c0 in col0s:
        logits[:M, c0: c0 + 4 * K] = torch.from_numpy(rs.standard_normal((M, 4 * K)).astype(np.float32) * 2)
    return dict(logits=logits, col0s=col0s, ld=ld, props=torch.from_numpy(props), img_off=img_off, rows=rows,
                gt_boxes=gt_boxes, gt_classes=gt_classes, gt_count=gt_count)


def kernel_reference(c, K, thr, lab, weights=(10.0, 10.0, 5.0, 5.0), loss_scale=1.0):
    """the fp64 restatement on a kernel_case's fp32 inputs, plus which foreground entries the gradient rule checks"""
    M = c["props"].shape[0]
    lg = torch.nan_to_num(c["logits"][:M].double(), nan=0.0)  # (the NaN padding is never gathered: the heads' columns are finite)
    r = annot_box_reg(lg, c["col0s"], K, c["props"].numpy(), c["img_off"].tolist(), c["gt_boxes"], c["gt_classes"], c["gt_count"],
                      thr, lab, weights, loss_scale)
    tol = GRAD_RULE * torch.clamp(r["target"].abs(), min=1.0)
    fg = torch.from_numpy(r["fg"])
    r["checked"] = [(a > tol) & fg[:, None] for a in r["absdiff"]]
    r["n_fg_entries"] = int(fg.sum()) * 4
    return r
