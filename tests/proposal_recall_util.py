"""Test infrastructure of the box-proposal recall evaluator: a plain numpy restatement of the reference's
_evaluate_box_proposals (detectron2/evaluation/coco_evaluation.py:372-480, cited below) with this package's three rules
(stable objectness order; first index wins among proposals and among boxes; include/drn_wsod.h), plus the loaders of
tests/golden/proposal_recall.npz (written by tests/golden/gen_golden_proposal_recall.py from the unmodified function).

A case is a dict of flat arrays:
  img_ids [I]                      image ids in the order the ops-level tests lay the images out
  gt_img [G] image id, gt_box [G, 4] f64 XYWH, gt_area [G] f64, gt_crowd [G] u8          in annotation order
  pr_img [n] image id, pr_box [n, 4] f32 XYXY, pr_logit [n] f32                           an image's rows in input order
and its golden results, over AREA_NAMES x LIMITS in that order (pair q = a * len(LIMITS) + l):
  ov, ov_off [A * L + 1]           the pairs' sorted gt_overlaps, concatenated
  recalls [A, L, T] f32, ar [A, L] f32, num_pos [A, L] i64"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proposal_recall.npz")
CASES = ("ties", "wide", "plain")
INPUT_KEYS = ("img_ids", "gt_img", "gt_box", "gt_area", "gt_crowd", "pr_img", "pr_box", "pr_logit")
RESULT_KEYS = ("ov", "ov_off", "recalls", "ar", "num_pos")

# coco_evaluation.py:380-399
AREA_NAMES = ("all", "small", "medium", "large", "96-128", "128-256", "256-512", "512-inf")
AREA_RANGES = {"all": [0 ** 2, 1e5 ** 2], "small": [0 ** 2, 32 ** 2], "medium": [32 ** 2, 96 ** 2], "large": [96 ** 2, 1e5 ** 2],
               "96-128": [96 ** 2, 128 ** 2], "128-256": [128 ** 2, 256 ** 2], "256-512": [256 ** 2, 512 ** 2],
               "512-inf": [512 ** 2, 1e5 ** 2]}
LIMITS = (1, 4, 20, 64, None)


def default_thresholds():
    import torch

    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)  # :465-467


def load_case(name):
    d = np.load(GOLDEN, allow_pickle=False)
    pre = name + "_"
    return {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}


def golden_pair(case, area, limit):
    q = AREA_NAMES.index(area) * len(LIMITS) + LIMITS.index(limit)
    a, l = divmod(q, len(LIMITS))
    return dict(gt_overlaps=case["ov"][case["ov_off"][q]:case["ov_off"][q + 1]], recalls=case["recalls"][a, l],
                ar=case["ar"][a, l], num_pos=int(case["num_pos"][a, l]))


def pairwise_iou(p, g):
    """detectron2/structures/boxes.py:329-361 in float32, operation for operation -> [len(p), len(g)]"""
    p, g = p.astype(np.float32).reshape(-1, 4), g.astype(np.float32).reshape(-1, 4)
    a1 = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    a2 = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    wh = np.minimum(p[:, None, 2:], g[:, 2:]) - np.maximum(p[:, None, :2], g[:, :2])
    wh = np.maximum(wh, np.float32(0))
    inter = wh[:, :, 0] * wh[:, :, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (a1[:, None] + a2 - inter)
    return np.where(inter > 0, iou, np.float32(0)).astype(np.float32)


def images_of(case, image_order=None):
    """-> [(proposal boxes f32 XYXY, logits f32, gt boxes f32 XYXY, gt areas f32)] per image: the annotations that are not
    crowd, XYWH -> XYXY by one fp32 addition per corner (BoxMode.convert of a python list, boxes.py:63,111-113)"""
    out = []
    for iid in (case["img_ids"] if image_order is None else image_order):
        gs = np.nonzero((case["gt_img"] == iid) & (case["gt_crowd"] == 0))[0]
        b = case["gt_box"][gs].astype(np.float32).reshape(-1, 4)
        gb = np.stack([b[:, 0], b[:, 1], b[:, 2] + b[:, 0], b[:, 3] + b[:, 1]], 1).astype(np.float32)
        ps = np.nonzero(case["pr_img"] == iid)[0]
        out.append((case["pr_box"][ps].astype(np.float32).reshape(-1, 4), case["pr_logit"][ps].astype(np.float32), gb,
                    case["gt_area"][gs].astype(np.float32)))
    return out


def match_image(pb, pl, gb, ga, area, limit):
    """One image of the loop :405-459 -> (the image's recorded entries f32, or None when it is skipped; its num_pos)"""
    if len(gb) == 0 or len(pb) == 0:  # :424-425
        return None, 0
    lo, hi = (np.float32(v) for v in AREA_RANGES[area])
    gb = gb[(ga >= lo) & (ga <= hi)]  # :427-428
    if len(gb) == 0:  # :432-433
        return np.zeros(0, np.float32), 0
    pb = pb[np.argsort(-pl, kind="stable")]  # :410, equal logits in input order
    if limit is not None and len(pb) > limit:
        pb = pb[:limit]
    ov = pairwise_iou(pb, gb)
    ent = np.zeros(len(gb), np.float32)
    for j in range(min(len(pb), len(gb))):
        arg = ov.argmax(0)  # the first index of the maximum, as torch.max on the CPU
        mx = ov[arg, np.arange(ov.shape[1])]
        g = int(mx.argmax())
        ent[j] = mx[g]
        ov[arg[g], :] = -1
        ov[:, g] = -1
    return ent, len(gb)


def aggregate(gt_overlaps, num_pos, thresholds=None):
    """:460-480 with the reference's torch expressions -> its dict, as numpy"""
    import torch

    ov, _ = torch.sort(torch.from_numpy(np.asarray(gt_overlaps, np.float32)))
    thr = default_thresholds() if thresholds is None else thresholds
    recalls = torch.zeros_like(thr)
    for i, t in enumerate(thr):
        recalls[i] = (ov >= t).float().sum() / float(num_pos)
    return dict(ar=recalls.mean().numpy(), recalls=recalls.numpy(), thresholds=thr.numpy(), gt_overlaps=ov.numpy(),
                num_pos=int(num_pos))


def evaluate_numpy(case, area="all", limit=None, thresholds=None):
    ents, num_pos = [], 0
    for pb, pl, gb, ga in images_of(case):
        e, n = match_image(pb, pl, gb, ga, area, limit)
        num_pos += n
        if e is not None:
            ents.append(e)
    return aggregate(np.concatenate(ents) if ents else np.zeros(0, np.float32), num_pos, thresholds)


def flat_inputs(case, image_order=None):
    """what ops.proposal_recall takes, as numpy: the images in img_ids order (or image_order)"""
    imgs = images_of(case, image_order)
    cat = lambda k, shape, dt: (np.concatenate([im[k] for im in imgs]) if imgs else np.zeros(0)).astype(dt).reshape(shape)
    off = lambda k: np.concatenate([[0], np.cumsum([len(im[k]) for im in imgs])]).astype(np.int32)
    return dict(prop_box=cat(0, (-1, 4), np.float32), prop_logit=cat(1, (-1,), np.float32), prop_off=off(1),
                gt_box=cat(2, (-1, 4), np.float32), gt_area=cat(3, (-1,), np.float32), gt_off=off(3))


def area_array(areas):
    return np.array([AREA_RANGES[a] for a in areas], np.float32).reshape(-1, 2)


def limit_array(limits):
    return np.array([0 if l is None else l for l in limits], np.int32)


def device_layout(f, areas, limits, thresholds):
    """the three arrays drn_proposal_recall writes for the flat inputs f: overlaps [A, L, G] (-1 = not an entry), counts
    [A, L, T], num_pos [A]"""
    G, I, thr = len(f["gt_area"]), len(f["gt_off"]) - 1, np.asarray(thresholds, np.float32)
    ov = np.full((len(areas), len(limits), G), -1, np.float32)
    counts = np.zeros((len(areas), len(limits), len(thr)), np.int64)
    num_pos = np.zeros(len(areas), np.int64)
    for i in range(I):
        g0, g1, p0, p1 = f["gt_off"][i], f["gt_off"][i + 1], f["prop_off"][i], f["prop_off"][i + 1]
        for a, area in enumerate(areas):
            for l, limit in enumerate(limits):
                e, n = match_image(f["prop_box"][p0:p1], f["prop_logit"][p0:p1], f["gt_box"][g0:g1], f["gt_area"][g0:g1], area,
                                   limit)
                if e is None:
                    continue
                ov[a, l, g0:g0 + len(e)] = e
                counts[a, l] += (e[None, :] >= thr[:, None]).sum(1)
                if l == 0:
                    num_pos[a] += n
    return ov, counts, num_pos


def annotations_of(case):
    """the COCO-format dict of a case's ground truth"""
    return {"images": [{"id": int(i)} for i in case["img_ids"]], "categories": [{"id": 1, "name": "object"}],
            "annotations": [{"id": q + 1, "image_id": int(case["gt_img"][q]), "category_id": 1,
                             "bbox": [float(v) for v in case["gt_box"][q]], "area": float(case["gt_area"][q]),
                             "iscrowd": int(case["gt_crowd"][q])} for q in range(len(case["gt_img"]))]}


def proposals_of(case, iid, structures, device="cpu"):
    """the Instances of one image's proposals"""
    import torch

    sel = np.nonzero(case["pr_img"] == iid)[0]
    return structures.Instances((480, 640),
                                proposal_boxes=structures.Boxes(torch.from_numpy(case["pr_box"][sel].reshape(-1, 4)).to(device)),
                                objectness_logits=torch.from_numpy(case["pr_logit"][sel]).to(device))
