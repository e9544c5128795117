"""Golden of the UNMODIFIED reference `GeneralizedRCNNWithTTAUNION` (build container only).

    cd <repo> && python tests/golden/gen_golden_tta_union.py

ref_harness auto-stubs wsl.modeling.test_time_augmentation_union; after rh.install() the reference's file is loaded by path
under that module name, so the class below is the reference's own.  The case is case_tta's (gen_golden.py): oicr_WSR_50_DC5_1x +
TINY_R50 + C4, R = 48, a 60 x 84 uint8 image, sizes (48, 72), max 96, proposal top-k 40, flip - four augmentations - under
seed 40 instead of case_tta's 38 (see below).
Four runs: mapper in {"avg": the reference's DatasetMapperTTAAVG (proposals follow their images), "def": the default
DatasetMapperTTAUNION (every augmentation gets the ORIGINAL proposals)} x TEST.DETECTIONS_PER_IMAGE in {100, 12}.

Stored (data only): the input, every augmentation's image (once: the four runs produce the same images, asserted) and, per run,
its proposals, each pass's detections as model.inference(..., do_postprocess=False)[0] delivered them, the union arrays of
_get_augmented_boxes, and the merged detections of _merge_detections (= what __call__ returns, asserted).

Margins, "avg" runs: `iou_margin` = the smallest |IoU - NMS_THRESH| over every comparison a greedy NMS makes (a kept box against
each later candidate no earlier kept box has suppressed), over the four per-pass NMS AND the merge; `score_gap` = the smallest
gap between distinct candidate scores of the merge.  The generator asserts iou_margin > 1e-3 and score_gap > 1e-5, far beyond
the 1e-4 / 1e-6 fp32 bounds the GPU test allows this model, so that a low-order-bit difference of the trunk cannot flip a
decision.  Seed 38 misses both (1.7e-4, 5.3e-6); `search N` prints the margins of N seeds from SEED on, and 40 is the first
of 38 .. 77 that meets them (1.5e-3, 1.03e-5).  `pass_score_gap`, the same gap among each pass's own 200 candidates (every
class of every proposal passes the 1e-5 threshold), is recorded but not asserted: 800 softmax scores of a five-class head do not
keep 1e-5 apart (2.2e-7 under seed 38, 2.2e-6 under seed 40).  What the golden comparison rests on instead is recorded and
asserted: `nms_pair_score_gap`, the smallest score gap over the pairs whose order decides a suppression (same class and
IoU > NMS_THRESH), over the per-pass NMS and the merge, is above 1e-5 as well.  `det_rows` are the union rows the merge kept (the
second value of the reference's fast_rcnn_inference_single_image).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

NAME = "tta_union_r50c4_tiny"
SEED, R, H, W, MIN_SIZES, MAX_SIZE, PROP_TOPK = 40, 48, 60, 84, (48, 72), 96, 40
TOPKS = (100, 12)
IOU_MARGIN, SCORE_GAP = 1e-3, 1e-5


def load_reference_union(rh):
    name = "wsl.modeling.test_time_augmentation_union"
    path = os.path.join(rh.REF, "projects", "WSL", "wsl", "modeling", "test_time_augmentation_union.py")
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def margins(boxes, scores, classes, nms_thresh):
    """candidates (clipped boxes, scores, classes, in candidate order) of one NMS -> (smallest |IoU - thresh| over the comparisons
    the greedy pass makes: a kept box against every later candidate that no earlier kept box has suppressed; smallest gap
    between distinct scores; smallest score gap over the pairs whose ORDER decides a suppression: same class and IoU > thresh)"""
    from oracle import wsod_oracle as O

    n = boxes.shape[0]
    if n == 0:
        return np.inf, np.inf, np.inf
    b, s, c = torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(classes).long()
    order = torch.argsort(s, descending=True, stable=True)
    ob = (b + (c.to(b) * (b.max() + 1))[:, None])[order]  # batched_nms' class offsets, in sorted order
    iou = O.pairwise_iou(ob, ob)
    dead = torch.zeros(n, dtype=torch.bool)
    m, kept = np.inf, []
    for i in range(n):
        if dead[i]:
            continue
        kept.append(int(order[i]))
        if i + 1 < n:
            alive = ~dead[i + 1:]
            if alive.any():
                m = min(m, float((iou[i, i + 1:][alive] - nms_thresh).abs().min()))
            dead[i + 1:] |= iou[i, i + 1:] > nms_thresh
    assert kept == O.batched_nms(b, s, c, nms_thresh).tolist()
    u = np.unique(scores)
    gap = np.diff(u).min() if len(u) > 1 else np.inf
    so = s[order]
    over = torch.triu(iou > nms_thresh, diagonal=1)  # (the class offsets keep other classes' boxes apart: IoU 0)
    pair = float((so[:, None] - so[None, :]).abs()[over].min()) if over.any() else np.inf
    return m, float(gap), pair


def pass_candidates(boxes, scores, size, thresh):
    """the candidates of fast_rcnn_inference_single_image (wsl fast_rcnn.py:88-141) of one pass: clip, threshold, row-major order"""
    K = scores.shape[1] - 1
    nreg = boxes.shape[1] // 4
    b = boxes.reshape(-1, nreg, 4).clone()
    b[..., 0::2] = b[..., 0::2].clamp(min=0, max=size[1])
    b[..., 1::2] = b[..., 1::2].clamp(min=0, max=size[0])
    mask = scores[:, :K] > thresh
    inds = mask.nonzero()
    bb = b[inds[:, 0], 0] if nreg == 1 else b[mask]
    return bb.numpy(), scores[:, :K][mask].numpy(), inds[:, 1].numpy()


def run(seed, check=True):
    """the four runs under one seed -> (the golden's dict, {run: (iou margin, merge score gap)})"""
    import gen_golden as GG  # rh.install(), fill_reference, make_inputs, the tiny-model options
    rh = GG.rh
    from detectron2.structures import Boxes, Instances
    from detectron2.utils.events import EventStorage
    from wsl.modeling.test_time_augmentation_avg import DatasetMapperTTAAVG

    U = load_reference_union(rh)
    yaml_rel = "PascalVOC-Detection/oicr_WSR_50_DC5_1x.yaml"
    base = list(GG.TINY_R50 + GG.C4) + ["TEST.AUG.ENABLED", "True", "TEST.AUG.MIN_SIZES", str(tuple(MIN_SIZES)),
                                        "TEST.AUG.MAX_SIZE", str(MAX_SIZE), "TEST.AUG.FLIP", "True",
                                        "DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TEST", str(PROP_TOPK)]
    d = {"seed": np.int64(seed), "min_sizes": np.array(MIN_SIZES), "max_size": np.int64(MAX_SIZE), "topk": np.int64(PROP_TOPK),
         "det_topks": np.array(TOPKS)}
    images, found = None, {}
    for topk in TOPKS:
        o = base + ["TEST.DETECTIONS_PER_IMAGE", str(topk)]
        cfg, model = rh.build_reference_model(yaml_rel, o)
        GG.fill_reference(model, seed)
        model.eval()
        K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
        thr, nms = cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST, cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST
        b = GG.make_inputs(1, R, K, H, W, seed + 17)[0]
        img8 = b["image"].astype(np.uint8)
        d.update({"image_u8": img8, "proposal_boxes": b["proposal_boxes"], "objectness_logits": b["objectness_logits"],
                  "num_classes": np.int64(K), "score_thresh": np.float64(thr), "nms_thresh": np.float64(nms)})
        prop = Instances((H, W))
        prop.proposal_boxes = Boxes(torch.from_numpy(b["proposal_boxes"]))
        prop.objectness_logits = torch.from_numpy(b["objectness_logits"])
        inp = {"image": torch.from_numpy(img8), "proposals": prop, "height": H, "width": W}
        for tag in ("avg", "def"):
            tta = U.GeneralizedRCNNWithTTAUNION(cfg, model, tta_mapper=DatasetMapperTTAAVG(cfg) if tag == "avg" else None)
            assert tag == "avg" or type(tta.tta_mapper) is U.DatasetMapperTTAUNION
            pre = "%s_k%d_" % (tag, topk)
            with torch.no_grad(), EventStorage():
                aug, tfms = tta._get_augmented_inputs(dict(inp))
                assert len(aug) == 4
                d["n_aug"] = np.int64(len(aug))
                ims = [a["image"].numpy().copy() for a in aug]
                if images is None:
                    images = ims
                    for i, im in enumerate(ims):
                        d["aug%d_image" % i] = im
                assert all(np.array_equal(x, y) for x, y in zip(ims, images))
                iou_m, gap_m, pass_gap, pair_gap = np.inf, np.inf, np.inf, np.inf
                for i, a in enumerate(aug):
                    d[pre + "aug%d_boxes" % i] = a["proposals"].proposal_boxes.tensor.numpy().copy()
                    d[pre + "aug%d_obj" % i] = a["proposals"].objectness_logits.numpy().copy()
                    d[pre + "aug%d_size" % i] = np.array(a["proposals"].image_size)
                outputs = tta._batch_inference(aug)
                for i, out in enumerate(outputs):
                    d[pre + "pass%d_boxes" % i] = out.pred_boxes.tensor.numpy().copy()
                    d[pre + "pass%d_scores" % i] = out.scores.numpy().copy()
                    d[pre + "pass%d_classes" % i] = out.pred_classes.numpy().copy()
                    if tag == "avg":
                        _, all_s, all_b = model.inference([aug[i]], None, do_postprocess=False)
                        cb, cs, cc = pass_candidates(all_b[0][0] if all_b[0].dim() == 3 else all_b[0],
                                                     all_s[0][0] if all_s[0].dim() == 3 else all_s[0],
                                                     a_size(aug[i]), thr)
                        mi, mg, mp = margins(cb, cs, cc, nms)
                        iou_m, pass_gap, pair_gap = min(iou_m, mi), min(pass_gap, mg), min(pair_gap, mp)
                all_boxes, all_scores, all_classes = tta._get_augmented_boxes(aug, tfms)
                ub = all_boxes.numpy().copy()
                us = np.array([float(s) for s in all_scores], dtype=np.float32)
                uc = np.array([int(c) for c in all_classes], dtype=np.int64)
                assert np.array_equal(us, np.concatenate([d[pre + "pass%d_scores" % i] for i in range(len(aug))]))
                d[pre + "union_boxes"], d[pre + "union_scores"], d[pre + "union_classes"] = ub, us, uc
                merged = tta._merge_detections(all_boxes, all_scores, all_classes, (H, W))
                # the kept union rows: _merge_detections drops the second value of fast_rcnn_inference_single_image, so the
                # reference's own function (the name the union module imported) is called once more on the same matrix
                s2d = torch.zeros(len(all_boxes), K + 1)
                for idx, (cls, score) in enumerate(zip(all_classes, all_scores)):
                    s2d[idx, cls] = score
                again, rows = U.fast_rcnn_inference_single_image(all_boxes, s2d, (H, W), 1e-8, nms, topk)
                assert torch.equal(again.pred_boxes.tensor, merged.pred_boxes.tensor) and torch.equal(again.scores, merged.scores)
                d[pre + "det_rows"] = rows.numpy().copy()
                final = tta([dict(inp)])[0]["instances"]
            d[pre + "det_boxes"] = merged.pred_boxes.tensor.numpy().copy()
            d[pre + "det_scores"] = merged.scores.numpy().copy()
            d[pre + "det_classes"] = merged.pred_classes.numpy().copy()
            assert np.array_equal(final.pred_boxes.tensor.numpy(), d[pre + "det_boxes"])
            assert np.array_equal(final.scores.numpy(), d[pre + "det_scores"])
            ties = len(us) - len(np.unique(us))
            if tag == "avg":
                clipped = ub.copy()
                clipped[:, 0::2] = np.clip(clipped[:, 0::2], 0, W)
                clipped[:, 1::2] = np.clip(clipped[:, 1::2], 0, H)
                live = us > np.float32(1e-8)
                mi, mg, mp = margins(clipped[live], us[live], uc[live], nms)
                iou_m, gap_m, pair_gap = min(iou_m, mi), mg, min(pair_gap, mp)
                d[pre + "nms_pair_score_gap"] = np.float64(pair_gap)
                d[pre + "iou_margin"], d[pre + "score_gap"] = np.float64(iou_m), np.float64(gap_m)
                d[pre + "pass_score_gap"] = np.float64(pass_gap)
                found[pre] = (iou_m, gap_m, pair_gap)
                assert not check or (iou_m > IOU_MARGIN and gap_m > SCORE_GAP and pair_gap > SCORE_GAP), (pre, iou_m, gap_m, pair_gap)
            print(pre, "union rows", len(us), "kept", len(d[pre + "det_scores"]), "classes",
                  len(np.unique(d[pre + "det_classes"])), "exact score ties", ties,
                  "margins", (iou_m, gap_m, pass_gap, pair_gap) if tag == "avg" else "-")
    return d, found


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "search":  # `search N`: the margins of seeds SEED .. SEED + N - 1, nothing written
        for seed in range(SEED, SEED + int(sys.argv[2])):
            _, found = run(seed, check=False)
            ok = all(i > IOU_MARGIN and g > SCORE_GAP and p > SCORE_GAP for i, g, p in found.values())
            print("seed", seed, "OK" if ok else "no", found)
        return
    d, _ = run(SEED)
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def a_size(aug):
    return tuple(aug["proposals"].image_size)


if __name__ == "__main__":
    main()
