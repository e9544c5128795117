"""COCOEvaluator.evaluate() on a synthetic minival-sized input - 5000 images, 100 detections each, 80 classes, about 36 k
ground-truth boxes - split into its device stages with HIP events: the ordering passes, the matching, the second
ordering, the accumulation, and the read-back of the three result arrays.  After `--warmup` untimed runs, `--repeats`
timed ones; the median and the range of each stage are printed (profiles/coco_eval_bench.txt keeps a copy).  There is no pass / fail time:
the figure to hold it against is the reference's C++ on the same input (tests/golden/gen_golden_coco.py --time, build
container, CPU), which is recorded next to it by hand.

    python tools/coco_eval_bench.py [--images 5000] [--warmup 3] [--repeats 10] [--out FILE]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_input(images=5000, dets=100, classes=80, gt_per_image=7.2, seed=0):
    """a case in the flat format of tests/coco_eval_util.py: 640 x 480 images, GT boxes of 8 .. 300 px, ~ 8 % crowd; 60 %
    of the detections are jittered GT boxes of their image (class kept), the rest random; scores uniform float32"""
    rng = np.random.default_rng(seed)
    ng = rng.poisson(gt_per_image, images)
    G = int(ng.sum())
    gt_img = np.repeat(np.arange(1, images + 1), ng)
    wh = rng.uniform(8, 300, (G, 2))
    xy = rng.uniform(0, 1, (G, 2)) * (np.array([640.0, 480.0]) - np.minimum(wh, [600, 440]))
    gt_box = np.round(np.concatenate([xy, wh], 1), 2)
    gt_cat = rng.integers(1, classes + 1, G)
    n = images * dets
    dt_img = np.repeat(np.arange(1, images + 1), dets)
    rwh = rng.uniform(8, 300, (n, 2))
    rxy = rng.uniform(0, 400, (n, 2))
    box = np.concatenate([rxy, rxy + rwh], 1)
    cls = rng.integers(0, classes, n)
    g_off = np.concatenate([[0], np.cumsum(ng)])
    has = ng[dt_img - 1] > 0
    src = g_off[dt_img - 1] + (rng.random(n) * np.maximum(ng[dt_img - 1], 1)).astype(np.int64)
    src = np.minimum(src, max(G - 1, 0))
    from_gt = has & (rng.random(n) < 0.6)
    gb = gt_box[src]
    jit = rng.normal(0, 0.08, (n, 4)) * np.concatenate([gb[:, 2:], gb[:, 2:]], 1)
    gxyxy = np.concatenate([gb[:, :2], gb[:, :2] + gb[:, 2:]], 1) + jit
    gxyxy[:, 2:] = np.maximum(gxyxy[:, 2:], gxyxy[:, :2] + 1)
    box[from_gt] = gxyxy[from_gt]
    cls[from_gt] = gt_cat[src[from_gt]] - 1
    return dict(img_ids=np.arange(1, images + 1), cat_ids=np.arange(1, classes + 1), gt_img=gt_img, gt_cat=gt_cat,
                gt_box=gt_box, gt_area=np.round(gt_box[:, 2] * gt_box[:, 3] * 0.7, 2),
                gt_crowd=(rng.random(G) < 0.08).astype(np.uint8), dt_img=dt_img, dt_cls=cls.astype(np.int64),
                dt_box=box.astype(np.float32), dt_score=rng.random(n).astype(np.float32))


def annotations_of(case):
    """the COCO-format dict of a case's ground truth"""
    return {"images": [{"id": int(i)} for i in case["img_ids"]],
            "categories": [{"id": int(c), "name": "c%d" % int(c)} for c in case["cat_ids"]],
            "annotations": [{"id": j + 1, "image_id": int(case["gt_img"][j]), "category_id": int(case["gt_cat"][j]),
                             "bbox": [float(v) for v in case["gt_box"][j]], "area": float(case["gt_area"][j]),
                             "iscrowd": int(case["gt_crowd"][j])} for j in range(len(case["gt_img"]))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the figures to this file")
    args = ap.parse_args()
    import torch

    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package

    load_package()
    from drn_wsod_pytorch_amd.evaluation import COCOEvaluator
    from drn_wsod_pytorch_amd.structures import Boxes, Instances

    case = make_input(images=args.images)
    ev = COCOEvaluator(annotations_of(case))
    dev = torch.device("cuda")
    box, score, cls = (torch.from_numpy(case[k]).to(dev) for k in ("dt_box", "dt_score", "dt_cls"))
    per = len(case["dt_img"]) // args.images
    for i in range(args.images):
        s = slice(i * per, (i + 1) * per)
        ev.process([{"image_id": int(case["img_ids"][i])}],
                   [{"instances": Instances((480, 640), pred_boxes=Boxes(box[s]), scores=score[s], pred_classes=cls[s])}])
    times = {}
    for r in range(args.warmup + args.repeats):
        marks = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

        ev._mark = mark
        res = ev.evaluate()
        torch.cuda.synchronize()
        if r >= args.warmup:
            for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
                times.setdefault(name, []).append(e0.elapsed_time(e1))
            times.setdefault("total", []).append(marks[0][1].elapsed_time(marks[-1][1]))
    lines = ["COCOEvaluator.evaluate(), device stages (HIP events, ms; median [min .. max] of %d runs after %d warm-up runs)"
             % (args.repeats, args.warmup),
             "input: %d images, %d detections, %d classes, %d ground-truth boxes (tools/coco_eval_bench.py make_input, seed 0)"
             % (args.images, len(case["dt_img"]), len(case["cat_ids"]), len(case["gt_img"])),
             "machine: %s" % torch.cuda.get_device_name(0)]
    for name, v in times.items():
        lines.append("  %-26s %9.3f  [%9.3f .. %9.3f]" % (name, statistics.median(v), min(v), max(v)))
    lines.append("AP %.4f  AP50 %.4f  AP75 %.4f" % (res["bbox"]["AP"], res["bbox"]["AP50"], res["bbox"]["AP75"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
