"""PascalVOCDetectionEvaluator on a synthetic VOC07-test-sized input - 4952 images, 100 detections each, 20 classes - host
path against device path (device="cuda") on the same input and the same machine:

  * device evaluate(), split into its stages with HIP events: after `--warmup` untimed runs, `--repeats` timed ones, the
    median and the range of each stage;
  * process() over the whole set, wall clock, both paths (the host path copies every image's predictions to the host
    and formats one text line per detection; the device path keeps the tensors);
  * the host evaluate() once, wall clock (`--no-host` leaves it out: it takes minutes).

There is no pass / fail time.  profiles/voc_eval_bench.txt keeps a copy of the output.

    python tools/voc_eval_bench.py [--images 4952] [--warmup 3] [--repeats 10] [--no-host] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_input(images=4952, dets=100, classes=20, gt_per_image=2.5, seed=0):
    """-> (class names, annotations {image_id: [(name, difficult, [xmin, ymin, xmax, ymax])]}, per image (boxes [dets, 4]
    f32, scores [dets] f32, classes [dets] i64)).  500 x 375 images, integer GT boxes of 20 .. 300 px, ~ 15 % difficult;
    60 % of the detections are jittered GT boxes of their image (class kept), the rest random; scores float32, half of
    them below 0.05 as after a 1e-5 score threshold"""
    rng = np.random.default_rng(seed)
    names = ["class%02d" % k for k in range(classes)]
    annos, preds = {}, []
    for i in range(images):
        ng = int(rng.poisson(gt_per_image))
        wh = rng.integers(20, 300, (ng, 2))
        xy = 1 + (rng.random((ng, 2)) * np.maximum(np.array([500, 375]) - wh, 1)).astype(np.int64)
        gt = np.concatenate([xy, xy + wh], 1)
        gcls = rng.integers(0, classes, ng)
        annos["%06d" % (i + 1)] = [(names[int(gcls[j])], int(rng.random() < 0.15), [int(v) for v in gt[j]]) for j in range(ng)]
        rxy = rng.uniform(0, 300, (dets, 2))
        box = np.concatenate([rxy, rxy + rng.uniform(20, 300, (dets, 2))], 1)
        cls = rng.integers(0, classes, dets)
        if ng:
            src = rng.integers(0, ng, dets)
            from_gt = rng.random(dets) < 0.6
            jit = rng.normal(0, 0.08, (dets, 4)) * np.tile(wh[src], 2)
            gb = gt[src] - [1, 1, 0, 0] + jit
            box[from_gt], cls[from_gt] = gb[from_gt], gcls[src[from_gt]]
        score = np.where(rng.random(dets) < 0.5, rng.random(dets) * 0.05, rng.random(dets))
        preds.append((box.astype(np.float32), score.astype(np.float32), cls.astype(np.int64)))
    return names, annos, preds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4952)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the host evaluate()")
    ap.add_argument("--out", default="", help="also write the figures to this file")
    args = ap.parse_args()
    import torch

    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package

    load_package()
    from drn_wsod_pytorch_amd.evaluation import PascalVOCDetectionEvaluator
    from drn_wsod_pytorch_amd.structures import Boxes, Instances

    names, annos, preds = make_input(images=args.images)
    ids = list(annos)
    dev = torch.device("cuda")
    staged = []
    for iid, (box, score, cls) in zip(ids, preds):
        inst = Instances((375, 500), pred_boxes=Boxes(torch.from_numpy(box).to(dev)), scores=torch.from_numpy(score).to(dev),
                         pred_classes=torch.from_numpy(cls).to(dev))
        staged.append(([{"image_id": iid}], [{"instances": inst}]))
    torch.cuda.synchronize()

    def feed(ev):
        t0 = time.perf_counter()
        for inputs, outputs in staged:
            ev.process(inputs, outputs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    ev = PascalVOCDetectionEvaluator(names, annotations=annos, year=2007, device="cuda")
    feed(ev)  # warm-up
    ev.reset()
    t_proc_dev = feed(ev)
    times, wall = {}, []
    for r in range(args.warmup + args.repeats):
        marks = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

        ev._mark = mark
        t0 = time.perf_counter()
        res = ev.evaluate()
        torch.cuda.synchronize()
        if r >= args.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
                times.setdefault(name, []).append(e0.elapsed_time(e1))
            times.setdefault("total (start .. read-back)", []).append(marks[0][1].elapsed_time(marks[-1][1]))
    host = PascalVOCDetectionEvaluator(names, annotations=annos, year=2007)
    t_proc_host = feed(host)
    n = sum(len(p[1]) for p in preds)
    lines = ["PascalVOCDetectionEvaluator, host path (device=None) against device path (device=\"cuda\"), year 2007",
             "command: python tools/voc_eval_bench.py --images %d --warmup %d --repeats %d%s"
             % (args.images, args.warmup, args.repeats, " --no-host" if args.no_host else ""),
             "input: %d images, %d detections, %d classes, %d ground-truth boxes (tools/voc_eval_bench.py make_input, seed 0)"
             % (args.images, n, len(names), sum(len(v) for v in annos.values())),
             "machine: %s; host figures are wall clock on this machine's CPU" % torch.cuda.get_device_name(0),
             "device evaluate(), stages by HIP events (ms; median [min .. max] of %d runs after %d warm-up runs)"
             % (args.repeats, args.warmup)]
    for name, v in times.items():
        lines.append("  %-28s %9.3f  [%9.3f .. %9.3f]" % (name, statistics.median(v), min(v), max(v)))
    lines.append("  %-28s %9.3f  [%9.3f .. %9.3f]" % ("wall clock, whole call", statistics.median(wall), min(wall), max(wall)))
    lines.append("process() over the whole set (s, wall clock):   host %9.3f    device %9.3f" % (t_proc_host, t_proc_dev))
    if args.no_host:
        lines.append("evaluate() (s, wall clock):                     host   (skipped)    device %9.3f" % (statistics.median(wall) / 1e3))
    else:
        t0 = time.perf_counter()
        hres = host.evaluate()
        t_eval_host = time.perf_counter() - t0
        lines.append("evaluate() (s, wall clock):                     host %9.3f    device %9.3f"
                     % (t_eval_host, statistics.median(wall) / 1e3))
        lines.append("host    AP %.6f  AP50 %.6f  CL50 %.6f  (np.argsort tie order)"
                     % (hres["bbox"]["AP"], hres["bbox"]["AP50"], hres["bbox CorLoc"]["CL50"]))
    lines.append("device  AP %.6f  AP50 %.6f  CL50 %.6f  (ties in processing order)"
                 % (res["bbox"]["AP"], res["bbox"]["AP50"], res["bbox CorLoc"]["CL50"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
