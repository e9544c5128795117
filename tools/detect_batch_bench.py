"""Time the batched, sync-free inference tail and the padded evaluation loop against the per-image path they sit next to.

(a) tail:  R = 2000 proposals, K = 20, softmax scores; ONE ops.detect_topk_batch call (postprocess inside) for N = 1, 4, 8 images
           against N x (ops.detect_topk + detector_postprocess), the per-image path.  HIP events around the calls (device time line,
           host gaps included) and wall clock, medians of alternating rounds.  The launch counts are those of the two chains in
           csrc/detect.hip (the per-image path's torch postprocess launches are not counted).
(b) loop:  IMAGES synthetic 375 x 500 images with 2000 proposals through the R50-C4 model of bench.py, the TTA wrapper with the
           shipped TEST.AUG settings and the device VOC evaluator: evaluation.inference_on_dataset on the padded wrapper against
           the same loop on the unpadded one; wall clock per image, evaluate() included.
(c) plain: the same images through model.inference at batch 4, padded against unpadded, with the device VOC evaluator.
Each part runs in a child process of its own under its own time limit; a part that fails or runs out of time ends the run.
Appends the figures to profiles/detect_batch_bench.txt (--out)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, R, K = 375, 500, 2000, 20
SINGLE_LAUNCHES, BATCH_LAUNCHES = 15, 19  # csrc/detect.hip: drn_detect_topk + drn_detect_gather; drn_detect_topk_batch
LIMITS = {"a": 240, "b": 600, "c": 300}   # seconds per part


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _emit(lines, out_path):
    print("\n".join(lines), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def part_tail(args):
    import torch
    import torch.nn.functional as F

    from __graft_entry__ import load_package

    load_package()
    from drn_wsod_pytorch_amd import ops
    from drn_wsod_pytorch_amd.modeling.rcnn import detector_postprocess
    from drn_wsod_pytorch_amd.structures import Boxes, Instances

    g = torch.Generator().manual_seed(3)
    out_size, thr, nms, topk = (480, 640), 1e-5, 0.3, 100

    def image():
        x0, y0 = torch.rand(R, generator=g) * (W - 60), torch.rand(R, generator=g) * (H - 60)
        p = torch.stack([x0, y0, x0 + 20 + torch.rand(R, generator=g) * (W - x0 - 20) * 0.6,
                         y0 + 20 + torch.rand(R, generator=g) * (H - y0 - 20) * 0.6], 1)
        boxes = (p.repeat(1, K) + torch.randn(R, 4 * K, generator=g) * 4).contiguous()
        return boxes.cuda(), F.softmax(torch.randn(R, K + 1, generator=g) * 3, 1).cuda()

    lines = ["detect_batch_bench (a): the tail alone, R=%d, K=%d, topk=%d, postprocess to %dx%d, %s" %
             (R, K, topk, out_size[0], out_size[1], torch.cuda.get_device_name(0)),
             "  medians of %d alternating rounds x %d calls, us per call of N images: device time line (HIP events) / wall clock" %
             (args.rounds, args.inner)]
    for N in (1, 4, 8):
        imgs = [image() for _ in range(N)]
        boxes, scores = torch.cat([b for b, _ in imgs]), torch.cat([s for _, s in imgs])
        off = [R * i for i in range(N + 1)]

        def batched():
            return ops.detect_topk_batch(boxes, scores, off, [(H, W)] * N, [out_size] * N, score_thresh=thr, nms_thresh=nms, topk=topk)

        def single():
            res = []
            for b, s in imgs:
                ob, os_, oc, _ = ops.detect_topk(b, s, (H, W), thr, nms, topk)
                res.append(detector_postprocess(Instances((H, W), pred_boxes=Boxes(ob), scores=os_, pred_classes=oc), *out_size))
            return res

        fns = dict(batched=batched, single=single)
        for f in fns.values():
            for _ in range(3):
                f()
        got, want = batched(), single()
        cnt = got[4].tolist()
        same = all(cnt[i] == len(want[i]) and torch.equal(got[0][i, :cnt[i]], want[i].pred_boxes.tensor)
                   and torch.equal(got[1][i, :cnt[i]], want[i].scores) for i in range(N))
        ev_us, wall_us = {k: [] for k in fns}, {k: [] for k in fns}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for k, f in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(args.inner):
                    f()
                e1.record()
                torch.cuda.synchronize()
                wall_us[k].append((time.perf_counter() - t0) * 1e6 / args.inner)
                ev_us[k].append(e0.elapsed_time(e1) * 1e3 / args.inner)
        mb, ms = _median(ev_us["batched"]), _median(ev_us["single"])
        lines.append("  N=%d  batched: %2d launches, 0 host reads, %8.1f / %8.1f us   per-image path: %3d launches, %d host reads, "
                     "%8.1f / %8.1f us   batched / per-image = %.3f (device), %.3f (wall)   same bits: %s   detections %s" %
                     (N, BATCH_LAUNCHES, mb, _median(wall_us["batched"]), SINGLE_LAUNCHES * N, 2 * N, ms, _median(wall_us["single"]),
                      mb / ms, _median(wall_us["batched"]) / _median(wall_us["single"]), same, cnt))
    _emit(lines, args.out)


def _model_and_images(n_images, tta):
    import torch

    import bench
    from __graft_entry__ import load_package

    pkg = load_package()
    pkg.set_precision("bf16")
    from drn_wsod_pytorch_amd.modeling import build_model
    from drn_wsod_pytorch_amd.structures import Boxes, Instances

    cfg = bench.build_cfg(pkg, "cuda")
    if tta:
        cfg.merge_from_list(["TEST.AUG.ENABLED", "True", "TEST.AUG.MIN_SIZES", "(480, 576, 672, 768, 864, 960, 1056, 1152)",
                             "TEST.AUG.MAX_SIZE", "4000", "TEST.AUG.FLIP", "True"])
    model = build_model(cfg)
    bench.init_weights(model, seed=0)
    model.eval()
    g = torch.Generator().manual_seed(1)
    distinct = []
    for _ in range(8):
        img = torch.randint(0, 256, (3, H, W), generator=g).to(torch.uint8)
        x0, y0 = torch.rand(R, generator=g) * (W - 60), torch.rand(R, generator=g) * (H - 60)
        p = Instances((H, W))
        p.proposal_boxes = Boxes(torch.stack([x0, y0, x0 + 20 + torch.rand(R, generator=g) * (W - x0 - 20) * 0.6,
                                              y0 + 20 + torch.rand(R, generator=g) * (H - y0 - 20) * 0.6], 1))
        p.objectness_logits = torch.rand(R, generator=g)
        distinct.append((img if tta else img.float(), p))
    images = [{"image": distinct[i % 8][0], "proposals": distinct[i % 8][1], "height": H, "width": W, "image_id": "%06d" % (i + 1)}
              for i in range(n_images)]
    names = ["c%d" % k for k in range(cfg.MODEL.ROI_HEADS.NUM_CLASSES)]
    annos = {x["image_id"]: [(names[(i + j) % len(names)], 0, [20 + 7 * j, 30 + 5 * j, 200 + 9 * j, 180 + 11 * j]) for j in range(3)]
             for i, x in enumerate(images)}
    return cfg, model, images, names, annos


def _time_loops(args, loops, loader, names, annos, n_images, title):
    """loops {name: model}: alternating rounds of evaluation.inference_on_dataset, wall clock per image"""
    import torch

    from drn_wsod_pytorch_amd import evaluation as E

    ms, res = {k: [] for k in loops}, {}
    for k, m in loops.items():  # warm-up: packs, allocator, the evaluator's kernels
        E.inference_on_dataset(m, loader[:3], E.PascalVOCDetectionEvaluator(names, annotations=annos, year=2007, device="cuda"))
    for _ in range(args.loop_rounds):
        for k, m in loops.items():
            ev = E.PascalVOCDetectionEvaluator(names, annotations=annos, year=2007, device="cuda")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = E.inference_on_dataset(m, loader, ev)
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / n_images)
    med = {k: _median(v) for k, v in ms.items()}
    lines = [title, "  medians of %d alternating rounds, ms per image (wall clock, evaluate() included); [min .. max]" % args.loop_rounds]
    for k in loops:
        lines.append("  %-9s %8.3f   [%.3f .. %.3f]" % (k, med[k], min(ms[k]), max(ms[k])))
    lines.append("  padded / unpadded = %.4f   same result dict: %s" % (med["padded"] / med["unpadded"],
                                                                        repr(res["padded"]) == repr(res["unpadded"])))
    _emit(lines, args.out)


def part_loop(args):
    import torch

    cfg, model, images, names, annos = _model_and_images(args.images, True)
    from drn_wsod_pytorch_amd.modeling.tta import GeneralizedRCNNWithTTAAVG

    loops = dict(padded=GeneralizedRCNNWithTTAAVG(cfg, model, padded=True), unpadded=GeneralizedRCNNWithTTAAVG(cfg, model))
    _time_loops(args, loops, [[x] for x in images], names, annos, len(images),
                "detect_batch_bench (b): inference_on_dataset, %d images of %dx%d, R=%d, R50-C4 bf16, TTA (16 passes per image) + "
                "device VOC evaluator, %s" % (len(images), H, W, R, torch.cuda.get_device_name(0)))


def part_plain(args):
    import torch

    cfg, model, images, names, annos = _model_and_images(args.images, False)

    class Plain(torch.nn.Module):
        def __init__(self, padded):
            super().__init__()
            self.model, self.padded = model, padded

        def forward(self, batched_inputs):
            return self.model.inference(batched_inputs, padded=self.padded)

    loader = [images[i: i + 4] for i in range(0, len(images), 4)]
    _time_loops(args, dict(padded=Plain(True), unpadded=Plain(False)), loader, names, annos, len(images),
                "detect_batch_bench (c): inference_on_dataset, %d images of %dx%d in batches of 4, R=%d, R50-C4 bf16, model.inference + "
                "device VOC evaluator, %s" % (len(images), H, W, R, torch.cuda.get_device_name(0)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["a", "b", "c"], default=None, help="run one part in this process (default: all, one child each)")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--loop-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_batch_bench.txt"))
    args = ap.parse_args()
    if args.part is None:
        for part in ("a", "b", "c"):
            cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--rounds", str(args.rounds), "--inner", str(args.inner),
                   "--images", str(args.images), "--loop-rounds", str(args.loop_rounds), "--out", args.out]
            rc = subprocess.run(cmd, timeout=LIMITS[part]).returncode  # a part past its limit raises: nothing more is started
            if rc != 0:
                sys.exit("part (%s) failed with exit status %d: the parts after it are not started" % (part, rc))
        return
    import torch

    assert torch.cuda.is_available(), "a timing needs the GPU: nothing is measured without one"
    {"a": part_tail, "b": part_loop, "c": part_plain}[args.part](args)


if __name__ == "__main__":
    main()
