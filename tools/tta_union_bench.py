"""Time GeneralizedRCNNWithTTAUNION's tail and the whole wrapper on one GPU.

(a) tail:    R = 2000 proposals, K = 20, 16 augmentations (8 sizes x flip), top-k 100.  The two launch chains the wrapper runs -
             ONE ops.detect_topk_batch over the 16 passes as "images" and ONE ops.detect_union_batch - against the same result
             composed from entries that existed before the union entry: 16 x ops.detect_topk (one count read each), the
             back-transform and the scatter into the [n, K+1] score matrix in torch, and one more ops.detect_topk.  HIP events
             around the calls (device time line, host gaps included) and wall clock, medians of alternating rounds.  The launch
             counts are those of csrc/detect.hip (the composed path's torch launches are not counted).
(b) wrapper: synthetic 375 x 500 images with 2000 proposals through the R50-C4 model of bench.py with the shipped TEST.AUG
             settings (16 passes per image): GeneralizedRCNNWithTTAUNION(padded=True) against GeneralizedRCNNWithTTAAVG(padded=True),
             both on DatasetMapperTTAAVG(device=...) - the same augmented inputs; wall clock per image.
Each part runs in a child process of its own under its own time limit; a part that fails or runs out of time ends the run.
Appends the figures to profiles/tta_union_bench.txt (--out)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

H, W, R, K, TOPK = 375, 500, 2000, 20, 100
SIZES = (480, 576, 672, 768, 864, 960, 1056, 1152)
SINGLE_LAUNCHES, BATCH_LAUNCHES, UNION_LAUNCHES = 15, 19, 17  # csrc/detect.hip: drn_detect_topk + _gather; _topk_batch; _union_batch
LIMITS = {"a": 240, "b": 420}  # seconds per part


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
    import numpy as np
    import torch
    import torch.nn.functional as F

    from __graft_entry__ import load_package

    load_package()
    from drn_wsod_pytorch_amd import ops
    from drn_wsod_pytorch_amd.modeling.roi_heads import padded_detections
    from drn_wsod_pytorch_amd.modeling.tta import resize_shortest_edge_shape

    g = torch.Generator().manual_seed(3)
    thr, nms = 1e-5, 0.3
    passes, tfms, sizes = [], [], []
    for size in SIZES:
        nh, nw = resize_shortest_edge_shape(H, W, size, 4000)
        for fl in (False, True):
            x0, y0 = torch.rand(R, generator=g) * (nw - 60), torch.rand(R, generator=g) * (nh - 60)
            p = torch.stack([x0, y0, x0 + 20 + torch.rand(R, generator=g) * (nw - x0 - 20) * 0.6,
                             y0 + 20 + torch.rand(R, generator=g) * (nh - y0 - 20) * 0.6], 1)
            boxes = (p.repeat(1, K) + torch.randn(R, 4 * K, generator=g) * 4).contiguous()
            passes.append((boxes.cuda(), F.softmax(torch.randn(R, K + 1, generator=g) * 3, 1).cuda()))
            tfms.append((W * 1.0 / nw, H * 1.0 / nh, float(nw) if fl else -1.0))
            sizes.append((nh, nw))
    A = len(passes)
    all_b, all_s = torch.cat([b for b, _ in passes]), torch.cat([s for _, s in passes])

    def two_chains():
        det = padded_detections(all_b, all_s, [R] * A, sizes, None, thr, nms, TOPK)
        return ops.detect_union_batch(det.boxes, det.scores, det.classes, det.count, [0, A], tfms, [(H, W)], num_classes=K,
                                      nms_thresh=nms, topk=TOPK)

    def composed():
        ub, us, uc = [], [], []
        for (b, s), (sx, sy, fw), size in zip(passes, tfms, sizes):
            ob, os_, oc, _ = ops.detect_topk(b, s, size, thr, nms, TOPK)  # (reads its count)
            x0, y0, x1, y1 = ob.unbind(1)
            if fw >= 0:
                x0, x1 = fw - x0, fw - x1
            sx, sy = float(np.float32(sx)), float(np.float32(sy))
            x0, x1, y0, y1 = x0 * sx, x1 * sx, y0 * sy, y1 * sy
            ub.append(torch.stack([torch.minimum(x0, x1), torch.minimum(y0, y1), torch.maximum(x0, x1), torch.maximum(y0, y1)], 1))
            us.append(os_)
            uc.append(oc)
        ub, us, uc = torch.cat(ub), torch.cat(us), torch.cat(uc)
        s2 = torch.zeros((ub.shape[0], K + 1), device=ub.device)
        s2[torch.arange(ub.shape[0], device=ub.device), uc] = us
        return ops.detect_topk(ub.contiguous(), s2, (H, W), 1e-8, nms, TOPK)

    fns = dict(two_chains=two_chains, composed=composed)
    for f in fns.values():
        for _ in range(3):
            f()
    got, want = two_chains(), composed()
    n = int(got[4][0])
    same = (n == want[1].shape[0] and torch.equal(got[0][0, :n], want[0]) and torch.equal(got[1][0, :n], want[1])
            and torch.equal(got[2][0, :n].long(), want[2]))
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
    mt, mc = _median(ev_us["two_chains"]), _median(ev_us["composed"])
    _emit(["tta_union_bench (a): the union tail alone, R=%d, K=%d, %d augmentations, topk=%d, %s" %
           (R, K, A, TOPK, torch.cuda.get_device_name(0)),
           "  medians of %d alternating rounds x %d calls, us per image: device time line (HIP events) / wall clock" %
           (args.rounds, args.inner),
           "  two chains: %d + %d launches, 0 host reads, %8.1f / %8.1f us" %
           (BATCH_LAUNCHES, UNION_LAUNCHES, mt, _median(wall_us["two_chains"])),
           "  composed:   %d x %d + %d launches (+ torch's), %d host reads, %8.1f / %8.1f us" %
           (A, SINGLE_LAUNCHES, SINGLE_LAUNCHES, A + 1, mc, _median(wall_us["composed"])),
           "  two chains / composed = %.3f (device), %.3f (wall)   same bits: %s   merged detections: %d" %
           (mt / mc, _median(wall_us["two_chains"]) / _median(wall_us["composed"]), same, n)], args.out)


def part_wrapper(args):
    import torch

    import detect_batch_bench as DB

    cfg, model, images, _, _ = DB._model_and_images(args.images, True)
    cfg.merge_from_list(["TEST.DETECTIONS_PER_IMAGE", str(TOPK)])
    from drn_wsod_pytorch_amd.modeling.tta import DatasetMapperTTAAVG, GeneralizedRCNNWithTTAAVG, GeneralizedRCNNWithTTAUNION

    mapper = DatasetMapperTTAAVG(cfg, device=model.device)
    models = dict(union=GeneralizedRCNNWithTTAUNION(cfg, model, tta_mapper=mapper, padded=True),
                  avg=GeneralizedRCNNWithTTAAVG(cfg, model, tta_mapper=mapper, padded=True))
    ms, cnt = {k: [] for k in models}, {}
    with torch.no_grad():
        for m in models.values():
            for x in images[:3]:
                m([x])
        for _ in range(args.loop_rounds):
            for k, m in models.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for x in images:
                    out = m([x])
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / len(images))
                cnt[k] = int(out.count[0])
    med = {k: _median(v) for k, v in ms.items()}
    lines = ["tta_union_bench (b): the whole wrapper, %d images of %dx%d, R=%d, R50-C4 bf16, 16 passes per image, padded=True, %s" %
             (len(images), H, W, R, torch.cuda.get_device_name(0)),
             "  medians of %d alternating rounds, ms per image (wall clock); [min .. max]; detections of the last image" % args.loop_rounds]
    for k in models:
        lines.append("  %-6s %8.3f   [%.3f .. %.3f]   %d" % (k, med[k], min(ms[k]), max(ms[k]), cnt[k]))
    lines.append("  union / avg = %.4f" % (med["union"] / med["avg"]))
    _emit(lines, args.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=["a", "b"], default=None, help="run one part in this process (default: both, one child each)")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--loop-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_union_bench.txt"))
    args = ap.parse_args()
    if args.part is None:
        for part in ("a", "b"):
            cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--rounds", str(args.rounds), "--inner", str(args.inner),
                   "--images", str(args.images), "--loop-rounds", str(args.loop_rounds), "--out", args.out]
            rc = subprocess.run(cmd, timeout=LIMITS[part]).returncode  # a part past its limit raises: nothing more is started
            if rc != 0:
                sys.exit("part (%s) failed with exit status %d: the parts after it are not started" % (part, rc))
        return
    import torch

    assert torch.cuda.is_available(), "a timing needs the GPU: nothing is measured without one"
    {"a": part_tail, "b": part_wrapper}[args.part](args)


if __name__ == "__main__":
    main()
