"""ProposalRecallEvaluator.evaluate() on a synthetic VOC07-trainval-sized input - 5011 images, 2000 proposals each, 1 to 6
boxes per image, the 8 default (area, limit) pairs - split with HIP events into the upload, the ordering passes, the
matching and the read-back.  The proposals go in through the proposal-file helper (host tensors), as a proposal file
would.  Beside it, on the same input and the same machine's host, the numpy restatement of the reference
(tests/proposal_recall_util.py: test infrastructure whose bits equal the reference's, not the code under test), on the
first `--host-images` images and scaled.  The two are timed in alternating rounds; medians and ranges are printed
(profiles/proposal_recall_bench.txt keeps a copy).  There is no pass / fail time.  The unmodified reference function is
timed where the reference is: tests/golden/gen_golden_proposal_recall.py --time (build container, CPU).

    python tools/proposal_recall_bench.py [--images 5011] [--warmup 2] [--repeats 7] [--host-images 200] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_input(images=5011, proposals=2000, seed=0):
    """a case in the flat format of tests/proposal_recall_util.py: 500 x 375 images, 1 .. 6 boxes of 12 .. 360 px, ~ 5 %
    crowd, areas 0.7 w h; 30 % of the proposals are jittered boxes of their image, the rest random; logits a per-image
    permutation (distinct), in shuffled order"""
    rng = np.random.default_rng(seed)
    ng = rng.integers(1, 7, images)
    G = int(ng.sum())
    gt_img = np.repeat(np.arange(1, images + 1), ng)
    wh = rng.uniform(12, 360, (G, 2))
    xy = rng.uniform(0, 1, (G, 2)) * np.maximum(np.array([500.0, 375.0]) - wh, 1)
    gt_box = np.round(np.concatenate([xy, wh], 1), 2)
    n = images * proposals
    pr_img = np.repeat(np.arange(1, images + 1), proposals)
    rwh = rng.uniform(8, 300, (n, 2))
    rxy = rng.uniform(0, 300, (n, 2))
    box = np.concatenate([rxy, rxy + rwh], 1)
    g_off = np.concatenate([[0], np.cumsum(ng)])
    src = g_off[pr_img - 1] + (rng.random(n) * ng[pr_img - 1]).astype(np.int64)
    from_gt = rng.random(n) < 0.3
    gb = gt_box[src]
    jit = rng.normal(0, 0.12, (n, 4)) * np.concatenate([gb[:, 2:], gb[:, 2:]], 1)
    gxyxy = np.concatenate([gb[:, :2], gb[:, :2] + gb[:, 2:]], 1) + jit
    gxyxy[:, 2:] = np.maximum(gxyxy[:, 2:], gxyxy[:, :2] + 1)
    box[from_gt] = gxyxy[from_gt]
    logit = np.argsort(rng.random((images, proposals)), 1).astype(np.float32).reshape(-1) / 16
    return dict(img_ids=np.arange(1, images + 1), gt_img=gt_img, gt_box=gt_box,
                gt_area=np.round(gt_box[:, 2] * gt_box[:, 3] * 0.7, 2), gt_crowd=(rng.random(G) < 0.05).astype(np.uint8),
                pr_img=pr_img, pr_box=box.astype(np.float32), pr_logit=logit)


def proposal_file_of(case):
    """the dict a proposal file in the format of data.load_proposals_into_dataset holds"""
    I = len(case["img_ids"])
    return {"ids": [int(i) for i in case["img_ids"]], "boxes": list(case["pr_box"].reshape(I, -1, 4)),
            "objectness_logits": list(case["pr_logit"].reshape(I, -1)), "bbox_mode": 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5011)
    ap.add_argument("--proposals", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-images", type=int, default=200, help="images the numpy restatement is timed on per round")
    ap.add_argument("--out", default="", help="also write the figures to this file")
    args = ap.parse_args()
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from __graft_entry__ import load_package

    load_package()
    import proposal_recall_util as U
    from drn_wsod_pytorch_amd.evaluation import ProposalRecallEvaluator

    case = make_input(images=args.images, proposals=args.proposals)
    ev = ProposalRecallEvaluator(U.annotations_of(case))
    assert ev.process_proposal_file(proposal_file_of(case)) == args.images
    pairs = [(a, l) for l in (100, 1000) for a in ("all", "small", "medium", "large")]
    hn = min(args.host_images, args.images)
    host_images = U.images_of(case, case["img_ids"][:hn])
    times, host = {}, []
    for r in range(args.warmup + args.repeats):  # alternating: one device run, one host run
        marks = []

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

        ev._mark = mark
        res = ev.evaluate()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for area, limit in pairs:
            for pb, pl, gb, ga in host_images:
                U.match_image(pb, pl, gb, ga, area, limit)
        t1 = time.perf_counter()
        if r >= args.warmup:
            for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
                times.setdefault(name, []).append(e0.elapsed_time(e1))
            times.setdefault("total", []).append(marks[0][1].elapsed_time(marks[-1][1]))
            host.append((t1 - t0) * 1e3 * args.images / hn)
    want = U.evaluate_numpy({k: (v[: hn] if k == "img_ids" else v) for k, v in case.items()}, "all", 100)
    sub = ProposalRecallEvaluator(U.annotations_of(case), limits=(100,), areas=("all",))
    sub.process_proposal_file({k: v[:hn] for k, v in proposal_file_of(case).items() if k != "bbox_mode"})
    sub.evaluate()
    same = np.array_equal(sub.results[("all", 100)]["gt_overlaps"].numpy(), want["gt_overlaps"])
    lines = ["ProposalRecallEvaluator.evaluate(), stages by HIP events, ms; median [min .. max] of %d runs after %d warm-up runs,"
             % (args.repeats, args.warmup), " in rounds alternating with the host figure below",
             "input: %d images x %d proposals (host tensors, as from a proposal file), %d boxes, 8 (area, limit) pairs"
             % (args.images, args.proposals, len(case["gt_img"])),
             "       (tools/proposal_recall_bench.py make_input, seed 0)",
             "machine: %s" % torch.cuda.get_device_name(0)]
    for name, v in times.items():
        lines.append("  %-26s %10.3f  [%10.3f .. %10.3f]" % (name, statistics.median(v), min(v), max(v)))
    b = res["box_proposals"]
    lines.append("  AR@100 %.4f  ARs@100 %.4f  AR@1000 %.4f  ARl@1000 %.4f" % (b["AR@100"], b["ARs@100"], b["AR@1000"], b["ARl@1000"]))
    lines += ["numpy restatement of the reference (tests/proposal_recall_util.py match_image), this machine's host, one thread:",
              "  the 8 pairs on the first %d images, scaled to %d images" % (hn, args.images),
              "  %-26s %10.1f  [%10.1f .. %10.1f]" % ("matching", statistics.median(host), min(host), max(host)),
              "  its gt_overlaps (all, 100) on those images equal the device's bit for bit: %s" % same]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
