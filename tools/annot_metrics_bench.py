"""The annotated-box block of the per-step metrics (ROIHeads.enable_metrics(annotated=True)): what it costs on the graphed
bench-shape step - BASELINE configs[1] (R50-C4, 224 x 224, R = 2000, bf16, one GPU, synthetic inputs built as bench.py builds them),
GraphedTrainStep as bench.py runs it.  The protocol of tools/metrics_bench.py: ONE process, alternating blocks of `--steps` steps,
`--repeats` rounds each after a warm-up, the ring drained every `--drain` steps; every form is a model and a step object of its own,
so the off form is built TWICE - first and last, the on form between them - and off2 - off is what one object differs from another.
Both forms record metrics; "off" is enable_metrics() as it was (the launch sequence tests/test_annot_metrics_gpu.py holds the
option's off state to), "on" adds drn_label_proposals and drn_mil_metrics to the captured heads graph, swaps the record launch for
its variant with the block, and lengthens the label upload by n_img * (5 * max_gt + 1) words.

    python tools/annot_metrics_bench.py [--repeats 3] [--steps 200] [--drain 20] [--out profiles/annot_metrics_bench.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/annot_metrics_bench.py --trace   (a short run of the on form alone: the
                                                                                                new kernels' own times are in the stats)"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

NAMES = ("roi_head/num_fg_samples", "roi_head/num_bg_samples", "roi_head/num_ig_samples", "fast_rcnn/cls_accuracy",
         "fast_rcnn/fg_cls_accuracy", "fast_rcnn/false_negative")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proposals", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3, help="alternating timing rounds per form")
    ap.add_argument("--steps", type=int, default=200, help="steps per timing block")
    ap.add_argument("--drain", type=int, default=20, help="steps between two drains of the ring")
    ap.add_argument("--trunk-group", type=int, default=4)
    ap.add_argument("--max-gt", type=int, default=64)
    ap.add_argument("--classes", type=int, nargs="*", default=[20], help="head widths K to measure")
    ap.add_argument("--trace", action="store_true", help="the on form only, 60 steps, nothing written (for rocprofv3)")
    ap.add_argument("--note", action="append", default=[], help="a line copied into the profile")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "annot_metrics_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU (no fallback)"
    device = "cuda:0"
    torch.cuda.set_device(0)
    torch.manual_seed(1234)
    pkg = load_package()
    pkg._cabi.lib()
    pkg.set_precision("bf16")
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer
    from drn_wsod_pytorch_amd.modeling import build_model

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    R, G = args.proposals, args.trunk_group
    say("annot_metrics_bench: R50-C4 224x224 R=%d bf16, max_gt %d, device %s" % (R, args.max_gt, torch.cuda.get_device_name(0)))
    for K in args.classes:
        cfg = bench.build_cfg(pkg, device)
        cfg.merge_from_list(["MODEL.ROI_HEADS.NUM_CLASSES", str(K)])
        batches = bench.synthetic_batches(8, R, K, device, 0, pkg, 1)
        window = lambda j: [batches[(j + q) % len(batches)] for q in range(2 * G)]
        runs = {}
        for mode in (("on",) if args.trace else ("off", "on", "off2")):
            model = build_model(cfg)
            bench.init_weights(model, seed=0)
            model.train()
            opt = build_optimizer(cfg, model)
            opt.enable_pipelined(None)
            if mode == "on":
                ring = model.roi_heads.enable_metrics(slots=256, annotated=True, max_gt=args.max_gt)
            else:
                ring = model.roi_heads.enable_metrics(slots=256)
            stp = GraphedTrainStep(model, opt, batches[0], split_tail=True, lookahead=2, trunk_pairs=G, eager_fc6=True)
            runs[mode] = dict(stp=stp, pos=0, ms=[], ring=ring, got=0, lost=0, last=None)

        def run(r, n):
            for _ in range(n):
                last = r["stp"].step(*window(r["pos"]))
                r["pos"] += 1
                if r["pos"] % args.drain == 0:
                    recs, lost = r["ring"].collect(wait=True)  # the previous drain: `--drain` steps old
                    r["got"], r["lost"] = r["got"] + len(recs), r["lost"] + lost
                    r["last"] = recs[-1] if recs else r["last"]
                    r["ring"].drain()
            return last

        for r in runs.values():
            run(r, 60 if args.trace else 40)
        torch.cuda.synchronize()
        for _ in range(0 if args.trace else args.repeats):
            for mode, r in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last = run(r, args.steps)
                torch.cuda.synchronize()
                r["ms"].append(1e3 * (time.perf_counter() - t0) / args.steps)
                bench.assert_sane_losses({k: v.detach() for k, v in last.items()}, mode)
        torch.cuda.synchronize()
        for r in runs.values():
            r["ring"].drain()
            recs, lost = r["ring"].collect(wait=True)
            r["got"], r["lost"] = r["got"] + len(recs), r["lost"] + lost
            r["last"] = recs[-1] if recs else r["last"]
        on = runs["on"]
        assert all(k in on["last"][1] for k in NAMES[:4]), sorted(on["last"][1])
        if not args.trace:
            say()
            say("K = %d: GraphedTrainStep on enable_pipelined(), %d alternating rounds x %d steps, drain every %d steps, ms per step"
                % (K, args.repeats, args.steps, args.drain))
            for mode, r in runs.items():
                say("  annotated %-4s blocks %s   median %.4f" % (mode, " ".join("%.4f" % x for x in r["ms"]), statistics.median(r["ms"])))
            off, off2 = runs["off"]["ms"], runs["off2"]["ms"]
            d = statistics.median(on["ms"]) - statistics.median(off)
            d2 = statistics.median(on["ms"]) - statistics.median(off2)
            say("  on - off = %+.1f us per step (%+.2f %%), on - off2 = %+.1f us; off2 - off (two objects of the same form) = %+.1f us; "
                "the off blocks' own spread: %.1f us"
                % (1e3 * d, 100.0 * d / statistics.median(off), 1e3 * d2, 1e3 * (statistics.median(off2) - statistics.median(off)),
                   1e3 * (max(off) - min(off))))
            say("  records decoded %d of %d steps, lost %d; the last one: iteration %d, %s"
                % (on["got"], on["pos"], on["lost"], on["last"][0],
                   ", ".join("%s %.4g" % (k, on["last"][1][k]) for k in NAMES if k in on["last"][1])))
            assert not any(k in runs["off"]["last"][1] for k in NAMES)
            for r in runs.values():
                assert r["lost"] == 0 and r["got"] == r["pos"], (r["got"], r["lost"], r["pos"])
        for r in runs.values():
            r["stp"].release()
        del runs
    if args.trace:
        return
    if args.note:
        say()
        for n in args.note:
            say(n)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
