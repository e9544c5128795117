"""Time the stand-alone NMS and the uncapped inference tail on the bench shape's candidate set (R = 2000 proposals, K = 20, the
generator of tools/detect_batch_bench.py part (a), score threshold 1e-5) at nms_thresh 0.3 and 0.7:

(a) ops.batched_nms(padded=True) over all candidates (threshold, clip and compaction done beforehand with torch, outside the timing);
(b) ops.detect_all(topk=-1): the whole tail, every survivor, its one 4-byte read included;
(c) ops.detect_all(topk=100) against ops.detect_topk(topk=100), the one-wave kernel with its early exit, which this tool's commit
    leaves as it was.

HIP events around single calls (device time line, host gaps and the tails' read of the count included) and wall clock; the median
of --runs runs (at least 7) after 2 warm-up runs, in rounds that alternate between the four calls.  Writes the figures to
profiles/nms_bench.txt (--out)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, R, K = 375, 500, 2000, 20
SCORE_THRESH, TOPK = 1e-5, 100


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nms_bench.txt"))
    args = ap.parse_args()
    assert args.runs >= 7, "the median of at least 7 runs"
    import torch
    import torch.nn.functional as F

    assert torch.cuda.is_available(), "a timing needs the GPU: nothing is measured without one"
    from __graft_entry__ import load_package

    load_package()
    from drn_wsod_pytorch_amd import ops

    g = torch.Generator().manual_seed(3)
    x0, y0 = torch.rand(R, generator=g) * (W - 60), torch.rand(R, generator=g) * (H - 60)
    p = torch.stack([x0, y0, x0 + 20 + torch.rand(R, generator=g) * (W - x0 - 20) * 0.6,
                     y0 + 20 + torch.rand(R, generator=g) * (H - y0 - 20) * 0.6], 1)
    boxes = (p.repeat(1, K) + torch.randn(R, 4 * K, generator=g) * 4).contiguous().cuda()
    scores = F.softmax(torch.randn(R, K + 1, generator=g) * 3, 1).cuda()
    # the candidates as the tail forms them (fast_rcnn.py:100-127), for (a)
    cb = boxes.view(R, K, 4).clone()
    cb[..., 0::2].clamp_(0, W)
    cb[..., 1::2].clamp_(0, H)
    mask = scores[:, :K] > SCORE_THRESH
    idx = mask.nonzero()
    c_box, c_score, c_cls = cb[mask].contiguous(), scores[:, :K][mask].contiguous(), idx[:, 1].int().contiguous()
    n = c_box.shape[0]

    lines = ["nms_bench: R=%d, K=%d, score_thresh=%g -> %d candidates, %s" % (R, K, SCORE_THRESH, n, torch.cuda.get_device_name(0)),
             "  command: python tools/nms_bench.py --runs %d" % args.runs,
             "  us per call: median [min .. max] of %d runs after 2 warm-up runs, rounds alternating between the calls;"
             " device time line (HIP events) / wall clock" % args.runs]
    for thr in (0.3, 0.7):
        fns = {
            "(a) batched_nms, all candidates, padded": lambda: ops.batched_nms(c_box, c_score, c_cls, thr, padded=True),
            "(b) detect_all(topk=-1)": lambda: ops.detect_all(boxes, scores, (H, W), SCORE_THRESH, thr, topk=-1),
            "(c) detect_all(topk=%d)" % TOPK: lambda: ops.detect_all(boxes, scores, (H, W), SCORE_THRESH, thr, topk=TOPK),
            "(c) detect_topk(topk=%d)" % TOPK: lambda: ops.detect_topk(boxes, scores, (H, W), SCORE_THRESH, thr, TOPK),
        }
        for f in fns.values():
            for _ in range(2):
                f()
        keep, count = fns["(a) batched_nms, all candidates, padded"]()
        every = fns["(b) detect_all(topk=-1)"]()
        first, old = fns["(c) detect_all(topk=%d)" % TOPK](), fns["(c) detect_topk(topk=%d)" % TOPK]()
        kept = int(count)
        same = (kept == len(every[1]) and torch.equal(c_score[keep[:kept]], every[1])
                and all(torch.equal(a, b) for a, b in zip(first, old))
                and all(torch.equal(a[:TOPK], b) for a, b in zip(every, old)))
        ev, wall = {k: [] for k in fns}, {k: [] for k in fns}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.runs):
            for k, f in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e6)
                ev[k].append(e0.elapsed_time(e1) * 1e3)
        lines.append("  nms_thresh %.1f: %d of %d candidates survive (%.3f); (a) = (b) = the first %d of (c), bit for bit: %s"
                     % (thr, kept, n, kept / max(n, 1), TOPK, same))
        for k in fns:
            lines.append("    %-42s %9.1f [%9.1f .. %9.1f] / %9.1f [%9.1f .. %9.1f]"
                         % (k, _median(ev[k]), min(ev[k]), max(ev[k]), _median(wall[k]), min(wall[k]), max(wall[k])))
        a, b = _median(ev["(c) detect_all(topk=%d)" % TOPK]), _median(ev["(c) detect_topk(topk=%d)" % TOPK])
        lines.append("    (c) detect_all / detect_topk at topk=%d = %.2f (device time line)" % (TOPK, a / b))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
