"""Time the PCL device path (drn_pcl_adjacency + drn_pcl_refine) on SURVEY 8(d)-shaped synthetic proposals and report
the sizes that drive it (top-cluster members per labelled class, centres).

--images N: N such images (different boxes, scores and labels each) as ONE batch through drn_pcl_adjacency_batch +
drn_pcl_refine_batch against the N sequential single-image triples, in one process: alternating rounds, HIP events, medians.
Appends the figures to profiles/pcl_batch_bench.txt (--out).
--images N --step: the whole PCL training step (bench.py's R50-C4 model and synthetic batches, bf16, GraphedTrainStep in its
default form) with N images per step on the opted-in head against the 1-image step, same process, alternating rounds."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from drn_wsod_pytorch_amd import ops  # noqa: E402


def _inputs(R, K, NB, G, mode, seed):
    g = torch.Generator().manual_seed(seed)
    W = H = 224.0
    if mode == "random":
        x0 = torch.rand(R, generator=g) * (W - 40)
        y0 = torch.rand(R, generator=g) * (H - 40)
        bw = 20 + torch.rand(R, generator=g) * (W - x0 - 20)
        bh = 20 + torch.rand(R, generator=g) * (H - y0 - 20)
    else:  # clustered around 12 objects
        c = torch.randint(0, 12, (R,), generator=g)
        cx0, cy0 = torch.rand(12, generator=g) * 120, torch.rand(12, generator=g) * 120
        cw, ch = 40 + torch.rand(12, generator=g) * 60, 40 + torch.rand(12, generator=g) * 60
        j = torch.randn(R, 4, generator=g) * 5
        x0, y0 = (cx0[c] + j[:, 0]).clamp(0, W - 25), (cy0[c] + j[:, 1]).clamp(0, H - 25)
        bw, bh = (cw[c] + j[:, 2]).clamp(min=20), (ch[c] + j[:, 3]).clamp(min=20)
    boxes = torch.stack([x0, y0, (x0 + bw).clamp(max=W), (y0 + bh).clamp(max=H)], 1).contiguous().cuda()
    a = torch.randn(R, K, generator=g) * 2
    b = torch.randn(R, K, generator=g) * 3
    ws = (torch.softmax(a, 1) * torch.softmax(b, 0)).contiguous().cuda()
    logits = (torch.randn(R, NB * (K + 1), generator=g) * 2).cuda()
    onehot = torch.zeros(K)
    onehot[torch.randperm(K, generator=g)[:G]] = 1
    onehot = onehot.cuda()
    return boxes, ws, logits, onehot


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def bench_images(N, R, K, NB, G, mode, rounds, out_path):
    """the batched triple against N sequential single-image triples; one round = `inner` calls of each, A B A B ..."""
    imgs = [_inputs(R, K, NB, G, mode, 7 + i) for i in range(N)]
    cols = [b_ * (K + 1) for b_ in range(NB)]
    boxes = torch.cat([i[0] for i in imgs]).contiguous()
    ws = torch.cat([i[1] for i in imgs]).contiguous()
    logits = torch.cat([i[2] for i in imgs]).contiguous()
    onehot = torch.stack([i[3] for i in imgs]).contiguous()
    off = torch.tensor([R * i for i in range(N + 1)], dtype=torch.int32).cuda()
    dl = torch.zeros_like(logits)
    dls = [torch.zeros_like(i[2]) for i in imgs]

    def batched():
        adj = ops.pcl_adjacency_batch(boxes, off, N, R, 0.4)
        return ops.pcl_refine_batch(logits, cols, K, ws, boxes, adj, onehot, off, N, R, dl, rows=[R] * N)

    def sequential(n=N):
        out = None
        for (b, w, l, o), d in list(zip(imgs, dls))[:n]:
            out = ops.pcl_refine(l, cols, K, w, b, ops.pcl_adjacency(b, 0.4), o, d)
        return out

    fns = dict(batched=batched, sequential=sequential, one_image=lambda: sequential(1))
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    per, _, _ = batched()
    seq = [ops.pcl_refine(l, cols, K, w, b, ops.pcl_adjacency(b, 0.4), o, d) for (b, w, l, o), d in zip(imgs, dls)]
    torch.cuda.synchronize()
    same = all(torch.equal(per[i][b_]["labels"], seq[i][b_]["labels"]) and torch.equal(per[i][b_]["loss"], seq[i][b_]["loss"])
               for i in range(N) for b_ in range(NB))
    inner, times = 5, {k: [] for k in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for k, f in fns.items():
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / inner)
    med = {k: _median(v) for k, v in times.items()}
    lines = ["pcl_bench --images %d: R=%d per image, K=%d, %d branches, G=%d labelled classes, boxes=%s, %s" %
             (N, R, K, NB, G, mode, torch.cuda.get_device_name(0)),
             "  medians of %d alternating rounds x %d calls (HIP events), us per call; [min .. max]" % (rounds, inner)]
    for k in fns:
        lines.append("  %-11s %9.1f   [%.1f .. %.1f]" % (k, med[k], min(times[k]), max(times[k])))
    lines += ["  batched / sequential (%d single-image triples) = %.3f   (gate: <= 1)" % (N, med["batched"] / med["sequential"]),
              "  batched / one single-image triple = %.3f" % (med["batched"] / med["one_image"]),
              "  per-image labels and losses equal the single-image path's: %s" % same]
    print("\n".join(lines))
    if out_path:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def bench_step(N, R, rounds, out_path, steps=40):
    """two step objects in one process: 1 image per step (the default head) and N images per step (enable_image_batches)"""
    import bench as B
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer
    from drn_wsod_pytorch_amd.modeling import build_model

    pkg = load_package()
    pkg.set_precision("bf16")
    runs = {}
    for ims in (1, N):
        torch.manual_seed(1234)
        cfg = B.build_cfg(pkg, "cuda")
        cfg.merge_from_list(["MODEL.ROI_HEADS.NAME", "PCLROIHeads"])
        model = build_model(cfg)
        B.init_weights(model, seed=0)
        model.train()
        if ims > 1:
            model.roi_heads.enable_image_batches(True)
        opt = build_optimizer(cfg, model)
        batches = B.synthetic_batches(8, R, cfg.MODEL.ROI_HEADS.NUM_CLASSES, "cuda", 0, pkg, ims)
        stp = GraphedTrainStep(model, opt, batches[0])
        runs[ims] = dict(stp=stp, batches=batches, pos=0, ms=[], last=None)

    def run(r, n):
        for _ in range(n):
            b = r["batches"]
            r["last"] = r["stp"].step(b[r["pos"] % len(b)], b[(r["pos"] + 1) % len(b)])
            r["pos"] += 1

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in runs.values():
        run(r, 10)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for r in runs.values():
            e0.record()
            run(r, steps)
            e1.record()
            torch.cuda.synchronize()
            r["ms"].append(e0.elapsed_time(e1) / steps)
    m1, mN = _median(runs[1]["ms"]), _median(runs[N]["ms"])
    lines = ["pcl_bench --images %d --step: PCLROIHeads on bench.py's R50-C4 / 224x224 / R=%d per image / K=20 / bf16 model, "
             "GraphedTrainStep (default form), %s" % (N, R, torch.cuda.get_device_name(0)),
             "  medians of %d alternating rounds x %d steps, ms per step (img/s); [min .. max]" % (rounds, steps),
             "  1 image per step   %.4f (%.1f)   [%.4f .. %.4f]" % (m1, 1e3 / m1, min(runs[1]["ms"]), max(runs[1]["ms"])),
             "  %d images per step  %.4f (%.1f)   [%.4f .. %.4f]" % (N, mN, N * 1e3 / mN, min(runs[N]["ms"]), max(runs[N]["ms"])),
             "  %d-image step / %d 1-image steps = %.3f" % (N, N, mN / (N * m1)),
             "  last losses, 1 image: %s" % {k: round(float(v.detach()), 4) for k, v in runs[1]["last"].items()},
             "  last losses, %d images: %s" % (N, {k: round(float(v.detach()), 4) for k, v in runs[N]["last"].items()})]
    print("\n".join(lines))
    if out_path:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--step", action="store_true", help="with --images N: time the whole N-image training step instead")
    ap.add_argument("--images", type=int, default=0, help="time an N-image batch against N single-image calls (0: off)")
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "pcl_batch_bench.txt"))
    args = ap.parse_args()
    R = int(os.environ.get("PCL_R", 2000))
    K, NB, G = 20, 3, int(os.environ.get("PCL_G", 2))
    mode = os.environ.get("PCL_BOXES", "random")
    if args.images > 0 and args.step:
        return bench_step(args.images, R, min(args.rounds, 7), args.out)
    if args.images > 0:
        return bench_images(args.images, R, K, NB, G, mode, args.rounds, args.out)
    boxes, ws, logits, onehot = _inputs(R, K, NB, G, mode, 7)
    dl = torch.zeros_like(logits)
    cols = [b_ * (K + 1) for b_ in range(NB)]

    def run():
        adj = ops.pcl_adjacency(boxes, 0.4)
        return ops.pcl_refine(logits, cols, K, ws, boxes, adj, onehot, dl)

    out = run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20
    e0.record()
    for _ in range(n):
        out = run()
    e1.record()
    torch.cuda.synchronize()
    print("R=%d boxes=%s G=%d: %.1f us per call (adjacency + softmax + refine, %d branches); centres per branch %s; "
          "fg rows per branch %s" % (R, mode, G, e0.elapsed_time(e1) * 1e3 / n, NB, [int(o["n_pc"]) for o in out],
                                     [int((o["labels"] > 0).sum()) for o in out]))


    if os.environ.get("PCL_PROFILE"):  # library built with -DPCL_PROFILE: phase clocks of branch 0 (100 MHz ticks)
        t = out[-1]["pc_scores"][-10:].cpu().numpy()
        names = ["gather+sort", "prefix+cuts", "k-means search", "members+degrees", "greedy loop", "top-5", "assign+stats",
                 "loss+dlogits"]
        print("  last branch phases (us):", {n_: round(float(v) / 100.0, 1) for n_, v in zip(names, t[:8])},
              "greedy iterations", int(t[8]))


if __name__ == "__main__":
    main()
