"""Time the box regression of the PCL heads (reg/pcl_* recipes) at R = 2000 proposals, K = 20 classes, an annotated block of 64 boxes
per image, one regressing branch.

default: the fused launch pair (drn_annot_box_reg: labelling, target, loss and dlogits) against the composition of the kernels
         that existed before it (drn_label_proposals + a gather of the matched boxes + drn_box_reg_loss), one process, alternating
         rounds, HIP events, medians; the two must give the same dlogits bit for bit and the same loss.
--step:  the whole training step (bench.py's R50-C4 model and synthetic batches, bf16, GraphedTrainStep in its default form) of
         PCLROIHeads with REFINE_NUM 4 / REFINE_REG [F, F, F, T] against the same head without the regressing flag (the plain pcl
         step with as many branches), same process, alternating rounds, learning rate 0 (the optimizer's launches run, the weights
         stay: both heads then cluster the same scores, which is what the PCL launches' time depends on).
Appends the figures to profiles/pcl_reg_bench.txt (--out)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from drn_wsod_pytorch_amd import ops  # noqa: E402

W4 = (10.0, 10.0, 5.0, 5.0)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _emit(lines, out_path):
    print("\n".join(lines))
    if out_path:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def _inputs(R, K, G, max_gt, seed):
    """R proposals of a 224 x 224 image, G annotated boxes (a third of the proposals sit next to one), K-class deltas behind the
    (K + 1)-wide columns of four branches"""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(G, 2, generator=g) * 120
    gb = torch.cat([xy, xy + 30 + torch.rand(G, 2, generator=g) * 70], 1)
    x0, y0 = torch.rand(R, generator=g) * 184, torch.rand(R, generator=g) * 184
    props = torch.stack([x0, y0, x0 + 20 + torch.rand(R, generator=g) * (204 - x0), y0 + 20 + torch.rand(R, generator=g) * (204 - y0)], 1)
    near = torch.rand(R, generator=g) < 0.33
    pick = torch.randint(0, G, (R,), generator=g)
    props[near] = (gb[pick] + torch.randn(R, 4, generator=g) * 3)[near]
    gt_boxes = torch.zeros(1, max_gt, 4)
    gt_boxes[0, :G] = gb
    gt_classes = torch.zeros(1, max_gt, dtype=torch.int32)
    gt_classes[0, :G] = torch.randint(0, K, (G,), generator=g, dtype=torch.int32)
    col0 = 2 * K + 4 * (K + 1)
    logits = torch.randn(R, col0 + 4 * K, generator=g) * 2
    return dict(props=props.contiguous().cuda(), gt_boxes=gt_boxes.cuda(), gt_classes=gt_classes.cuda(),
                gt_count=torch.tensor([G], dtype=torch.int32).cuda(), logits=logits.cuda(), col0=col0,
                img_off=torch.tensor([0, R], dtype=torch.int32).cuda())


def bench_kernels(R, K, G, max_gt, rounds, out_path, inner=20):
    x = _inputs(R, K, G, max_gt, 11)
    dl_a, dl_b = torch.zeros_like(x["logits"]), torch.zeros_like(x["logits"])

    def fused():
        return ops.annot_box_reg(x["logits"], [x["col0"]], K, x["props"], x["img_off"], 1, x["gt_boxes"], x["gt_classes"], x["gt_count"],
                                 (0.5,), (0, 1), W4, dlogits=dl_a)

    def composed():
        lp = ops.label_proposals(x["props"], x["img_off"], 1, x["gt_boxes"], x["gt_classes"], x["gt_count"], K, (0.5,), (0, 1))
        gathered = x["gt_boxes"][0].index_select(0, lp["matched"])
        return ops.box_reg_loss(x["logits"], x["col0"], K, lp["labels"], x["props"], gathered, W4, dlogits=dl_b)

    fns = dict(fused=fused, composed=composed)
    for f in fns.values():
        for _ in range(5):
            f()
    la, lb = fused(), composed()
    torch.cuda.synchronize()
    same = torch.equal(dl_a, dl_b) and torch.equal(la, lb)
    n_fg = int((dl_a != 0).any(1).sum())
    times = {k: [] for k in fns}
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
    lines = ["pcl_reg_bench: R=%d, K=%d, %d annotated boxes in a block of %d, one regressing branch, %d foreground rows, %s" %
             (R, K, G, max_gt, n_fg, torch.cuda.get_device_name(0)),
             "  medians of %d alternating rounds x %d calls (HIP events, eager launches incl. their host side), us per call; "
             "[min .. max]" % (rounds, inner)]
    for k in fns:
        lines.append("  %-9s %9.1f   [%.1f .. %.1f]" % (k, med[k], min(times[k]), max(times[k])))
    lines += ["  fused (drn_annot_box_reg) / composed (drn_label_proposals + gather + drn_box_reg_loss) = %.3f" %
              (med["fused"] / med["composed"]),
              "  dlogits and loss bit-equal between the two: %s" % same]
    _emit(lines, out_path)


def bench_step(R, rounds, out_path, steps=40):
    import bench as B
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer
    from drn_wsod_pytorch_amd.modeling import build_model

    pkg = load_package()
    pkg.set_precision("bf16")
    runs = {}
    for name, reg in (("pcl", "[False, False, False, False]"), ("reg/pcl", "[False, False, False, True]")):
        torch.manual_seed(1234)
        cfg = B.build_cfg(pkg, "cuda")
        # (BASE_LR 0: the clustering's cost follows the scores, and two models that train apart would be timed on different
        # clusterings - with the weights held both heads cluster the same proposals on the same scores, step for step)
        cfg.merge_from_list(["MODEL.ROI_HEADS.NAME", "PCLROIHeads", "WSL.REFINE_NUM", "4", "WSL.REFINE_REG", reg,
                             "SOLVER.BASE_LR", "0.0"])
        model = build_model(cfg)
        B.init_weights(model, seed=0)
        model.train()
        opt = build_optimizer(cfg, model)
        batches = B.synthetic_batches(8, R, cfg.MODEL.ROI_HEADS.NUM_CLASSES, "cuda", 0, pkg, 1)
        runs[name] = dict(stp=GraphedTrainStep(model, opt, batches[0]), batches=batches, pos=0, ms=[], last=None)

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
    lines = ["pcl_reg_bench --step: PCLROIHeads, 4 branches, on bench.py's R50-C4 / 224x224 / R=%d / K=20 / bf16 model, "
             "GraphedTrainStep (default form), BASE_LR 0, %s" % (R, torch.cuda.get_device_name(0)),
             "  medians of %d alternating rounds x %d steps, ms per step (img/s); [min .. max]" % (rounds, steps)]
    med = {}
    for name, r in runs.items():
        med[name] = _median(r["ms"])
        lines.append("  %-8s %.4f (%.1f)   [%.4f .. %.4f]" % (name, med[name], 1e3 / med[name], min(r["ms"]), max(r["ms"])))
    lines.append("  reg/pcl step / pcl step = %.4f" % (med["reg/pcl"] / med["pcl"]))
    for name, r in runs.items():
        lines.append("  last losses, %s: %s" % (name, {k: round(float(v.detach()), 4) for k, v in r["last"].items()}))
    _emit(lines, out_path)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--step", action="store_true", help="time the whole reg/pcl training step against the plain pcl step")
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "pcl_reg_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU: nothing is measured without one"
    R = int(os.environ.get("PCL_R", 2000))
    if args.step:
        return bench_step(R, min(args.rounds, 7), args.out)
    return bench_kernels(R, 20, int(os.environ.get("PCL_G", 8)), 64, args.rounds, args.out)


if __name__ == "__main__":
    main()
