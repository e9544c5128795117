"""SOLVER.CLIP_GRADIENTS: what clipping costs, at BASELINE configs[1]'s arena (R50-C4, 224 x 224, R = 2000, bf16, one GPU, synthetic
inputs built as bench.py builds them), in ONE process:

  1. drn_grad_norms over the whole fp32 gradient arena and over the fc6 bf16 bucket, with the achieved GB/s beside the stand-alone
     drn_sgd_step of the same run (alternating launches, one HIP event pair per launch, medians);
  2. the plain optimizer step() unclipped, value-clipped and norm-clipped (the same optimizer, the same gradients);
  3. GraphedTrainStep with value clipping (fc6 dW unfused, every bucket through the clipping entry points) against the graphed step as
     shipped (fused fc6 dW + SGD), alternating rounds, img/s.

`--note` lines (e.g. the bench.py result lines of this tree and of its parent on the same box) are copied into the profile.

    python tools/clip_bench.py [--launches 30] [--rounds 5] [--steps 60] [--out profiles/clip_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

HBM_GBS = 8000.0


def med(xs):
    return statistics.median(xs) if xs else float("nan")


def spread(xs):
    return "%.1f [%.1f .. %.1f] n=%d" % (med(xs), min(xs), max(xs), len(xs)) if xs else "-"


def make_model(pkg, device, clip=None):
    from drn_wsod_pytorch_amd.engine import build_optimizer
    from drn_wsod_pytorch_amd.modeling import build_model

    cfg = bench.build_cfg(pkg, device)
    if clip is not None:
        cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
        cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE, cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = clip
    model = build_model(cfg)
    bench.init_weights(model, seed=0)
    model.train()
    return cfg, model, build_optimizer(cfg, model)


def alternate(forms, reps):
    """forms: {label: callable}; every repetition runs each form once, each launch between its own pair of HIP events -> us"""
    times = {k: [] for k in forms}
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proposals", type=int, default=2000)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5, help="alternating timing rounds per graphed form")
    ap.add_argument("--steps", type=int, default=60, help="steps per timing round")
    ap.add_argument("--trunk-group", type=int, default=4)
    ap.add_argument("--note", action="append", default=[], help="a line copied into the profile")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU (no fallback)"
    R = args.proposals
    device = "cuda:0"
    torch.cuda.set_device(0)
    torch.manual_seed(1234)
    pkg = load_package()
    pkg._cabi.lib()
    pkg.set_precision("bf16")
    from drn_wsod_pytorch_amd import ops
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("clip_bench: R50-C4 224x224 R=%d bf16, device %s" % (R, torch.cuda.get_device_name(0)))

    # ---- 1 + 2: the kernels and the plain step on one model's arena ---------------------------------------------------------
    cfg, model, opt = make_model(pkg, device)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    batches = bench.synthetic_batches(8, R, K, device, 0, pkg, 1)
    opt.zero_grad()
    losses = model(batches[0])
    sum(losses.values()).backward()
    opt.step()  # momentum exists, tables are on the device; the gradients stay valid for the timed steps below
    torch.cuda.synchronize()
    eng = model.roi_heads._engine
    segs, nseg = opt._segs()
    n_arena = sum(g["cnt"] for g in opt.param_groups if g["used"])
    o1, n1 = eng._seg["fc1.weight"]
    seg = np.zeros(1, dtype=[("off", "<i8"), ("cnt", "<i8"), ("lr", "<f4"), ("wd", "<f4")])
    seg[0] = (o1, n1, 0.0, 0.0)
    fc1_seg = torch.from_numpy(seg.view(np.uint8)).to(device)
    bucket = eng.arena_g[o1: o1 + n1].to(torch.bfloat16)
    norms = torch.empty((nseg,), dtype=torch.float32, device=device)
    ws = torch.empty((ops.grad_norms_ws_bytes(nseg),), dtype=torch.uint8, device=device)
    shadow = eng.arena_s
    per_elem_sgd = 4 + 8 + 8 + (2 if shadow is not None else 0)  # g read; w, momentum read + written; bf16 shadow written
    forms = {
        "drn_grad_norms L2, fp32 arena (%d segments)" % nseg:
            (lambda: ops.grad_norms(eng.arena_g, segs, nseg, 2.0, 1.0, out=norms, workspace=ws), 4 * n_arena),
        "drn_grad_norms inf, fp32 arena":
            (lambda: ops.grad_norms(eng.arena_g, segs, nseg, float("inf"), 1.0, out=norms, workspace=ws), 4 * n_arena),
        "drn_grad_norms L2, fc6 bf16 bucket":
            (lambda: ops.grad_norms(bucket, fc1_seg, 1, 2.0, 1.0, grad_off=o1, out=norms[:1], workspace=ws), 2 * n1),
        "drn_sgd_step, fp32 arena (stand-alone)":
            (lambda: ops.sgd_step(eng.arena_w, opt._mom, eng.arena_g, segs, nseg, 0.9, False, 1.0, shadow=shadow),
             per_elem_sgd * n_arena),
        "drn_sgd_step_clip value, fp32 arena":
            (lambda: ops.sgd_step(eng.arena_w, opt._mom, eng.arena_g, segs, nseg, 0.9, False, 1.0, shadow=shadow,
                                  clip=(ops.CLIP_VALUE, 1.0, None)), per_elem_sgd * n_arena),
        "drn_sgd_step_clip norm, fp32 arena":
            (lambda: ops.sgd_step(eng.arena_w, opt._mom, eng.arena_g, segs, nseg, 0.9, False, 1.0, shadow=shadow,
                                  clip=(ops.CLIP_NORM, 1.0, norms)), per_elem_sgd * n_arena),
    }
    t = alternate({k: v[0] for k, v in forms.items()}, args.launches)
    say()
    say("kernels at the heads' arena (%d elements, %.0f MB fp32; fc6.weight %d elements), alternating, %d launches each"
        % (n_arena, 4 * n_arena / 1e6, n1, args.launches))
    say("%-46s %28s %9s %8s %7s" % ("launch", "us median [min .. max]", "MB moved", "GB/s", "roof"))
    for k, (_, nbytes) in forms.items():
        gbs = nbytes / med(t[k]) / 1e3
        say("%-46s %28s %9.1f %8.0f %7.3f" % (k, spread(t[k]), nbytes / 1e6, gbs, gbs / HBM_GBS))

    def plain(clip_type):
        def run():
            opt.clip_type = clip_type
            opt.step()
        return run

    t = alternate({"plain step(), unclipped": plain(None), "plain step(), CLIP_TYPE value": plain("value"),
                   "plain step(), CLIP_TYPE norm (L2)": plain("norm")}, args.launches)
    opt.clip_type = None
    say()
    say("the plain optimizer step (the heads' arena, same gradients), alternating, us median [min .. max]")
    for k, v in t.items():
        say("  %-44s %s" % (k, spread(v)))
    del model, opt, eng, bucket, forms, losses, shadow
    torch.cuda.empty_cache()

    # ---- 3: the graphed step ---------------------------------------------------------------------------------------------
    G = args.trunk_group
    window = lambda j: [batches[(j + q) % len(batches)] for q in range(2 * G)]
    runs = {}
    for label, clip in (("as shipped (fused fc6 dW + SGD)", None), ("value clipping (unfused)", ("value", 1.0))):
        cfg_i, model_i, opt_i = make_model(pkg, device, clip)
        opt_i.enable_pipelined(None)
        fused = model_i.roi_heads._engine.fc1_fused_tn is not None
        stp = GraphedTrainStep(model_i, opt_i, batches[0], split_tail=True, lookahead=2, trunk_pairs=G, eager_fc6=True)
        runs[label] = dict(stp=stp, pos=0, rate=[], fused=fused, keep=(model_i, opt_i))

    def run(r, n):
        for _ in range(n):
            last = r["stp"].step(*window(r["pos"]))
            r["pos"] += 1
        return last

    for r in runs.values():
        run(r, 8)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for label, r in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = run(r, args.steps)
            torch.cuda.synchronize()
            r["rate"].append(args.steps / (time.perf_counter() - t0))
            bench.assert_sane_losses({k: v.detach() for k, v in last.items()}, label)
    say()
    say("GraphedTrainStep on enable_pipelined(), %d alternating rounds x %d steps, img/s median [min .. max]" % (args.rounds, args.steps))
    for label, r in runs.items():
        say("  %-36s fused_tn %-3s %s" % (label, "on" if r["fused"] else "off", spread(r["rate"])))
    a, b = [med(r["rate"]) for r in runs.values()]
    say("  clipped / shipped = %.3f" % (b / a))
    for r in runs.values():
        r["stp"].release()
    if args.note:
        say()
        for n in args.note:
            say(n)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
