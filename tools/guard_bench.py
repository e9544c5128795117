"""The anomaly guard (FusedSGD(nonfinite=...)): what it costs on the graphed bench-shape step - BASELINE configs[1] (R50-C4, 224 x 224,
R = 2000, bf16, one GPU, synthetic inputs built as bench.py builds them), GraphedTrainStep as bench.py runs it - with the guard
off and with nonfinite="raise", in ONE process, alternating, `--repeats` timing rounds of `--steps` steps each, img/s.  The guard adds
one one-wave launch (drn_loss_guard) behind the loss tail of the captured heads graph and switches every update launch - the fused
fc6 dW + SGD launch included - to its guarded instantiation.  The difference is reported beside the off runs' own spread.

    python tools/guard_bench.py [--repeats 3] [--steps 200] [--out profiles/guard_bench.txt]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proposals", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3, help="alternating timing rounds per form")
    ap.add_argument("--steps", type=int, default=200, help="steps per timing round")
    ap.add_argument("--trunk-group", type=int, default=4)
    ap.add_argument("--note", action="append", default=[], help="a line copied into the profile")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guard_bench.txt"))
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
    say("guard_bench: R50-C4 224x224 R=%d bf16, device %s" % (R, torch.cuda.get_device_name(0)))
    cfg = bench.build_cfg(pkg, device)
    batches = bench.synthetic_batches(8, R, cfg.MODEL.ROI_HEADS.NUM_CLASSES, device, 0, pkg, 1)
    window = lambda j: [batches[(j + q) % len(batches)] for q in range(2 * G)]
    runs = {}
    for mode in ("off", "raise"):
        model = build_model(cfg)
        bench.init_weights(model, seed=0)
        model.train()
        opt = build_optimizer(cfg, model, nonfinite=mode)
        opt.enable_pipelined(None)
        stp = GraphedTrainStep(model, opt, batches[0], split_tail=True, lookahead=2, trunk_pairs=G, eager_fc6=True)
        runs[mode] = dict(stp=stp, pos=0, rate=[], opt=opt, model=model, fused=model.roi_heads._engine.fc1_fused_tn is not None)

    def run(r, n):
        for _ in range(n):
            last = r["stp"].step(*window(r["pos"]))
            r["pos"] += 1
        return last

    for r in runs.values():
        run(r, 8)
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for mode, r in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = run(r, args.steps)
            torch.cuda.synchronize()
            r["rate"].append(args.steps / (time.perf_counter() - t0))
            bench.assert_sane_losses({k: v.detach() for k, v in last.items()}, mode)
    say()
    say("GraphedTrainStep on enable_pipelined(), %d alternating rounds x %d steps, img/s (us per step)" % (args.repeats, args.steps))
    for mode, r in runs.items():
        say("  nonfinite=%-6s fused_tn %-3s rounds %s   median %.1f img/s (%.1f us)"
            % (mode, "on" if r["fused"] else "off", " ".join("%.1f" % x for x in r["rate"]), statistics.median(r["rate"]),
               1e6 / statistics.median(r["rate"])))
    off, on = runs["off"]["rate"], runs["raise"]["rate"]
    d_us = 1e6 / statistics.median(on) - 1e6 / statistics.median(off)
    spread_us = 1e6 / min(off) - 1e6 / max(off)
    say("  raise - off = %+.1f us per step (%+.2f %%); the off rounds' own spread: %.1f us" %
        (d_us, 100.0 * d_us * statistics.median(off) / 1e6, spread_us))
    st = runs["raise"]["opt"].guard_state()
    say("  guard state after the run: %s" % (st,))
    assert st["bad"] == 0 and st["calls"] == runs["raise"]["pos"], st
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
