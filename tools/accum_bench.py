"""Gradient accumulation (WSL.ITER_SIZE = N) on the graphed, fused step: what a window of N micro-iterations costs.

BASELINE configs[1] (R50-C4, 224 x 224, R = 2000, bf16, one GPU, synthetic inputs built as bench.py builds them), three forms in
ONE process, timed in alternating rounds, medians over the rounds:

  (a) GraphedTrainStep at iter_size = 1                 - bench.py's step: an optimizer step per image
  (b) GraphedTrainStep at iter_size = N, whole windows  - N - 1 accumulating micro-steps (drn_gemm_tn, fp32 C into the arena) and
                                                          one closing micro-step (drn_gemm_tn_acc_sgd); per-launch durations of
                                                          both from HIP events on their stream (sampled micro-steps)
  (c) the eager unpipelined Trainer with ITER_SIZE = N  - the only way to run such a recipe without (b)

and the gate for the fused closing launch: drn_gemm_tn_acc_sgd against the unfused closing sequence it replaces (drn_gemm_tn
accumulate + drn_cast2d + drn_sgd_step_block) at the fc6 shape, alternating on one stream, medians.

    python tools/accum_bench.py [--iter-size 32] [--rounds 5] [--windows 2] [--out profiles/accum_bench.txt]"""
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


def med(xs):
    return statistics.median(xs) if xs else float("nan")


def spread(xs):
    return "%.1f [%.1f .. %.1f] n=%d" % (med(xs), min(xs), max(xs), len(xs)) if xs else "-"


def make_model(pkg, device, iter_size):
    from drn_wsod_pytorch_amd.engine import build_optimizer
    from drn_wsod_pytorch_amd.modeling import build_model

    cfg = bench.build_cfg(pkg, device)
    cfg.WSL.ITER_SIZE = iter_size
    model = build_model(cfg)
    bench.init_weights(model, seed=0)
    model.train()
    return cfg, model, build_optimizer(cfg, model)


def closing_gate(ops, device, D1, K1, R, reps):
    """the fused closing launch against the unfused closing sequence, same buffers, alternating, HIP events on one stream"""
    Mp = ops.kpad(R, torch.bfloat16)
    g = torch.Generator(device="cpu").manual_seed(5)
    dPT = torch.zeros((D1, Mp), dtype=torch.bfloat16, device=device)
    dPT[:, :R] = (torch.randn((D1, R), generator=g) * 0.05).to(device, torch.bfloat16)
    A = (torch.rand((R, K1), generator=g)).to(device, torch.bfloat16)
    acc = (torch.randn((D1, 1024), generator=g) * 0.5).to(device).repeat(1, K1 // 1024 + 1)[:, :K1].contiguous()
    w = torch.randn((D1 * K1,), generator=g).to(device) * 0.01
    mom, sh = torch.zeros_like(w), torch.zeros((D1 * K1,), dtype=torch.bfloat16, device=device)
    bucket = torch.zeros((D1, K1), dtype=torch.bfloat16, device=device)
    seg = np.zeros(1, dtype=[("off", "<i8"), ("cnt", "<i8"), ("lr", "<f4"), ("wd", "<f4")])
    seg[0] = (0, D1 * K1, 1e-4, 5e-4)
    seg_dev = torch.from_numpy(seg.view(np.uint8)).to(device)
    v2 = lambda t: t.view(D1, K1)
    scratch = acc.clone()

    def fused():
        assert ops.gemm_tn_acc_sgd(dPT, A, D1, K1, Mp, R, acc, bucket, v2(w), v2(mom), v2(sh), seg_dev, 0.9, False, 1.0)

    def unfused():
        ops.gemm_tn(dPT, A, D1, K1, Mp, R, out=scratch.unsqueeze(0), accumulate=True)
        ops.cast2d(scratch, D1, K1, bucket)
        ops.sgd_step_block(w, mom, bucket, seg_dev, 0, D1, 0, K1, K1, 0.9, False, 1.0, shadow=sh, grad_off=0)

    def accumulate_only():
        ops.gemm_tn(dPT, A, D1, K1, Mp, R, out=scratch.unsqueeze(0), accumulate=True)

    forms = {"fused closing (drn_gemm_tn_acc_sgd)": fused, "unfused closing (gemm_tn acc + cast2d + sgd_step_block)": unfused,
             "accumulating micro-step (drn_gemm_tn, fp32 C, accumulate)": accumulate_only}
    times = {k: [] for k in forms}
    for k, fn in forms.items():
        fn()  # warm
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in forms.items():
            scratch.copy_(acc)  # (keeps the accumulator's values bounded over the repetitions)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iter-size", type=int, default=32)
    ap.add_argument("--proposals", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5, help="alternating timing rounds per form")
    ap.add_argument("--windows", type=int, default=2, help="whole windows per timing round")
    ap.add_argument("--gate-reps", type=int, default=15)
    ap.add_argument("--trunk-group", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_bench.txt"))
    args = ap.parse_args()
    N, R = args.iter_size, args.proposals
    device = "cuda:0"
    torch.cuda.set_device(0)
    torch.manual_seed(1234)
    pkg = load_package()
    pkg._cabi.lib()
    pkg.set_precision("bf16")
    from drn_wsod_pytorch_amd import ops
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, Trainer

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    G = args.trunk_group
    n_ahead = 2 * G
    steps = N * args.windows
    say("accum_bench: R50-C4 224x224 R=%d bf16, ITER_SIZE %d, %d rounds x %d micro-steps per form, device %s"
        % (R, N, args.rounds, steps, torch.cuda.get_device_name(0)))

    # ---- the three forms -------------------------------------------------------------------------------------------------
    cfg_a, model_a, opt_a = make_model(pkg, device, 1)
    K = cfg_a.MODEL.ROI_HEADS.NUM_CLASSES
    batches = bench.synthetic_batches(8, R, K, device, 0, pkg, 1)
    window = lambda j: [batches[(j + q) % len(batches)] for q in range(n_ahead)]
    opt_a.enable_pipelined(None)
    stp_a = GraphedTrainStep(model_a, opt_a, batches[0], split_tail=True, lookahead=2, trunk_pairs=G, eager_fc6=True)
    cfg_b, model_b, opt_b = make_model(pkg, device, N)
    opt_b.enable_pipelined(None, iter_size=N)
    fused_on = model_b.roi_heads._engine.fc1_fused_tn is not None
    stp_b = GraphedTrainStep(model_b, opt_b, batches[0], split_tail=True, lookahead=2, trunk_pairs=G, eager_fc6=True)
    cfg_c, model_c, opt_c = make_model(pkg, device, N)

    def cycle():
        i = 0
        while True:
            yield batches[i % len(batches)]
            i += 1

    tr_c = Trainer(cfg_c, model_c, cycle(), optimizer=opt_c)
    pos = {"a": 0, "b": 0}

    def run_a(n):
        for _ in range(n):
            last = stp_a.step(*window(pos["a"]))
            pos["a"] += 1
        return last

    def run_b(n, timing=None):
        for i in range(n):
            # (HIP events on every closing micro-step - the rounds start at it % N == 1 - and on every 8th accumulating one)
            ops.GEMM_TIMING = timing if (timing is not None and (i % N == N - 1 or i % 8 == 3)) else None
            last = stp_b.step(*window(pos["b"]))
            pos["b"] += 1
        ops.GEMM_TIMING = None
        return last

    def run_c(n):
        for _ in range(n):
            last = tr_c.run_step()
        return last

    # warm-up: prime + capture, then one whole window each; (b) and (c) start their timed rounds on a window boundary (it % N == 1)
    run_a(8)
    run_b(1 + N)
    run_c(1 + N)
    torch.cuda.synchronize()
    assert pos["b"] % N == 1 and tr_c.iter % N == 1
    rate = {"a": [], "b": [], "c": []}
    gemm_events = []
    for _ in range(args.rounds):
        for name, fn in (("a", lambda: run_a(steps)), ("b", lambda: run_b(steps, gemm_events)), ("c", lambda: run_c(steps))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = fn()
            torch.cuda.synchronize()
            rate[name].append(steps / (time.perf_counter() - t0))
            bench.assert_sane_losses({k: v.detach() for k, v in last.items()}, "form (%s)" % name)
    D1, K1 = model_b.roi_heads.box_head.fc1.weight.shape
    acc_us = [e0.elapsed_time(e1) * 1e3 for e0, e1, _, tag in gemm_events if tag == (D1, K1, ops.kpad(R, torch.bfloat16))]
    close_us = [e0.elapsed_time(e1) * 1e3 for e0, e1, _, tag in gemm_events if tag[0] == "tn_acc_sgd"]
    fwd_us = [e0.elapsed_time(e1) * 1e3 for e0, e1, _, tag in gemm_events if tag[:2] == (R, D1)]
    say()
    say("form                                                   img/s median [min .. max]")
    say("(a) GraphedTrainStep, iter_size 1                      %s" % spread(rate["a"]))
    say("(b) GraphedTrainStep, iter_size %-3d (fused closing %s)  %s" % (N, "on" if fused_on else "off", spread(rate["b"])))
    say("(c) eager unpipelined Trainer, ITER_SIZE %-3d            %s" % (N, spread(rate["c"])))
    say("(b) / (c) = %.2f    (b) / (a) = %.2f" % (med(rate["b"]) / med(rate["c"]), med(rate["b"]) / med(rate["a"])))
    say()
    say("in-step launch durations of (b), HIP events on the main stream, us median [min .. max]")
    say("  fc6 forward (drn_gemm_nt, eager)                      %s" % spread(fwd_us))
    say("  accumulating dW (drn_gemm_tn, fp32 C, accumulate)     %s" % spread(acc_us))
    say("  closing dW + SGD (drn_gemm_tn_acc_sgd)                %s" % spread(close_us))
    stp_a.release(), stp_b.release()
    del stp_a, stp_b, tr_c, model_a, model_b, model_c, opt_a, opt_b, opt_c
    torch.cuda.empty_cache()

    # ---- the gate ----------------------------------------------------------------------------------------------------------
    gate = closing_gate(ops, device, D1, K1, R, args.gate_reps)
    say()
    say("closing launch alone at the fc6 shape [%d x %d] x K %d, alternating, us median [min .. max]" % (D1, K1, R))
    for k, v in gate.items():
        say("  %-58s %s" % (k, spread(v)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
