"""Time the standard ResNet trunks of the wsddn_R_50 / wsddn_R_101 recipes (build_resnet_backbone, bf16, full width, frozen):
the whole launch plan per image size - eager and as a replayed hipGraph, median of repeated timings - and the stem on its own:
the 7x7 / stride-2 conv launch, the 3x3 / stride-2 max-pool launch, the pair and the one-launch form
(drn_stem7x7_pool_nhwc), with the bytes they move against the 8 TB/s HBM
figure DESIGN.md uses.
  python tools/resnet_std_bench.py [--depth 50|101|both] [--sizes 224x224,800x1216] [--reps 30]
  python tools/resnet_std_bench.py --trace 50 800x1216     (a few plain forwards: run it under rocprofv3 --kernel-trace --stats
                                                            for the per-launch table)"""
import importlib
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package

pkg = load_package()
pkg.set_precision("bf16")
import resnet_std_util as U  # the recipes' recorded merged configs
from drn_wsod_pytorch_amd.modeling import build_backbone

ops = importlib.import_module("drn_wsod_pytorch_amd.ops")
HBM_TBS = 8.0


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def trunk(depth):
    rel = U.R50 if depth == 50 else U.R101
    bb = build_backbone(U.recorded_cfg(rel, tempfile.mkdtemp(), device="cuda")).cuda().eval()
    g = torch.Generator().manual_seed(depth)
    sd = {}
    for n, t in bb.state_dict().items():  # He-scaled weights, near-identity FrozenBN: O(1) activations at every depth
        if n.endswith("running_var"):
            sd[n] = torch.ones_like(t)
        elif n.endswith("running_mean") or n.endswith("norm.bias"):
            sd[n] = torch.zeros_like(t)
        elif n.endswith("norm.weight"):
            sd[n] = torch.full_like(t, 0.7)
        else:
            sd[n] = torch.randn(t.shape, generator=g) * (2.0 / (t.shape[1] * t.shape[2] * t.shape[3])) ** 0.5
    bb.load_state_dict(sd)
    return bb


def timed(fn, reps, inner=1):
    """median / min / max of `reps` event timings of fn() (us per call; fn runs `inner` calls)"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(ts), min(ts), max(ts)


def graphed(fn, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            out = fn()
    g.replay()
    torch.cuda.synchronize()
    return g, out


if "--trace" in sys.argv:
    i = sys.argv.index("--trace")
    depth, (H, W) = int(sys.argv[i + 1]), [int(v) for v in sys.argv[i + 2].split("x")]
    bb = trunk(depth)
    x = (torch.rand(1, 3, H, W, device="cuda") * 255 - 110)
    with torch.no_grad():
        for _ in range(5):
            bb(x)
    torch.cuda.synchronize()
    print("traced 5 forwards of R-%d at %dx%d" % (depth, H, W))
    raise SystemExit(0)

depths = {"50": [50], "101": [101], "both": [50, 101]}[arg("--depth", "both")]
sizes = [tuple(int(v) for v in s.split("x")) for s in arg("--sizes", "224x224,800x1216").split(",")]
reps = int(arg("--reps", "30"))
print("standard ResNet trunks, bf16, batch 1; median [min .. max] of %d timings" % reps)
for depth in depths:
    bb = trunk(depth)
    for H, W in sizes:
        x = (torch.rand(1, 3, H, W, device="cuda") * 255 - 110)
        xn = bb._input_nhwc(x)

        def fwd():
            with torch.no_grad():
                return bb._run_plan(xn)

        for _ in range(3):
            fwd()
        e = timed(fwd, reps)
        g, out = graphed(fwd, 1)
        t = timed(g.replay, reps)
        p = next(iter(bb._plans.values()))
        if os.environ.get("DRN_FUSE_STEM", "1") != "0":  # A/B in the same process: the same plan with the stem as two launches
            p["ops"][0].kind &= ~0x400
            g2, out2 = graphed(fwd, 1)
            t2 = timed(g2.replay, reps)
            p["ops"][0].kind |= 0x400
            if not torch.equal(out2["res5"], out["res5"]):
                print("  (!) the two forms of the plan differ")
            print("R-%-3d %4dx%-4d   the same plan with the stem as two launches: graph %8.1f us [%.1f .. %.1f]" % (depth, H, W, t2[0], t2[1], t2[2]))
        f = out["res5"]
        print("R-%-3d %4dx%-4d plan of %3d ops: eager %8.1f us [%.1f .. %.1f]   graph %8.1f us [%.1f .. %.1f]   res5 %s max|.| %.2f"
              % (depth, H, W, p["n_ops"], e[0], e[1], e[2], t[0], t[1], t[2], tuple(f.shape), float(f.float().abs().max())))
    del bb
    torch.cuda.empty_cache()

print("\nthe stem alone (conv 7x7 / 2 / 3, 8 stored channels -> 64, FrozenBN + ReLU; max pool 3x3 / 2 / 1), 20 launches per graph")
for H, W in sizes:
    x = (torch.randn(1, H, W, 8, device="cuda") * 50).to(torch.bfloat16)
    x[..., 3:] = 0
    wt = torch.zeros((64, ops.kpad(49 * 8, torch.bfloat16)), device="cuda", dtype=torch.bfloat16)
    wt[:, :49 * 8] = (torch.randn(64, 49, 8, device="cuda") * 0.05).to(torch.bfloat16).reshape(64, -1)
    scale, bias = torch.rand(64, device="cuda") + 0.5, torch.randn(64, device="cuda") * 0.1
    conv = lambda: ops.conv2d_nhwc(x, wt, 64, 7, 7, 2, 3, 1, scale, bias, None, True)
    y = conv()
    pool = lambda: ops.maxpool3x3s2_nhwc(y)
    pair = lambda: ops.maxpool3x3s2_nhwc(conv())
    ho, wo = y.shape[1:3]
    hp, wp = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
    mb = {"conv": (H * W * 8 + ho * wo * 64) * 2 / 1e6, "pool": (ho * wo * 64 + hp * wp * 64) * 2 / 1e6}
    mb["pair"] = mb["conv"] + mb["pool"]
    mb["fused (never written: the conv map)"] = (H * W * 8 + hp * wp * 64) * 2 / 1e6
    fused = lambda: ops.stem7x7_pool_nhwc(x, wt, 64, scale, bias, True)
    print("%4dx%-4d one launch vs two: %d differing elements of %d" % (H, W, int((fused() != pair()).sum()), hp * wp * 64))
    mb["fused"] = mb["fused (never written: the conv map)"]
    # (alternating order: conv, fused, pool, pair, then fused and conv again - the gate compares `fused` with `conv`)
    for name, fn in (("conv", conv), ("fused", fused), ("pool", pool), ("pair", pair), ("fused", fused), ("conv", conv)):
        g, _ = graphed(fn, 20)
        t = timed(g.replay, reps, 20)
        print("%4dx%-4d %-5s %8.1f us [%.1f .. %.1f]  %6.1f MB  %5.2f TB/s = %.2f of %.0f TB/s" % (
            H, W, name, t[0], t[1], t[2], mb[name], mb[name] / t[0], mb[name] / t[0] / HBM_TBS, HBM_TBS))  # MB / us = TB/s
    k = "fused (never written: the conv map)"
    print("%4dx%-4d bytes of a one-launch stem: %.1f MB = %.1f us at %.0f TB/s; conv FLOPs %.1f GF" % (
        H, W, mb[k], mb[k] / HBM_TBS, HBM_TBS, 2.0 * ho * wo * 64 * 49 * 3 / 1e9))
