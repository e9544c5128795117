"""CSCROIHeads at the shipped shape (csc_WSR_18_DC5_1x.yaml: WS-ResNet18 DC5, 4096-wide neck, 20 classes, one image per
GPU; 688 x 917 image, 2000 proposals), eager steps (the head reads K scores on the host each step):
  * step without class maps (past CSC_MAX_ITER / no class reaches tau: what a random-init model does at tau = 0.7),
  * step with N class maps (tau = 0: every labelled class gets its image-gradient pass),
  * one image-gradient pass alone (seed -> heads d/dx -> RoIPool backward -> trunk d/dx -> map -> table -> CSCPool).
  python tools/csc_bench.py [--precision bf16|fp32] [--arch wsr18|vgg16] [--classes 2]
--images N: one step on an N-image batch (CSCROIHeads.enable_image_batches: one image-gradient pass per class slot) against N
single-image steps of the same weights accumulated into one update, fp32 and bf16, alternating in one process, HIP events,
medians of >= 11 rounds, with the number of d/dx passes of each form; appended to profiles/csc_batch_bench.txt (--out)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "tests")))
import golden_util as G  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from oracle import wsod_oracle as O  # noqa: E402  (synthetic inputs only)

ap = argparse.ArgumentParser()
ap.add_argument("--precision", default="bf16")
ap.add_argument("--arch", default="wsr18")
ap.add_argument("--classes", type=int, default=2)
ap.add_argument("--H", type=int, default=688)
ap.add_argument("--W", type=int, default=917)
ap.add_argument("--R", type=int, default=2000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--images", type=int, default=0, help="N > 0: one N-image step (enable_image_batches) against N 1-image steps")
ap.add_argument("--rounds", type=int, default=11, help="--images: alternating rounds (medians; at least 11)")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "csc_batch_bench.txt"), help="--images: the figures are appended here")
args = ap.parse_args()
load_package()
from drn_wsod_pytorch_amd.engine import build_optimizer  # noqa: E402


def bench_images(N, precision):
    """One step on an N-image batch (CSCROIHeads.enable_image_batches) against N single-image steps of the same weights that
    accumulate into one update, alternating in one process; HIP events, medians.  csc_WSR_18_DC5 at a real image size, R
    proposals per image, K = 20, `--classes` labelled classes per image, all active (tau = 0)."""
    ocfg = O.OracleCfg(arch="wsr18", out_feature="res5", res5_dilation=1, res2_out=64, dan_dim=(4096, 4096), num_classes=20,
                       heads="csc", refine_num=0, refine_reg=(), mean_loss=False, base_lr=0.0)
    batch = O.synthetic_batch(N, args.R, ocfg, seed=3, H=args.H, W=args.W)
    for i, b in enumerate(batch):
        b["gt_classes"] = (torch.arange(args.classes) + i * args.classes) % 20
    cfg, model = G.drn_model(ocfg, 3, "cuda", 5, precision)
    model.train()
    heads = model.roi_heads
    heads.tau = 0.0
    opt = build_optimizer(cfg, model)
    whole, singles = G.drn_inputs(batch), [G.drn_inputs([b]) for b in batch]
    passes = [0]
    inner = heads._engine.input_gradient

    def counted(*a, **k):
        passes[0] += 1
        return inner(*a, **k)

    class _Counting:  # the engine's state is closed (__slots__): count through the head's view of it instead
        def __getattr__(self, name):
            return counted if name == "input_gradient" else getattr(heads._engine, name)

    counting = _Counting()
    w_single, w_batch = heads._csc_weights, heads._csc_weights_batch
    heads._csc_weights = lambda eng, *a, **k: w_single(counting, *a, **k)
    heads._csc_weights_batch = lambda eng, *a, **k: w_batch(counting, *a, **k)

    def step(batched):
        heads.enable_image_batches(batched)
        opt.zero_grad()
        for x in ([whole] if batched else singles):
            heads.iter = 1
            losses = model(x)
            if not model.backward_losses(1.0 if batched else 1.0 / N):
                (sum(losses.values()) * (1.0 if batched else 1.0 / N)).backward()
        opt.step()
        return losses

    count = {}
    for form in (True, False):
        for _ in range(2):
            step(form)
        passes[0] = 0
        step(form)
        count[form] = passes[0]
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {True: [], False: []}
    rounds = max(11, args.rounds)
    for _ in range(rounds):
        for form in (True, False):
            e0.record()
            step(form)
            e1.record()
            e1.synchronize()
            times[form].append(e0.elapsed_time(e1))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    lines = ["csc_bench --images %d --precision %s: csc_WSR_18_DC5, image %dx%d, R=%d per image, K=20, %d labelled classes per "
             "image, all active (tau = 0), %s" % (N, precision, args.H, args.W, args.R, args.classes,
                                                  torch.cuda.get_device_name(0)),
             "  medians of %d alternating rounds (HIP events), ms per update of %d images; [min .. max]" % (rounds, N),
             "  one %d-image step      %8.3f   [%.3f .. %.3f]   d/dx passes: %d" % (
                 N, med[True], min(times[True]), max(times[True]), count[True]),
             "  %d single-image steps  %8.3f   [%.3f .. %.3f]   d/dx passes: %d" % (
                 N, med[False], min(times[False]), max(times[False]), count[False]),
             "  batched / sequential = %.3f" % (med[True] / med[False])]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if args.images > 0:
    for prec in ("fp32", "bf16"):
        bench_images(args.images, prec)
        torch.cuda.empty_cache()
    sys.exit(0)

if args.arch == "vgg16":
    ocfg = O.OracleCfg(arch="vgg16", out_feature="plain5", res5_dilation=2, dan_dim=(4096, 4096), num_classes=20,
                       pixel_mean=(103.939, 116.779, 123.68), heads="csc", refine_num=0, refine_reg=(), mean_loss=False,
                       base_lr=1e-5)
else:
    ocfg = O.OracleCfg(arch="wsr18", out_feature="res5", res5_dilation=1, res2_out=64, dan_dim=(4096, 4096),
                       num_classes=20, heads="csc", refine_num=0, refine_reg=(), mean_loss=False, base_lr=1e-5)
batch = O.synthetic_batch(1, args.R, ocfg, seed=3, H=args.H, W=args.W)
batch[0]["gt_classes"] = torch.arange(args.classes)
ocfg.base_lr = 0.0  # the weights stay where the seeded init put them: every timed step does the same work
cfg, model = G.drn_model(ocfg, 3, "cuda", 5, args.precision)
model.train()
opt = build_optimizer(cfg, model)
inputs = G.drn_inputs(batch)


def run(n, tau, it):
    model.roi_heads.tau = tau
    for i in range(n):
        model.roi_heads.iter = it
        opt.zero_grad()
        losses = model(inputs)
        sum(losses.values()).backward()
        opt.step()
    torch.cuda.synchronize()


def timed(tau, it):
    run(3, tau, it)
    t0 = time.perf_counter()
    run(args.steps, tau, it)
    return (time.perf_counter() - t0) / args.steps * 1e3


t_plain = timed(0.7, 10 ** 9)
t_maps = timed(0.0, 1)
aux = model.roi_heads._last_state["aux"]
nz = int((aux["cpgs"].flatten(1).amax(1) > 0).sum())
print("CSC %s %s  image %dx%d  R=%d  K=20: step without maps %.2f ms, with %d class maps %.2f ms -> %.2f ms per "
      "image-gradient pass (maps non-zero: %d; W range %.3f .. %.3f; losses %s)" % (
          args.arch, args.precision, args.H, args.W, args.R, t_plain, args.classes, t_maps,
          (t_maps - t_plain) / max(1, args.classes), nz, float(aux["W"].min()), float(aux["W"].max()),
          {k: round(float(v), 4) for k, v in model(inputs).items()}))
