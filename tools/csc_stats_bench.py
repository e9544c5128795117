"""What CSCROIHeads.enable_csc_stats costs, at the shape of tools/csc_bench.py (csc_WSR_18_DC5: WS-ResNet18 DC5, 4096-wide neck,
K = 20, 688 x 917 image, 2000 proposals per image, `--classes` labelled classes per image, all active: tau = 0), for one image
per step and for a 4-image batch (enable_image_batches):
  * drn_csc_stats alone on the step's own tensors: HIP events around `--reps` back-to-back calls, median over the rounds;
  * the whole eager step (forward, backward, update) with the option on against off: three forms alternate in one process -
    off, on, off again - HIP events, medians; the difference of the two identical off forms is the noise the on / off
    difference has to be read against;
  * for context, the reference's method on the same tensors: W_pos, W_neg, the labels, the image scores and the two weighted sums
    copied to the host (blocking, as .cpu().numpy() is), then a Python loop over labelled classes x rows; host clock, per image.
  python tools/csc_stats_bench.py [--precision bf16] [--rounds 21]        -> profiles/csc_stats_bench.txt (--out)
There is no pass / fail figure."""
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
ap.add_argument("--classes", type=int, default=2)
ap.add_argument("--H", type=int, default=688)
ap.add_argument("--W", type=int, default=917)
ap.add_argument("--R", type=int, default=2000)
ap.add_argument("--rounds", type=int, default=21, help="alternating rounds (medians; at least 11)")
ap.add_argument("--reps", type=int, default=50, help="back-to-back kernel calls per timed window")
ap.add_argument("--images", default="1,4")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "csc_stats_bench.txt"))
args = ap.parse_args()
load_package()
from drn_wsod_pytorch_amd import ops  # noqa: E402
from drn_wsod_pytorch_amd.engine import build_optimizer  # noqa: E402

assert torch.cuda.is_available(), "a timing needs the GPU"


def med(v):
    return sorted(v)[len(v) // 2]


def reference_method(scores, W, onehot, img_off, tau):
    """the reference's per-iteration cost, restated: six blocking copies to the host per image, then its host loop"""
    t0 = time.perf_counter()
    counts = [0, 0, 0]
    for i in range(len(img_off) - 1):
        s, w = scores[img_off[i]: img_off[i + 1]], W[img_off[i]: img_off[i + 1]]
        w_pos, w_neg = torch.clamp(w, min=0), torch.clamp(-w, min=0)
        label = onehot[i: i + 1].cpu().numpy()[0]
        pred = torch.clamp(s.sum(0, keepdim=True), 1e-6, 1 - 1e-6).cpu().numpy()[0]
        (s * w_pos).sum(0, keepdim=True).clamp(1e-20, 1.0).cpu().numpy()
        (s * w_neg).sum(0, keepdim=True).clamp(1e-20, 1.0).cpu().numpy()
        val = w_pos.cpu().numpy() - w_neg.cpu().numpy()
        for c in range(val.shape[1]):
            if label[c] <= 0.5 or pred[c] < tau:
                continue
            for r in range(val.shape[0]):
                if val[r, c] > 0:
                    counts[0] += 1
                elif val[r, c] < 0:
                    counts[1] += 1
                else:
                    counts[2] += 1
    return (time.perf_counter() - t0) * 1e3, counts


def bench(N):
    ocfg = O.OracleCfg(arch="wsr18", out_feature="res5", res5_dilation=1, res2_out=64, dan_dim=(4096, 4096), num_classes=20,
                       heads="csc", refine_num=0, refine_reg=(), mean_loss=False, base_lr=0.0)
    batch = O.synthetic_batch(N, args.R, ocfg, seed=3, H=args.H, W=args.W)
    for i, b in enumerate(batch):
        b["gt_classes"] = (torch.arange(args.classes) + i * args.classes) % 20
    cfg, model = G.drn_model(ocfg, 3, "cuda", 5, args.precision)
    model.train()
    heads = model.roi_heads
    heads.tau = 0.0
    heads.enable_image_batches(N > 1)
    opt = build_optimizer(cfg, model)
    inputs = G.drn_inputs(batch)
    stats = heads.enable_csc_stats(period=320, start_iter=1)
    heads.disable_csc_stats()
    eng = heads._engine

    def step(on):
        eng.csc_stats = stats if on else None
        heads.iter = 1
        opt.zero_grad()
        losses = model(inputs)
        if not model.backward_losses(1.0):
            sum(losses.values()).backward()
        opt.step()

    forms = (("off", False), ("on", True), ("off again", False))
    for _, on in forms * 3:
        step(on)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rounds = max(11, args.rounds)
    times = {name: [] for name, _ in forms}
    for _ in range(rounds):
        for name, on in forms:
            e0.record()
            step(on)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    # the kernel alone, on the tensors of the last step
    aux = heads._last_state["aux"]
    sched = heads._csc_sched
    dev = aux["scores"].device
    slots = sched.d_slot_rows if isinstance(sched, ops.CscBatchPlan) else torch.tensor(sched, dtype=torch.int64, device=dev)
    K = heads.num_classes
    onehot = torch.zeros((N, K), device=dev)
    for i, b in enumerate(batch):
        onehot[i, b["gt_classes"]] = 1.0
    off_host = [0]
    for b in batch:
        off_host.append(off_host[-1] + len(b["proposal_boxes"]))
    img_off = torch.tensor(off_host, dtype=torch.int32, device=dev)
    table = torch.zeros((ops.csc_stats_words(K),), dtype=torch.int64, device=dev)
    scratch = torch.empty((ops.csc_stats_scratch_words(N, K),), dtype=torch.int64, device=dev)
    call = lambda: ops.csc_stats(aux["scores"], aux["W"], img_off, N, onehot, slots, table, scratch)  # noqa: E731
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    ktimes = []
    for _ in range(rounds):
        e0.record()
        for _ in range(args.reps):
            call()
        e1.record()
        e1.synchronize()
        ktimes.append(e0.elapsed_time(e1) / args.reps * 1e3)
    reference_method(aux["scores"], aux["W"], onehot, off_host, heads.tau)
    rtimes = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        rtimes.append(reference_method(aux["scores"], aux["W"], onehot, off_host, heads.tau)[0])
    m = {k: med(v) for k, v in times.items()}
    lines = ["csc_stats_bench --images %d --precision %s: csc_WSR_18_DC5, image %dx%d, R=%d per image, K=20, %d labelled classes "
             "per image, all active (tau = 0), %s" % (N, args.precision, args.H, args.W, args.R, args.classes,
                                                      torch.cuda.get_device_name(0)),
             "  drn_csc_stats alone (both launches, %d back-to-back calls per window, HIP events): median %.2f us per call "
             "[%.2f .. %.2f] over %d windows" % (args.reps, med(ktimes), min(ktimes), max(ktimes), rounds),
             "  eager step, medians of %d alternating rounds (HIP events), ms; [min .. max]" % rounds]
    for name, _ in forms:
        lines.append("    %-10s %8.3f   [%.3f .. %.3f]" % (name, m[name], min(times[name]), max(times[name])))
    lines += ["    on - off = %+.3f ms (%+.2f %%); off again - off = %+.3f ms (%+.2f %%): the spread of two identical forms" % (
                  m["on"] - m["off"], 100 * (m["on"] - m["off"]) / m["off"], m["off again"] - m["off"],
                  100 * (m["off again"] - m["off"]) / m["off"]),
              "  the reference's method on the same tensors (six blocking copies per image + its Python loop, host clock): median "
              "%.3f ms per step [%.3f .. %.3f]" % (med(rtimes), min(rtimes), max(rtimes))]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


for n in [int(x) for x in args.images.split(",")]:
    bench(n)
    torch.cuda.empty_cache()
