"""RoIPool / ROIAlign backward: the atomic scatter (drn_roi_pool_backward_nhwc) against the order-fixed, atomic-free form
(drn_roi_pool_backward_det_nhwc), through the same ops call in one process.  Per shape: a warm-up, then N alternating A/B
launches each timed with its own pair of HIP events (median and min reported); the deterministic results of all launches
must be bit-identical, else the timing is aborted.  Bytes = the pooled gradient read once (+ the arg-max for RoIPool) + the
fp32 map gradient written once + rois, against the 8 TB/s HBM roof.
  python tools/roi_bwd_bench.py [--launches 50] [--out profiles/roi_bwd_det.txt]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from __graft_entry__ import load_package

HBM_GBS = 8000.0
R = 2000
# (label, mode, H, W, C, stride, dtype)
SHAPES = [("ROIAlign 14x14x1024", 1, 14, 14, 1024, 16, torch.bfloat16),
          ("RoIPool 14x14x1024", 0, 14, 14, 1024, 16, torch.bfloat16),
          ("RoIPool 60x80x512 (CSC, WS-R18 DC5)", 0, 60, 80, 512, 8, torch.float32),
          ("RoIPool 50x76x1024", 0, 50, 76, 1024, 16, torch.bfloat16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.launches >= 50, "at least 50 launches per form"
    assert torch.cuda.is_available(), "this measurement needs the GPU (no fallback)"
    load_package()
    ops = importlib.import_module("drn_wsod_pytorch_amd.ops")
    dev = "cuda"
    lines = ["%-38s %-5s %12s %12s %12s %12s %8s %9s %9s" % ("shape (R = %d)" % R, "dtype", "atomic us", "(min)", "det us", "(min)",
                                                              "det/atm", "MB moved", "det roof")]
    for label, mode, H, W, C, stride, dt in SHAPES:
        rs = np.random.RandomState(0)
        iw, ih = W * stride, H * stride
        x0, y0 = rs.rand(R) * (iw - 40), rs.rand(R) * (ih - 40)
        rois = np.stack([np.zeros(R), x0, y0, x0 + 20 + rs.rand(R) * (iw - x0 - 20), y0 + 20 + rs.rand(R) * (ih - y0 - 20)], 1)
        rois = torch.from_numpy(rois.astype(np.float32)).to(dev)
        obj = torch.rand(R, device=dev)
        es = 2 if dt == torch.bfloat16 else 4
        K = C * 49
        g = (torch.randn((R, ops.kpad(K, dt)), device=dev) * 0.1).to(dt)
        arg, ka = None, dict(mode=1, sampling_ratio=0, aligned=True)
        if mode == 0:
            feat = (torch.randn((1, H, W, C), device=dev).relu() * 0.5).to(dt)
            arg, ka = ops.roi_pool_nhwc(feat, rois, obj, 7, 1.0 / stride, want_argmax=True)[1], {}
            del feat
        nbytes = R * K * es + (R * K * 4 if mode == 0 else 0) + H * W * C * 4 + R * 20
        outs = {False: torch.empty((1, H, W, C), device=dev), True: torch.empty((1, H, W, C), device=dev)}

        def run(det):
            return ops.roi_pool_backward_nhwc(g, rois, obj, (1, H, W, C), 7, 1.0 / stride, argmax=arg, deterministic=det,
                                              out=outs[det], **ka)

        for _ in range(3):
            run(False)
            run(True)
        torch.cuda.synchronize()
        first = outs[True].clone()
        atomic = outs[False].clone()
        err = float((first - atomic).abs().max()) / max(float(atomic.abs().max()), 1e-30)
        assert err <= 1e-4, "the two forms disagree beyond a reordered fp32 sum: %g" % err
        ev = {False: [], True: []}
        for _ in range(args.launches):
            for det in (False, True):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(det)
                b.record()
                ev[det].append((a, b))
                if det and not torch.equal(outs[True].view(torch.int32), first.view(torch.int32)):
                    raise SystemExit("ABORT: the deterministic form changed its bits between launches (%s)" % label)
        torch.cuda.synchronize()
        t = {k: np.array([a.elapsed_time(b) * 1e3 for a, b in v]) for k, v in ev.items()}
        ta, td = float(np.median(t[False])), float(np.median(t[True]))
        lines.append("%-38s %-5s %12.1f %12.1f %12.1f %12.1f %8.2f %9.1f %9.4f" % (
            label, "bf16" if es == 2 else "fp32", ta, float(t[False].min()), td, float(t[True].min()), td / ta, nbytes / 1e6,
            nbytes / td / 1e3 / HBM_GBS))
        print(lines[-1], flush=True)
        del g, arg, outs
        torch.cuda.empty_cache()
    lines.append("times: median (min) of %d alternating launches, one HIP event pair per launch; det results bit-identical across"
                 " all launches; the two forms agree to a reordered fp32 sum" % args.launches)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
