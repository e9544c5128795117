"""The training DatasetMapper's image chain, host against device, on one VOC-sized image (375 x 500, INPUT.CROP on, the recipes'
brightness / saturation blends) at short edges 480 / 800 / 1216.

  python tools/mapper_bench.py
      per-image wall time of the host mapper (numpy + PIL: the parent's code path, DatasetMapper(cfg, True)) and of the device
      mapper's plan() + finish() (pinned upload + ONE launch of drn_augment_u8, ending in the item's event synchronise) in one
      process, the two alternating on the same seeds: median, min .. max over MAPPER_REPS draws, and the ratio.

  rocprofv3 --kernel-trace --stats -d DIR -- python tools/mapper_bench.py --kernels all|resize
  python tools/prof_summary.py DIR
      kernel times (a run of its own): drn_augment_u8 at the three shapes with every stage on (`all`) or as a plain resize
      (`resize`), and the per-pixel resize_u8_kernel of drn_resize_bilinear_u8 at the same resize in the same run; the summary
      splits rows by (kernel, grid), i.e. by shape.  Prints the bytes each launch moves."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from __graft_entry__ import load_package

pkg = load_package()
from drn_wsod_pytorch_amd import data as D
from drn_wsod_pytorch_amd import ops
from drn_wsod_pytorch_amd.config import add_wsl_config, get_cfg
from drn_wsod_pytorch_amd.modeling.tta import resize_shortest_edge_shape

H, W = 375, 500
SIZES = (480, 800, 1216)
REPS = int(os.environ.get("MAPPER_REPS", "15"))


def image():
    return np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)


def wall():
    img = image()
    rec = {"image_array": img, "height": H, "width": W, "image_id": 0}
    for size in SIZES:
        cfg = get_cfg()
        add_wsl_config(cfg)
        cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", "(%d,)" % size, "INPUT.MAX_SIZE_TRAIN", "4000", "INPUT.CROP.ENABLED", "True",
                             "MODEL.LOAD_PROPOSALS", "False"])
        host, dev = D.DatasetMapper(cfg, True), D.DatasetMapper(cfg, True, device="cuda")
        t = {"host": [], "device": [], "plan": []}
        for rep in range(-3, REPS):  # (three warm-up draws: tables, pinned buffers, the stream)
            np.random.seed(100 + rep)
            t0 = time.perf_counter()
            a = host(rec)["image"]
            t1 = time.perf_counter()
            np.random.seed(100 + rep)
            t2 = time.perf_counter()
            p = dev.plan(rec)
            t3 = time.perf_counter()
            b = dev.finish(p)["image"]  # (ends in the item's event synchronise)
            t4 = time.perf_counter()
            if rep >= 0:
                t["host"].append(t1 - t0), t["device"].append(t4 - t2), t["plan"].append(t3 - t2)
            if rep == 0:
                differ = int((a.float() != b.cpu()).sum())
        ms = {k: np.array(v) * 1e3 for k, v in t.items()}
        print("short edge %4d (%d x %d, %d draws): host %.2f ms [%.2f .. %.2f]   device plan + finish %.3f ms [%.3f .. %.3f] (plan %.3f)   "
              "host / device %.1fx   bytes that differ on draw 0: %d of %d" % (
                  size, a.shape[1], a.shape[2], REPS, np.median(ms["host"]), ms["host"].min(), ms["host"].max(),
                  np.median(ms["device"]), ms["device"].min(), ms["device"].max(), np.median(ms["plan"]),
                  np.median(ms["host"]) / np.median(ms["device"]), differ, a.numel()), flush=True)


def kernels(mode):
    src = torch.from_numpy(image()).cuda()
    n = 20
    for size in SIZES:
        nh, nw = resize_shortest_edge_shape(H, W, size, 4000)
        moved = H * W * 3 + nh * nw * 3 * 4
        print("short edge %d: %d x %d -> %d x %d, %.2f MB moved per launch (source bytes once + fp32 planes)" % (
            size, H, W, nh, nw, moved / 1e6), flush=True)
        for _ in range(n):
            if mode == "all":
                ops.augment_u8(src, None, (nh, nw), True, 1.2, 0.8)
            else:
                ops.augment_u8(src, None, (nh, nw))
        for _ in range(n):
            ops.resize_bilinear_u8(src, nh, nw)
        torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels" and sys.argv[2] in ("all", "resize"):
        kernels(sys.argv[2])
    elif len(sys.argv) == 1:
        wall()
    else:
        sys.exit(__doc__)
