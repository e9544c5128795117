"""Golden csc.txt blocks of the UNMODIFIED reference `Statistic` (build container only).

    cd <repo> && python tests/golden/gen_golden_csc_stats.py

Imports projects/WSL/wsl/modeling/roi_heads/third_party/cpg_stats.py as it is, replaces only `setup_logger` in that module's
namespace by a collector (before a Statistic is constructed), and feeds it a recorded sequence of steps the way
CSCOutputs.csc_loss does (fast_rcnn.py:897-918): PL, predict_probs_img(), the two clamped weighted sums, W_pos, W_neg - fp32,
shapes [1, K] / [R, K] - then LogIterStats().  A step of n images is n UpdateIterStats calls in ascending image order and one
LogIterStats (this package's definition of the statistics on an image batch).  Stored: the inputs of every step and every emitted
`info_all` block with its iteration.  Data only: numbers and the emitted text, no reference source.

The reference's accumulation width depends on its NumPy (0.0 + np.float32 stays fp32 under NumPy >= 2, is fp64 before), so every
score and weight is a small dyadic rational: scores multiples of 2^-6, weights multiples of 2^-4, hence every product and every
sum a multiple of 2^-10 below 2^10 - exact in fp32 and fp64 and in any order.  The generator asserts that of its own inputs.

The sequence (K = 4, LOG_PERIOD = 4 through num_gpus = 320, max_iter = 9, tau = 0.7, 14 steps) covers: class 0 never labelled;
class 1 labelled but below tau in some steps and above in others; class 2 active with only zero weights (+0.0 and -0.0); class 3
mixed signs; blocks at iterations 0, 4 and 8 with a reset between them; a first block of one step; iterations 12 and 13 past
max_iter (no block); steps of two images with unequal row counts; an image with no labelled class."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

NAME = "csc_stats"
K, TAU, NUM_GPUS, MAX_ITER, STEPS, SEED = 4, 0.7, 320, 9, 14, 7


class _Collector:
    def __init__(self):
        self.blocks = []

    def info(self, text):
        self.blocks.append(text)


def make_steps(rng):
    steps = []
    for it in range(STEPS):
        n_img = 2 if it in (2, 5, 9) else 1
        rows = [int(rng.integers(3, 8)) for _ in range(n_img)]
        img_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
        M = int(img_off[-1])
        scores = np.zeros((M, K), np.float32)
        W = np.zeros((M, K), np.float32)
        onehot = np.zeros((n_img, K), np.float32)
        for i in range(n_img):
            o0, o1 = int(img_off[i]), int(img_off[i + 1])
            R = o1 - o0
            empty = it == 5 and i == 1  # an image with no labelled class
            for c in range(K):
                # column sums in 1/64 units: class 1 alternates below / above tau, the others sit above it
                total = {0: 40, 1: 30 if (it + i) % 2 == 0 else 50, 2: 48, 3: 58}[c]
                cut = np.sort(rng.integers(0, total + 1, size=R - 1))
                parts = np.diff(np.concatenate([[0], cut, [total]]))
                scores[o0:o1, c] = parts / 64.0
                if c == 2:
                    W[o0:o1, c] = np.where(np.arange(R) % 2 == 0, 0.0, -0.0)
                else:
                    W[o0:o1, c] = rng.integers(-16, 17, size=R) / 16.0
            if not empty:
                onehot[i, 1:] = 1.0
                if it % 3 == 1:
                    onehot[i, 3] = 0.0
        steps.append(dict(scores=scores, W=W, img_off=img_off, onehot=onehot))
    return steps


def check_dyadic(steps):
    for s in steps:
        for a, unit in ((s["scores"], 64.0), (s["W"], 16.0)):
            assert a.dtype == np.float32 and np.array_equal(a * unit, np.round(a * unit))
        prod = s["scores"].astype(np.float64) * np.abs(s["W"]).astype(np.float64)
        for a in (s["scores"].astype(np.float64), prod):
            assert np.array_equal(a * 1024.0, np.round(a * 1024.0)) and a.sum() < 1024.0


def main():
    import ref_harness as rh

    rh.install()
    import wsl.modeling.roi_heads.third_party.cpg_stats as S

    col = _Collector()
    S.setup_logger = lambda output=None, name=None: col  # the ONE replacement; the class below is the reference's own
    stat = S.Statistic(MAX_ITER, TAU, NUM_GPUS, K, "/nonexistent", "")
    assert stat.LOG_PERIOD == 4
    steps = make_steps(np.random.default_rng(SEED))
    check_dyadic(steps)
    d = {"K": np.int64(K), "tau": np.float64(TAU), "period": np.int64(stat.LOG_PERIOD), "max_iter": np.int64(MAX_ITER),
         "steps": np.int64(STEPS), "numpy": np.array(np.__version__)}
    iters = []
    for it, s in enumerate(steps):
        for i in range(len(s["img_off"]) - 1):
            sc = s["scores"][s["img_off"][i]: s["img_off"][i + 1]]
            w = s["W"][s["img_off"][i]: s["img_off"][i + 1]]
            w_pos, w_neg = np.maximum(w, np.float32(0)), np.maximum(-w, np.float32(0))
            pred = np.clip(sc.sum(axis=0, keepdims=True, dtype=np.float32), np.float32(1e-6), np.float32(1.0 - 1e-6))
            pos = np.clip((sc * w_pos).sum(axis=0, keepdims=True, dtype=np.float32), np.float32(1e-20), np.float32(1.0))
            neg = np.clip((sc * w_neg).sum(axis=0, keepdims=True, dtype=np.float32), np.float32(1e-20), np.float32(1.0))
            stat.UpdateIterStats(s["onehot"][i: i + 1], pred, pos, neg, w_pos, w_neg)
        n = len(col.blocks)
        stat.LogIterStats()
        if len(col.blocks) > n:
            iters.append(it)
        for k, v in s.items():
            d["step%d_%s" % (it, k)] = v
    assert iters == [0, 4, 8], iters
    d["block_iters"] = np.array(iters, np.int64)
    d["blocks"] = np.array(col.blocks)
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes; numpy", np.__version__)
    for b in col.blocks:
        print(b)


if __name__ == "__main__":
    main()
