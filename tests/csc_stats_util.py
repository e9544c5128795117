"""The CSC weight statistics restated in numpy (fp64 / int64), for tests/test_csc_stats_{cpu,gpu}.py and the model-level test:
the table drn_csc_stats accumulates (include/drn_wsod.h, "CSC weight statistics"), from the definition in the header and in
the issue's words - not from the kernel.  `active` is handed in, as it is handed to the kernel.  No device code, no oracle."""
import numpy as np

INT_FIELDS = ("ori_label", "ori_num_roi", "csc_label", "csc_num_roi", "csc_roi_pos", "csc_roi_neg", "csc_roi_zero")
FP_FIELDS = ("ori_pred", "csc_pred", "csc_pred_pos", "csc_pred_neg")
F32 = np.float32
PRED_LO, PRED_HI = float(F32(1e-6)), float(F32(1.0 - 1e-6))  # torch.clamp on an fp32 tensor casts its bounds to fp32
W_LO, W_HI = float(F32(1e-20)), 1.0                          # (1.0 - 1e-20 IS 1.0)


def new_table(K):
    """zeros; bound_<fp field>: the sum over the contributions of one fp32 spacing each (what a device table may differ by)"""
    t = {"steps": 0, "num_img": 0}
    for f in INT_FIELDS:
        t[f] = np.zeros(K, np.int64)
    for f in FP_FIELDS:
        t[f] = np.zeros(K, np.float64)
        t["bound_" + f] = np.zeros(K, np.float64)
    return t


def _colsum(x):
    """fp64, ascending row order"""
    acc = 0.0
    for v in x:
        acc = acc + float(v)
    return acc


def _clamp(v, lo, hi, round32):
    if round32:
        v = float(F32(v))
    if v != v:
        return v
    return lo if v < lo else hi if v > hi else v


def add_step(t, scores, W, img_off, onehot, active, round32=True, M=None):
    """one launch: scores / W [M, K], img_off [n_img + 1], onehot [n_img, K], active: set of (image, class).  round32=False keeps
    the fp64 row sums unrounded (the value a device sum is compared with, within bound_*)."""
    scores, W = np.asarray(scores, np.float32), np.asarray(W, np.float32)
    onehot = np.asarray(onehot, np.float32).reshape(len(img_off) - 1, -1)
    K = scores.shape[1]
    M = scores.shape[0] if M is None else M
    t["steps"] += 1
    for i in range(len(img_off) - 1):
        o0, o1 = int(img_off[i]), int(img_off[i + 1])
        if o0 < 0 or o1 > M or o1 <= o0:
            continue  # skipped whole
        R = o1 - o0
        t["num_img"] += 1
        for c in range(K):
            if not onehot[i, c] > 0.5:
                continue
            s, w = scores[o0:o1, c].astype(np.float64), W[o0:o1, c].astype(np.float64)
            pred = _clamp(_colsum(s), PRED_LO, PRED_HI, round32)
            t["ori_label"][c] += 1
            t["ori_num_roi"][c] += R
            t["ori_pred"][c] += pred
            t["bound_ori_pred"][c] += float(np.spacing(F32(abs(pred))))
            if (i, c) not in active:
                continue
            wp = np.where(w > 0, w, 0.0)   # max(W, 0): -0.0 and NaN give 0
            wn = np.where(w < 0, -w, 0.0)  # max(-W, 0)
            pos = _clamp(_colsum(s * wp), W_LO, W_HI, round32)
            neg = _clamp(_colsum(s * wn), W_LO, W_HI, round32)
            t["csc_label"][c] += 1
            t["csc_num_roi"][c] += R
            npos, nneg = int((w > 0).sum()), int((w < 0).sum())
            t["csc_roi_pos"][c] += npos
            t["csc_roi_neg"][c] += nneg
            t["csc_roi_zero"][c] += R - npos - nneg
            for f, v in (("csc_pred", pred), ("csc_pred_pos", pos), ("csc_pred_neg", neg)):
                t[f][c] += v
                t["bound_" + f][c] += float(np.spacing(F32(abs(v))))
    return t


def to_words(t):
    """the table as the int64 words of include/drn_wsod.h: steps, num_img, the int fields [K], the fp64 fields [K] (their bits)"""
    return np.concatenate([np.array([t["steps"], t["num_img"]], np.int64)] + [t[f] for f in INT_FIELDS] +
                          [t[f].view(np.int64) for f in FP_FIELDS])


def active_of(scores, img_off, onehot, tau):
    """the reference's rule on exact inputs (cpg_stats.py:71): labelled and clamped fp32 image score >= tau"""
    act = set()
    for i in range(len(img_off) - 1):
        col = np.asarray(scores, np.float32)[int(img_off[i]): int(img_off[i + 1])].astype(np.float64).sum(axis=0)
        for c in range(col.shape[0]):
            if onehot[i, c] > 0.5 and _clamp(col[c], PRED_LO, PRED_HI, True) >= tau:
                act.add((i, c))
    return act


def add_tables(a, b):
    out = {}
    for k, v in a.items():
        out[k] = v + b[k]
    return out


def assert_close(dev, ref, what=""):
    """dev: metrics.decode_csc_stats' dict; ref: a table of add_step(round32=False).  Integer fields exact, every fp sum within
    the summed one-fp32-spacing-per-contribution bound."""
    assert dev["steps"] == ref["steps"] and dev["num_img"] == ref["num_img"], (what, dev["steps"], dev["num_img"], ref["steps"], ref["num_img"])
    for f in INT_FIELDS:
        assert np.array_equal(dev[f], ref[f]), (what, f, dev[f], ref[f])
    for f in FP_FIELDS:
        err = np.abs(dev[f] - ref[f])
        print(what, f, "max err %.3g, bound at it %.3g" % (err.max(), ref["bound_" + f][err.argmax()]))
        assert np.all(err <= ref["bound_" + f]), (what, f, dev[f], ref[f], ref["bound_" + f])
