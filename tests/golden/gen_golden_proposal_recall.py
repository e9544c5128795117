"""Golden vectors of the box-proposal recall evaluator, from the UNMODIFIED reference function (build container only).

    cd <repo> && python tests/golden/gen_golden_proposal_recall.py          # writes tests/golden/proposal_recall.npz
    cd <repo> && python tests/golden/gen_golden_proposal_recall.py --time   # times it on tools/proposal_recall_bench.py's input

The reference's _evaluate_box_proposals (detectron2/evaluation/coco_evaluation.py:372-480) is imported through ref_harness
- whose list of real modules under stubbed packages is extended here, at run time - and called with a duck-typed coco_api
(getAnnIds / loadAnns) and the reference's own Instances / Boxes.  Nothing of the reference is stored: the file holds the
inputs and, per (case, area, limit), gt_overlaps, recalls, ar and num_pos (layout: tests/proposal_recall_util.py).  The numpy
restatement in tests/proposal_recall_util.py is asserted equal to the reference bit for bit on every one of them.

Cases (fixed seeds; logits are distinct inside every case):
  ties   9 images with 0 .. 70 boxes and 0 .. 90 proposals: box corners on a 16-px grid, sides from {8 .. 768} (areas hit
         32^2 and 96^2 exactly and reach every one of the eight ranges), proposals derived from boxes by halving a side
         (IoU exactly 0.5), three-quartering one (0.75), exact copy (1.0), integer jitter, or at random; ~15 % crowd; an image
         without boxes, one without proposals, two with fewer proposals than boxes
  wide   one image with 70 boxes, none of them crowd, and 90 proposals (beyond one wave)
  plain  6 images with non-dyadic float32 boxes and annotation areas that are not w * h
Limits {1, 4, 20, 64, None} x all eight area names.  The file is written with fixed zip timestamps."""
import argparse
import io
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import proposal_recall_util as U  # noqa: E402

SEEDS = {"ties": 3, "wide": 4, "plain": 9}
SIDES = [8., 16., 32., 48., 96., 128., 256., 512., 768.]


def reference_function():
    import ref_harness

    ref_harness.REAL_UNDER_STUB = tuple(ref_harness.REAL_UNDER_STUB) + (
        "detectron2.evaluation.coco_evaluation", "detectron2.evaluation.evaluator", "detectron2.evaluation.fast_eval_api")
    ref_harness.install()
    from detectron2.evaluation.coco_evaluation import _evaluate_box_proposals
    from detectron2.structures import Boxes, Instances

    return _evaluate_box_proposals, Boxes, Instances


class CocoApi:
    """what _evaluate_box_proposals asks of pycocotools' COCO: an image's annotation ids, and the annotations of ids"""

    def __init__(self, case):
        self.anns = {q + 1: {"bbox": [float(v) for v in case["gt_box"][q]], "area": float(case["gt_area"][q]),
                             "iscrowd": int(case["gt_crowd"][q])} for q in range(len(case["gt_img"]))}
        self.by_img = {int(i): [q + 1 for q in np.nonzero(case["gt_img"] == i)[0]] for i in case["img_ids"]}

    def getAnnIds(self, imgIds):
        return list(self.by_img[int(imgIds)])

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]


def predictions_of(case, Boxes, Instances):
    import torch

    out = []
    for iid in case["img_ids"]:
        sel = np.nonzero(case["pr_img"] == iid)[0]
        p = Instances((2000, 2000))
        p.proposal_boxes = Boxes(torch.from_numpy(case["pr_box"][sel].reshape(-1, 4).copy()))
        p.objectness_logits = torch.from_numpy(case["pr_logit"][sel].copy())
        out.append({"image_id": int(iid), "proposals": p})
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------

def grid_image(rng, ng, npr, crowd=0.15):
    side = rng.choice(SIDES, (ng, 2))
    gb = np.concatenate([rng.integers(0, 40, (ng, 2)) * 16., side], 1)  # XYWH
    if ng:
        src = gb[rng.integers(0, ng, npr)].copy()
        m = rng.integers(0, 5, npr)
        src[m == 0, 2] *= 0.5   # IoU exactly 0.5
        src[m == 1, 3] *= 0.75  # IoU exactly 0.75
        src[m == 3] += rng.integers(-8, 9, (int((m == 3).sum()), 4))  # (m == 2: exact copy)
        rnd = np.concatenate([rng.integers(0, 40, (npr, 2)) * 16., rng.choice(SIDES, (npr, 2))], 1)
        src[m == 4] = rnd[m == 4]
        src[:, 2:] = np.maximum(src[:, 2:], 1)
    else:
        src = np.concatenate([rng.integers(0, 40, (npr, 2)) * 16., rng.choice(SIDES, (npr, 2))], 1)
    pb = np.stack([src[:, 0], src[:, 1], src[:, 0] + src[:, 2], src[:, 1] + src[:, 3]], 1)
    return gb, gb[:, 2] * gb[:, 3], rng.random(ng) < crowd, pb


def plain_image(rng, ng, npr):
    gb = np.concatenate([rng.uniform(0, 500, (ng, 2)), rng.uniform(6, 600, (ng, 2))], 1)
    area = gb[:, 2] * gb[:, 3] * rng.uniform(0.4, 1.0, ng)
    pb = []
    for _ in range(npr):
        if ng and rng.random() < 0.7:
            b = gb[rng.integers(0, ng)] * (1 + rng.normal(0, 0.07, 4))
        else:
            b = np.concatenate([rng.uniform(0, 500, 2), rng.uniform(6, 600, 2)])
        pb.append([b[0], b[1], b[0] + max(b[2], 1), b[1] + max(b[3], 1)])
    return gb, area, rng.random(ng) < 0.15, np.array(pb, np.float64).reshape(-1, 4)


def make_case(rng, img_ids, sizes, image_fn):
    gi, gb, ga, gc, pi, pb = [], [], [], [], [], []
    for iid, (ng, npr) in zip(img_ids, sizes):
        b, a, c, p = image_fn(rng, ng, npr)
        gi += [iid] * ng
        gb.append(b), ga.append(a), gc.append(c)
        pi += [iid] * npr
        pb.append(p)
    n = len(pi)
    logit = (rng.permutation(n) - n / 2) / 8  # distinct
    return dict(img_ids=np.array(img_ids, np.int64), gt_img=np.array(gi, np.int64),
                gt_box=np.concatenate(gb).astype(np.float64).reshape(-1, 4), gt_area=np.concatenate(ga).astype(np.float64),
                gt_crowd=np.concatenate(gc).astype(np.uint8), pr_img=np.array(pi, np.int64),
                pr_box=np.concatenate(pb).astype(np.float32).reshape(-1, 4), pr_logit=logit.astype(np.float32))


def make_cases():
    return {
        "ties": make_case(np.random.default_rng(SEEDS["ties"]), [101, 7, 55, 1030, 12, 900, 77, 3, 41],
                          [(0, 8), (4, 20), (9, 0), (25, 60), (70, 90), (3, 2), (12, 30), (40, 25), (6, 14)], grid_image),
        "wide": make_case(np.random.default_rng(SEEDS["wide"]), [5], [(70, 90)],
                          lambda rng, ng, npr: grid_image(rng, ng, npr, crowd=0.0)),
        "plain": make_case(np.random.default_rng(SEEDS["plain"]), [9, 2, 30, 4, 17, 8],
                           [(5, 40), (11, 70), (2, 9), (7, 3), (1, 25), (16, 50)], plain_image),
    }


def check_ties(res):
    """the non-degeneracy conditions, on the reference's results alone (tests/test_proposal_recall_cpu.py re-checks them
    on the file); res[(area, limit)] = the reference's dict as numpy"""
    top = res[("all", None)]
    ov = top["gt_overlaps"]
    n = {v: int((ov == np.float32(v)).sum()) for v in (0.0, 0.5, 0.75, 1.0)}
    msg = "ties: AR(all, no limit) %.3f, entries %d, == 0.5: %d, == 0.75: %d, == 1.0: %d, zeros: %d" % (
        float(top["ar"]), len(ov), n[0.5], n[0.75], n[1.0], n[0.0])
    print(msg)
    assert 0.15 <= float(top["ar"]) <= 0.85, msg
    assert n[0.5] >= 5 and n[0.75] >= 5 and n[1.0] >= 5, msg
    assert n[0.0] >= 1, msg  # (images with fewer proposals than boxes; the test checks that this is the cause)
    parts = sum(res[(a, None)]["num_pos"] for a in ("small", "medium", "large"))
    assert parts > top["num_pos"], (parts, top["num_pos"])  # the inclusive boundaries
    for a in U.AREA_NAMES:
        assert res[(a, None)]["num_pos"] > 0, a


def save_fixed(path, arrays):
    """np.savez_compressed with constant zip timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="time the reference on the bench tool's VOC07-trainval-sized input")
    ap.add_argument("--images", type=int, default=5011)
    args = ap.parse_args()
    ref, Boxes, Instances = reference_function()
    if args.time:
        from proposal_recall_bench import make_input

        case = make_input(images=args.images)
        preds, api = predictions_of(case, Boxes, Instances), CocoApi(case)
        t0 = time.perf_counter()
        ars = {}
        for limit in (100, 1000):
            for area in ("all", "small", "medium", "large"):
                ars[(area, limit)] = float(ref(preds, api, area=area, limit=limit)["ar"])
        dt = time.perf_counter() - t0
        print("reference _evaluate_box_proposals (unmodified, torch on the CPU), %d images x %d proposals, %d boxes, 8 pairs: "
              "%.1f s (%.2f ms per image and pair; one run); AR@100 %.4f AR@1000 %.4f"
              % (len(case["img_ids"]), len(case["pr_img"]) // len(case["img_ids"]), len(case["gt_img"]), dt,
                 dt * 1e3 / (8 * len(case["img_ids"])), 100 * ars[("all", 100)], 100 * ars[("all", 1000)]))
        return
    out = {}
    for name, case in make_cases().items():
        assert len(np.unique(case["pr_logit"])) == len(case["pr_logit"]), name
        preds, api = predictions_of(case, Boxes, Instances), CocoApi(case)
        res, ov, off = {}, [], [0]
        A, L = len(U.AREA_NAMES), len(U.LIMITS)
        recalls, ar, num_pos = np.zeros((A, L, 10), np.float32), np.zeros((A, L), np.float32), np.zeros((A, L), np.int64)
        for a, area in enumerate(U.AREA_NAMES):
            for l, limit in enumerate(U.LIMITS):
                r = ref(preds, api, area=area, limit=limit)
                r = dict(gt_overlaps=r["gt_overlaps"].numpy(), recalls=r["recalls"].numpy(), ar=r["ar"].numpy(),
                         num_pos=int(r["num_pos"]))
                mine = U.evaluate_numpy(case, area, limit)
                for k in ("gt_overlaps", "recalls", "ar"):  # the numpy restatement, bit for bit
                    assert np.array_equal(r[k], mine[k], equal_nan=True) and r[k].dtype == mine[k].dtype, (name, area, limit, k)
                assert r["num_pos"] == mine["num_pos"], (name, area, limit)
                res[(area, limit)] = r
                ov.append(r["gt_overlaps"])
                off.append(off[-1] + len(r["gt_overlaps"]))
                recalls[a, l], ar[a, l], num_pos[a, l] = r["recalls"], r["ar"], r["num_pos"]
        if name == "ties":
            check_ties(res)
        else:
            print("%s: AR(all, no limit) %.3f, %d entries" % (name, float(res[("all", None)]["ar"]),
                                                             len(res[("all", None)]["gt_overlaps"])))
        for k in U.INPUT_KEYS:
            out["%s_%s" % (name, k)] = case[k]
        out.update({name + "_ov": np.concatenate(ov).astype(np.float32), name + "_ov_off": np.array(off, np.int64),
                    name + "_recalls": recalls, name + "_ar": ar, name + "_num_pos": num_pos})
    path = os.path.join(HERE, "proposal_recall.npz")
    save_fixed(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
