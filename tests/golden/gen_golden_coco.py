"""Golden vectors of the COCO box-AP evaluator, from the UNMODIFIED reference C++ (build container only).

    cd <repo> && python tests/golden/gen_golden_coco.py            # writes tests/golden/coco_eval.npz
    cd <repo> && python tests/golden/gen_golden_coco.py --time     # times the C++ on tools/coco_eval_bench.py's input

The reference's native component detectron2/layers/csrc/cocoeval/cocoeval.cpp (EvaluateImages, Accumulate) is compiled
where it lies, against a small pybind11 binding that this script writes into a temporary directory; nothing compiled and
no reference text is stored.  The IoUs it is fed come from the restated pycocotools bbIou (tests/coco_eval_util.py), the
detections from the conversion COCOEvaluator applies (coco_evaluation.py:308-370).

Cases (fixed seeds; flat inputs and per-(image, category) results, see tests/coco_eval_util.py for the layout):
  ties   7 images x 5 categories: boxes on a 16-px grid with sides from {8, 16, 32, 48, 96, 128} (areas hit 32^2 and 96^2
         exactly), detections derived from GT by halving / three-quartering a side (IoU exactly 0.5 / 0.75) or integer
         jitter, scores k / 8, ~20 % crowd; empty pairs, a category without GT, a category without detections, an image
         without detections, non-contiguous dataset category ids and image ids
  wide   4 x 3 with one pair of 130 detections and 70 GT (beyond maxDets and beyond one wave)
  plain  12 x 4 with non-dyadic float32 boxes and scores, GT areas that are not w * h
The file is written with fixed zip timestamps, so a second run reproduces it byte for byte."""
import argparse
import importlib.util
import io
import os
import subprocess
import sys
import sysconfig
import tempfile
import time
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import coco_eval_util as U  # noqa: E402

REF = "/root/reference"
REF_DIR = os.path.join(REF, "detectron2", "layers", "csrc", "cocoeval")

BINDING = """#include "cocoeval.h"
using namespace detectron2::COCOeval;
PYBIND11_MODULE(cocoref, m) {
  m.def("EvaluateImages", &EvaluateImages);
  m.def("Accumulate", &Accumulate);
  pybind11::class_<InstanceAnnotation>(m, "InstanceAnnotation").def(pybind11::init<uint64_t, double, double, bool, bool>());
  pybind11::class_<ImageEvaluation>(m, "ImageEvaluation").def(pybind11::init<>())
      .def_readonly("detection_matches", &ImageEvaluation::detection_matches)
      .def_readonly("detection_scores", &ImageEvaluation::detection_scores)
      .def_readonly("ground_truth_ignores", &ImageEvaluation::ground_truth_ignores)
      .def_readonly("detection_ignores", &ImageEvaluation::detection_ignores);
}
"""


def build_binding(tmp):
    import pybind11

    src = os.path.join(tmp, "bind.cpp")
    with open(src, "w") as f:
        f.write(BINDING)
    so = os.path.join(tmp, "cocoref" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", REF_DIR, "-I", pybind11.get_include(),
                           "-I", sysconfig.get_paths()["include"], src, os.path.join(REF_DIR, "cocoeval.cpp"), "-o", so])
    spec = importlib.util.spec_from_file_location("cocoref", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_inputs(C, case):
    """the three nested lists COCOeval_opt hands to the C++ (cocoeval.cpp:141-149)"""
    I, K, pairs = U.prepare(case)
    gid, gts, dts, ious = 1, [], [], []
    for i in range(I):
        G_, D_, U_ = [], [], []
        for k in range(K):
            gb, garea, cr, db, sc = pairs[i][k]
            o = np.argsort(-sc, kind="mergesort")[:100]  # pycocotools computeIoU: by score, cut at maxDets[-1]
            G_.append([C.InstanceAnnotation(gid + j, 0.0, float(garea[j]), bool(cr[j]), bool(cr[j])) for j in range(len(gb))])
            gid += len(gb)
            D_.append([C.InstanceAnnotation(j + 1, float(sc[j]), float(db[j, 2] * db[j, 3]), False, False)
                       for j in range(len(db))])
            U_.append(U.bb_iou(db[o], gb, cr).tolist() if len(gb) and len(db) else [])
        gts.append(G_), dts.append(D_), ious.append(U_)
    return I, K, gts, dts, ious


def params_of(I, K):
    return types.SimpleNamespace(iouThrs=list(U.IOU_THRS), recThrs=list(U.REC_THRS), maxDets=[int(m) for m in U.MAX_DETS],
                                 areaRng=U.AREA_RNG.tolist(), catIds=list(range(K)), imgIds=list(range(I)), useCats=1)


def run_reference(C, case):
    I, K, gts, dts, ious = reference_inputs(C, case)
    A, T = len(U.AREA_RNG), len(U.IOU_THRS)
    evs = C.EvaluateImages(U.AREA_RNG.tolist(), 100, list(U.IOU_THRS), ious, gts, dts)
    nd_, ng_ = np.zeros((I, K), np.int32), np.zeros((I, K), np.int32)
    S, DM, DI, GI = [], [], [], []
    for i in range(I):
        for k in range(K):
            per = [evs[k * A * I + a * I + i] for a in range(A)]
            sc = np.array(per[0].detection_scores, np.float64)
            nd, ng = len(sc), len(per[0].ground_truth_ignores)
            for e in per:
                assert np.array_equal(np.array(e.detection_scores, np.float64), sc)
            nd_[i, k], ng_[i, k] = nd, ng
            S.append(sc)
            DM.append(np.array([np.array(e.detection_matches, np.uint64).reshape(T, nd) != 0 for e in per], np.uint8).ravel())
            DI.append(np.array([np.array(e.detection_ignores, bool).reshape(T, nd) for e in per], np.uint8).ravel())
            GI.append(np.array([np.array(e.ground_truth_ignores, bool).reshape(ng) for e in per], np.uint8).ravel())
    r = C.Accumulate(params_of(I, K), evs)
    counts = list(r["counts"])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt)
    return dict(nd=nd_, ng=ng_, det_scores=cat(S, np.float64), det_matched=cat(DM, np.uint8), det_ignored=cat(DI, np.uint8),
                gt_ignored=cat(GI, np.uint8), precision=np.array(r["precision"]).reshape(counts),
                recall=np.array(r["recall"]).reshape(counts[:1] + counts[2:]), scores=np.array(r["scores"]).reshape(counts),
                counts=np.array(counts, np.int64))


# ---- the cases ---------------------------------------------------------------------------------------------------------

def grid_case(rng, img_ids, cat_ids, wide=None, no_gt_cat=None, no_dt_cat=None, no_dt_img=None):
    I, K = len(img_ids), len(cat_ids)
    cat_sorted = np.sort(cat_ids)
    gt, dt = [], []
    for i, iid in enumerate(img_ids):
        mine = []
        for k in range(K):
            ng, nd = int(rng.integers(0, 6)), int(rng.integers(0, 14))
            if wide is not None and (i, k) == wide:
                ng, nd = 70, 130
            if k == no_gt_cat:
                ng = 0
            side = rng.choice([8., 16., 32., 48., 96., 128.], (ng, 2))
            gb = np.concatenate([rng.integers(0, 12, (ng, 2)) * 16., side], 1)
            cr = rng.random(ng) < 0.2
            if ng:
                src = gb[rng.integers(0, ng, nd)].copy()
                m = rng.integers(0, 4, nd)
                src[m == 0, 2] *= 0.5   # IoU exactly 0.5
                src[m == 1, 3] *= 0.75  # IoU exactly 0.75
                src[m == 2] += rng.integers(-8, 9, (int((m == 2).sum()), 4))
                src[:, 2:] = np.maximum(src[:, 2:], 1)
            else:
                src = np.concatenate([rng.integers(0, 12, (nd, 2)) * 16., rng.choice([8., 32., 96.], (nd, 2))], 1)
            sc = rng.integers(1, 9, nd) / 8
            for j in range(ng):
                gt.append((iid, cat_sorted[k], gb[j], gb[j, 2] * gb[j, 3], cr[j]))
            if k != no_dt_cat and i != no_dt_img:
                mine += [(iid, k, [src[j, 0], src[j, 1], src[j, 0] + src[j, 2], src[j, 1] + src[j, 3]], sc[j]) for j in range(nd)]
        dt += [mine[j] for j in rng.permutation(len(mine))]  # categories interleaved inside an image
    return pack(img_ids, cat_ids, gt, dt)


def plain_case(rng, img_ids, cat_ids):
    K, cat_sorted, gt, dt = len(cat_ids), np.sort(cat_ids), [], []
    for iid in img_ids:
        mine = []
        for k in range(K):
            ng, nd = int(rng.integers(0, 5)), int(rng.integers(0, 12))
            wh = rng.uniform(6, 180, (ng, 2))
            gb = np.concatenate([rng.uniform(0, 300, (ng, 2)), wh], 1)
            for j in range(ng):
                gt.append((iid, cat_sorted[k], gb[j], gb[j, 2] * gb[j, 3] * rng.uniform(0.4, 1.0), rng.random() < 0.15))
            for j in range(nd):
                if ng and rng.random() < 0.7:
                    b = gb[rng.integers(0, ng)] * (1 + rng.normal(0, 0.07, 4))
                else:
                    b = np.concatenate([rng.uniform(0, 300, 2), rng.uniform(6, 180, 2)])
                mine.append((iid, k, [b[0], b[1], b[0] + max(b[2], 1), b[1] + max(b[3], 1)], rng.random()))
        dt += [mine[j] for j in rng.permutation(len(mine))]
    return pack(img_ids, cat_ids, gt, dt)


def pack(img_ids, cat_ids, gt, dt):
    a = lambda xs, dt_, shape=(-1,): np.array(xs, dt_).reshape(shape)
    return dict(img_ids=a(img_ids, np.int64), cat_ids=a(cat_ids, np.int64),
                gt_img=a([g[0] for g in gt], np.int64), gt_cat=a([g[1] for g in gt], np.int64),
                gt_box=a([g[2] for g in gt], np.float64, (-1, 4)), gt_area=a([g[3] for g in gt], np.float64),
                gt_crowd=a([g[4] for g in gt], np.uint8),
                dt_img=a([d[0] for d in dt], np.int64), dt_cls=a([d[1] for d in dt], np.int64),
                dt_box=a([d[2] for d in dt], np.float32, (-1, 4)), dt_score=a([d[3] for d in dt], np.float32))


def make_cases():
    return {
        "ties": grid_case(np.random.default_rng(SEEDS["ties"]), [101, 7, 55, 1030, 12, 900, 77], [20, 3, 42, 7, 11],
                          no_gt_cat=3, no_dt_cat=1, no_dt_img=4),
        "wide": grid_case(np.random.default_rng(SEEDS["wide"]), [4, 2, 9, 6], [5, 1, 3], wide=(1, 0)),
        "plain": plain_case(np.random.default_rng(SEEDS["plain"]), list(range(40, 4, -3)), [2, 90, 17, 33]),
    }


SEEDS = {"ties": 2, "wide": 5, "plain": 11}


def exact_ious(case, value):
    _, _, pairs = U.prepare(case)
    return sum(int((U.bb_iou(p[3], p[0], p[2]) == value).sum()) for row in pairs for p in row)


def check_case(name, case, ev):
    """the non-degeneracy conditions (tests/test_coco_eval_cpu.py re-checks them on the file)"""
    frac = float((ev["precision"] == -1).mean())
    ap = ev["precision"][:, :, :, 0, 2]
    ap = float(ap[ap > -1].mean())
    msg = "%s: %.1f %% of precision at -1, AP(all, 100) %.3f" % (name, 100 * frac, ap)
    if name in ("ties", "wide"):
        n50, n75 = exact_ious(case, 0.5), exact_ious(case, 0.75)
        msg += ", IoU == 0.5: %d, == 0.75: %d" % (n50, n75)
        assert n50 >= 10 and n75 >= 10, msg
    print(msg)
    assert frac < 0.25 and 0.05 <= ap <= 0.9, msg


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
    ap.add_argument("--time", action="store_true", help="time the C++ on the bench tool's minival-sized input instead")
    ap.add_argument("--images", type=int, default=5000)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        C = build_binding(tmp)
        if args.time:
            from coco_eval_bench import make_input

            case = make_input(images=args.images)
            I, K, gts, dts, ious = reference_inputs(C, case)
            best = []
            for _ in range(3):
                t0 = time.perf_counter()
                evs = C.EvaluateImages(U.AREA_RNG.tolist(), 100, list(U.IOU_THRS), ious, gts, dts)
                t1 = time.perf_counter()
                r = C.Accumulate(params_of(I, K), evs)
                t2 = time.perf_counter()
                best.append((t2 - t0, t1 - t0, t2 - t1))
            tot, ev_, acc = min(best)
            pr = np.array(r["precision"]).reshape(list(r["counts"]))[:, :, :, 0, 2]
            print("reference C++ (cocoeval.cpp, g++ -O2, one CPU thread), %d images, %d detections, %d GT: EvaluateImages %.1f ms"
                  " + Accumulate %.1f ms = %.1f ms (best of 3; IoUs and list building not counted); AP %.4f"
                  % (I, len(case["dt_img"]), len(case["gt_img"]), ev_ * 1e3, acc * 1e3, tot * 1e3, 100 * float(pr[pr > -1].mean())))
            return
        out = {}
        for name, case in make_cases().items():
            ev = run_reference(C, case)
            mine = U.evaluate_numpy(case)
            for k in U.EV_KEYS:
                assert np.array_equal(ev[k], mine[k]), (name, k)  # the numpy restatement, bit for bit
            check_case(name, case, ev)
            for k in U.INPUT_KEYS:
                out["%s_%s" % (name, k)] = case[k]
            for k in U.EV_KEYS:
                out["%s_%s" % (name, k)] = ev[k]
        path = os.path.join(HERE, "coco_eval.npz")
        save_fixed(path, out)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
