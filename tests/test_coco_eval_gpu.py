"""GPU tests of the COCO box-AP evaluator's kernels (csrc/cocoeval.hip) and of COCOEvaluator end to end.  Everything is
compared with np.array_equal: the reference counts integers and performs single IEEE fp64 operations, and so do the
kernels - there is no tolerance to choose."""
import importlib

import numpy as np
import pytest
import torch

import coco_eval_util as U
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    load_package()
    return importlib.import_module("drn_wsod_pytorch_amd.ops")


@pytest.fixture(scope="module")
def ev_mod():
    load_package()
    return importlib.import_module("drn_wsod_pytorch_amd.evaluation")


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).cuda()


def params():
    return dev(U.IOU_THRS), dev(U.AREA_RNG), dev(U.MAX_DETS), dev(U.REC_THRS)


def run_match(ops, f):
    iou, area, _, _ = params()
    max_gt = int(np.diff(f["gt_off"]).max()) if len(f["gt_off"]) > 1 else 0
    out = ops.coco_match(dev(f["det_box"]), dev(f["det_score"]), dev(f["det_pair"]), dev(f["gt_box"]), dev(f["gt_area"]),
                         dev(f["gt_crowd"]), dev(f["gt_off"]), f["K"], max_gt, iou, area)
    return {k: v.cpu().numpy() for k, v in out.items() if k != "ws"}


def run_accumulate(ops, rec, I, K):
    _, _, md, rec_thr = params()
    out = ops.coco_accumulate(dev(rec["s_score"]), dev(rec["s_cat"]), dev(rec["s_rank"]), dev(rec["dm"]), dev(rec["di"]),
                              dev(rec["npig"]), I, K, len(U.IOU_THRS), md, rec_thr)
    return tuple(out[k].cpu().numpy() for k in ("precision", "recall", "scores"))


def check_match(got, want):
    for k in ("order", "s_score", "s_cat", "s_rank", "dm", "di", "npig", "gt_ign"):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("name", U.CASES)
def test_match_equals_golden(name, ops):
    c = U.load_case(name)
    f = U.flat_inputs(c)
    got = run_match(ops, f)
    kept = U.pack_records(c)  # the golden bit words of the kept detections, in (pair, rank) order
    keep = got["s_rank"] < 100
    for k in ("s_score", "s_cat", "s_rank", "dm", "di"):
        assert np.array_equal(got[k][keep], kept[k]), k
    assert np.array_equal(got["npig"], kept["npig"])
    assert not got["dm"][~keep].any() and not got["di"][~keep].any()
    # ground_truth_ignores of the golden are in partitioned order: npig falses, then trues; per GT the bit is its own
    blocks = U.split_pairs(c, len(U.AREA_RNG), len(U.IOU_THRS))
    K = f["K"]
    for p in range(len(f["gt_off"]) - 1):
        g = got["gt_ign"][f["gt_off"][p]:f["gt_off"][p + 1]]
        gi = blocks[p // K][p % K][3]
        for a in range(len(U.AREA_RNG)):
            assert np.array_equal(np.sort((g >> a) & 1), gi[a])
    check_match(got, U.full_records(f))


@pytest.mark.parametrize("name", U.CASES)
def test_accumulate_equals_golden(name, ops):
    c = U.load_case(name)
    I, K = c["nd"].shape
    P, RC, S = run_accumulate(ops, U.pack_records(c), I, K)
    assert np.array_equal(P, c["precision"]) and np.array_equal(RC, c["recall"]) and np.array_equal(S, c["scores"])


@pytest.mark.parametrize("name", U.CASES)
def test_evaluator_equals_golden(name, ev_mod):
    c = U.load_case(name)
    e = ev_mod.COCOEvaluator(U.annotations_of(c))
    U.feed(e, c, np.random.default_rng(1).permutation(c["img_ids"]), device="cuda")
    res = e.evaluate()
    for k in ("precision", "recall", "scores"):
        assert np.array_equal(e.eval[k], c[k]), k
    stats = U.summarize_numpy(c["precision"], c["recall"])
    assert np.array_equal(e.stats, stats)
    for i, m in enumerate(["AP", "AP50", "AP75", "APs", "APm", "APl"]):
        assert res["bbox"][m] == stats[i] * 100 or (stats[i] < 0 and np.isnan(res["bbox"][m]))
    for k, cid in enumerate(np.sort(c["cat_ids"])):
        pr = c["precision"][:, :, k, 0, -1]
        pr = pr[pr > -1]
        got = res["bbox"]["AP-cat%d" % cid]
        assert (np.isnan(got) and pr.size == 0) or got == float(np.mean(pr) * 100)


def random_case():
    """40 images x 8 categories; pairs with exactly 100 and with 101 detections, one with 65 GT (more than a wave), one
    whose GT is all crowd; quarter-pixel boxes so that ties in IoU occur"""
    rng = np.random.default_rng(7)
    I, K = 40, 8
    special = {(3, 1): (4, 100), (5, 2): (6, 101), (9, 0): (65, 30), (11, 4): (5, 9)}
    gt, dt = [], []
    for i in range(I):
        for k in range(K):
            ng, nd = special.get((i, k), (int(rng.integers(0, 4)), int(rng.integers(0, 6))))
            gb = np.concatenate([rng.integers(0, 1200, (ng, 2)) / 4, rng.integers(16, 600, (ng, 2)) / 4], 1)
            cr = np.ones(ng, bool) if (i, k) == (11, 4) else rng.random(ng) < 0.15
            for j in range(ng):
                gt.append((i + 1, k + 1, gb[j], gb[j, 2] * gb[j, 3] * rng.choice([0.5, 1.0]), cr[j]))
            for j in range(nd):
                b = gb[rng.integers(0, ng)] + rng.integers(-12, 13, 4) / 4 if ng and rng.random() < 0.75 else \
                    np.concatenate([rng.integers(0, 1200, 2) / 4, rng.integers(16, 600, 2) / 4])
                dt.append((i + 1, k, [b[0], b[1], b[0] + max(b[2], 1), b[1] + max(b[3], 1)], rng.integers(1, 200) / 256))
    dt = [dt[j] for j in rng.permutation(len(dt))]
    a = lambda xs, t, shape=(-1,): np.array(xs, t).reshape(shape)
    return dict(img_ids=np.arange(1, I + 1), cat_ids=np.arange(1, K + 1), gt_img=a([g[0] for g in gt], np.int64),
                gt_cat=a([g[1] for g in gt], np.int64), gt_box=a([g[2] for g in gt], np.float64, (-1, 4)),
                gt_area=a([g[3] for g in gt], np.float64), gt_crowd=a([g[4] for g in gt], np.uint8),
                dt_img=a([d[0] for d in dt], np.int64), dt_cls=a([d[1] for d in dt], np.int64),
                dt_box=a([d[2] for d in dt], np.float32, (-1, 4)), dt_score=a([d[3] for d in dt], np.float32))


def test_random_case_equals_restatement(ops):
    c = random_case()
    f = U.flat_inputs(c)
    cnt = np.bincount(f["det_pair"], minlength=f["I"] * f["K"])
    assert 100 in cnt and 101 in cnt and np.diff(f["gt_off"]).max() == 65
    want = U.full_records(f)
    got = run_match(ops, f)
    check_match(got, want)
    P, RC, S = run_accumulate(ops, got, f["I"], f["K"])
    wP, wRC, wS = U.accumulate_records(want, f["K"])
    assert np.array_equal(P, wP) and np.array_equal(RC, wRC) and np.array_equal(S, wS)
    assert float((wP > -1).mean()) > 0.9 and 0.02 < float(wP[wP > -1].mean()) < 0.95


def test_over_cap_is_refused(ops, ev_mod):
    """cap + 1 GT in one pair: a plain argument check before any launch"""
    cap = ops.COCO_MAX_GT
    C = importlib.import_module("drn_wsod_pytorch_amd._cabi")
    ann = {"images": [{"id": 5}, {"id": 9}], "categories": [{"id": 2, "name": "a"}, {"id": 6, "name": "b"}],
           "annotations": [{"id": j + 1, "image_id": 9, "category_id": 6, "bbox": [j % 50, j // 50, 10, 10], "area": 100.0,
                            "iscrowd": 0} for j in range(cap + 1)]}
    e = ev_mod.COCOEvaluator(ann)
    with pytest.raises(C.DrnError, match=r"image 9 / category 6 has %d ground-truth boxes.*at most %d" % (cap + 1, cap)):
        e.evaluate()
    f = dict(det_box=np.zeros((0, 4)), det_score=np.zeros(0, np.float32), det_pair=np.zeros(0, np.int32),
             gt_box=np.zeros((cap + 1, 4)), gt_area=np.ones(cap + 1), gt_crowd=np.zeros(cap + 1, np.uint8),
             gt_off=np.array([0, cap + 1], np.int32), K=1)
    with pytest.raises(C.DrnError, match="unsupported"):
        run_match(ops, f)
    ann["annotations"].pop()  # exactly the cap: accepted
    assert np.isfinite(ev_mod.COCOEvaluator(ann).evaluate()["bbox"]["AP"])


def test_empty_predictions(ev_mod):
    c = U.load_case("ties")
    e = ev_mod.COCOEvaluator(U.annotations_of(c))
    res = e.evaluate()
    pr, rc = e.eval["precision"], e.eval["recall"]
    has_gt = c["precision"] > -1  # where the category has countable GT in the area range
    assert np.array_equal(pr > -1, has_gt) and not pr[has_gt].any() and not e.eval["scores"][has_gt].any()
    assert np.array_equal(rc > -1, c["recall"] > -1) and not rc[rc > -1].any()
    assert not np.isnan(pr).any() and not np.isnan(rc).any() and res["bbox"]["AP"] == 0.0
    empty = int(np.sort(c["cat_ids"])[np.nonzero(c["ng"].sum(0) == 0)[0][0]])
    assert np.isnan(res["bbox"]["AP-cat%d" % empty])
