"""CPU tests of the device-side PASCAL VOC evaluator's foundations: the quantisation formulas the kernels use against the
text round trip of format_prediction, the stable-tie restatement (voc_eval_util.py) against the host path and the golden
fixture on tie-free inputs, the evaluator's device-mode constructor / process() checks, and the header's entry points."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import golden_util as G
import voc_eval_util as U
from __graft_entry__ import load_package


@pytest.fixture(scope="module")
def E():
    load_package()
    return importlib.import_module("drn_wsod_pytorch_amd.evaluation")


def _score_values():
    rng = np.random.default_rng(0)
    ties = (np.arange(0, 40000) / 2000.0).astype(np.float32)  # k / 2000: x.xxx5 where float32 holds it exactly
    v = np.concatenate([rng.random(60000).astype(np.float32), ties, (rng.random(20000) * 1e-3).astype(np.float32),
                        (rng.normal(0, 3, 5000)).astype(np.float32), np.array([0.0, -0.0, 1.0, 0.0005, 0.0015], np.float32)])
    bound = ((rng.integers(0, 2000, 5000) + 0.5) / 1000.0).astype(np.float32)  # next to a rounding boundary
    return np.concatenate([v, bound, np.nextafter(bound, np.float32(-9)), np.nextafter(bound, np.float32(9))])


def _coord_values():
    rng = np.random.default_rng(1)
    v = np.concatenate([(rng.random(60000) * 2000).astype(np.float32), (np.arange(0, 40000) / 20.0).astype(np.float32),
                        (rng.integers(0, 4000, 20000) / 4 + 0.05).astype(np.float32), np.array([0.0, -1.0, -0.05], np.float32)])
    bound = (rng.integers(0, 20000, 5000) / 10.0 + 0.05).astype(np.float32)
    return np.concatenate([v, bound, np.nextafter(bound, np.float32(-9)), np.nextafter(bound, np.float32(9e6))])


def test_quantisation_formulas_equal_the_text_round_trip(E):
    s, x = _score_values(), _coord_values()
    assert len(s) >= len(x) >= 100000
    s = np.concatenate([s[:len(x) - 5], s[-5:]])  # one line per value of each kind; the hand-picked scores stay in
    boxes = np.stack([x, x[::-1], x, x[::-1]], 1).copy()
    qs, qb = U.quant_score(s), U.quant_box(boxes)
    bad_s = bad_b = 0
    for i in range(len(s)):
        f = E.format_prediction("id", s[i], boxes[i].copy()).split(" ")
        bad_s += float(f[1]) != qs[i]
        bad_b += [float(z) for z in f[2:]] != list(qb[i])
    assert bad_s == 0 and bad_b == 0
    assert not np.signbit(U.quant_score(np.array([-0.0, -0.0004], np.float32))).any()


def _check_against_host(E, case, bound_only_area=True):
    U.assert_tie_free(case)
    res = U.restate(case)
    lines = U.host_lines(case, E)
    for k, name in enumerate(case["classes"]):
        nd = len(lines[k])
        for ti, thr in enumerate(U.THRS):
            cl = E.voc_eval_corloc(lines[k], case["annos"], name, thr, True)
            assert cl == res[k]["corloc"][ti]
            if not nd:
                continue
            rec, prec, ap07 = E.voc_eval(lines[k], case["annos"], name, thr, True)
            assert np.array_equal(rec, res[k]["rec"][ti]) and np.array_equal(prec, res[k]["prec"][ti])
            assert ap07 == res[k]["ap07"][ti]
            ap12 = E.voc_eval(lines[k], case["annos"], name, thr, False)[2]
            assert abs(ap12 - res[k]["ap12"][ti]) <= nd * 2.0 ** -53
    return res


def test_restatement_equals_host_and_golden_on_the_fixture(E):
    d = G.load("voc_eval")
    classes, annos, dets = G.voc_fixture(int(d["seed"]))
    case = U.golden_case(classes, annos, dets)
    f = U.flat_inputs(case)
    assert sorted(np.bincount(f["det_cls"]).tolist()) == [5, 7, 9]
    # float32 scores print like the fixture's python floats, so the golden numbers are the device path's too
    want = np.array([float("%.3f" % s) for _, _, s, _ in dets])
    got = np.concatenate([U.quant_score(c[2]) for c in case["calls"]])
    assert np.array_equal(np.sort(want), np.sort(got))
    res = _check_against_host(E, case)  # asserts tie-freeness first
    for ci, name in enumerate(classes):
        assert np.array_equal(res[ci]["rec"][0], d["rec_1_" + name]) and np.array_equal(res[ci]["prec"][0], d["prec_1_" + name])
        for ti in range(10):
            assert abs(res[ci]["ap07"][ti] * 100 - d["ap_y07"][ti, ci]) < 1e-9
            assert abs(res[ci]["ap12"][ti] * 100 - d["ap_y12"][ti, ci]) < 1e-9
            assert abs(res[ci]["corloc"][ti] * 100 - d["corloc_y07"][ti, ci]) < 1e-9
            assert abs(res[ci]["corloc"][ti] * 100 - d["corloc_y12"][ti, ci]) < 1e-9


def test_restatement_equals_host_on_a_larger_tie_free_case(E):
    case = U.tie_free_case(seed=4, n_img=25, n_cls=4, per_img=12)
    res = _check_against_host(E, case)
    assert any(r["tp"].any() for r in res) and any((r["tp"] + r["fp"] == 0).any() for r in res)
    ev = E.PascalVOCDetectionEvaluator(case["classes"], annotations=case["annos"], year=2007)
    U.feed(ev, case)
    host, mine = ev.evaluate(), U.results_dict(case, res, 2007)
    assert host["bbox"] == mine["bbox"] and host["bbox CorLoc"] == mine["bbox CorLoc"] and host["per_class"] == mine["per_class"]


def test_edge_case_holds_what_it_claims():
    """the situations tests/test_voc_eval_gpu.py lists are really in the tie-heavy case"""
    case = U.edge_case()
    f = U.flat_inputs(case)
    res = U.restate(case)
    qs = U.quant_score(f["det_score"])
    assert len(np.unique(qs)) <= 14 < len(np.unique(f["det_score"])) and f["npos"][4] == 0 and len(res[3]["order"]) == 0
    assert f["npos"][3] > 0 and len(res[4]["order"]) > 0 and len(f["det_score"]) >= 2500
    first = [int(np.nonzero(res[0]["order"] == j)[0][0]) for j in range(6)]  # the six hand-made detections of image 0
    assert res[0]["ovmax"][first[0]] == 0.5 and res[0]["fp"][0, first[0]] == 1  # IoU exactly 0.5: no match at 0.5
    assert res[0]["tp"][0, first[1]] == 1 and res[0]["fp"][0, first[2]] == 1  # the duplicate is a false positive
    assert res[0]["ovmax"][first[3]] == 0.0 and res[0]["ovmax"][first[4]] == 0.0
    one = [int(np.nonzero(res[1]["order"] == 75 + j)[0][0]) for j in range(2)]
    assert (res[1]["jmax"][one] == 0).all() and not res[1]["tp"][:, one].any() and not res[1]["fp"][0, one].any()
    two = [int(np.nonzero(res[2]["order"] == 75 + 2 + j)[0][0]) for j in range(2)]
    assert (res[2]["jmax"][two] == 0).all() and sorted(res[2]["tp"][0, two]) == [0, 1]


def test_device_mode_constructs_and_checks_without_a_gpu(E):
    case = U.edge_case()
    ev = E.PascalVOCDetectionEvaluator(case["classes"], annotations=case["annos"], year=2007, device="cuda")
    f = U.flat_inputs(case)
    for k in ("npos", "npos_im"):
        assert np.array_equal(ev._gt[k], f[k])
    assert np.array_equal(ev._gt["off"], f["gt_off"]) and np.array_equal(ev._gt["box"], f["gt_box"])
    assert np.array_equal(ev._gt["diff"], f["gt_diff"])
    U.feed(ev, case, calls=case["calls"][:2])  # CPU tensors are only kept here
    from drn_wsod_pytorch_amd.structures import Boxes, Instances

    inst = Instances((10, 10))
    inst.pred_boxes, inst.pred_classes = Boxes(torch.zeros(1, 4)), torch.zeros(1, dtype=torch.int64)
    inst.scores = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(TypeError, match="float32 or narrower"):
        ev.process([{"image_id": case["calls"][0][0]}], [{"instances": inst}])
    inst.scores = torch.zeros(1)
    with pytest.raises(ValueError, match="not in the annotations"):
        ev.process([{"image_id": "nope"}], [{"instances": inst}])


def test_header_declares_the_voc_entry_points():
    load_package()
    C = importlib.import_module("drn_wsod_pytorch_amd._cabi")
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    declared = set(re.findall(r"\b(drn_[a-z0-9_]+)\s*\(", hdr))
    used = {n for n in C._SIGS if n.startswith("drn_voc_")}
    assert used == {"drn_voc_match", "drn_voc_accumulate"} and used <= declared
    ops = importlib.import_module("drn_wsod_pytorch_amd.ops")
    assert int(re.search(r"#define DRN_VOC_MAX_GT (\d+)", hdr).group(1)) == ops.VOC_MAX_GT >= 64
    assert int(re.search(r"#define DRN_VOC_MAX_REC (\d+)", hdr).group(1)) == ops.VOC_MAX_REC
