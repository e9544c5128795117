"""GPU tests of the device-side PASCAL VOC evaluator: the kernels of csrc/voceval.hip through ops.voc_match /
ops.voc_accumulate and PascalVOCDetectionEvaluator(device="cuda") end to end, for the VOC07 and the area metric.

Everything is integer counting plus single IEEE fp64 operations in the host's order, so it is compared with equality; the
area AP alone is summed in another order: its terms are non-negative and sum to at most 1, so two orders differ by at most
nd * 2^-53 (nd = the class's detections).  The evaluator's dict multiplies by 100 and takes two means of at most ten
values <= 100, each a few roundings of numbers below 1024: (nd + 16) * 100 * 2^-53 bounds its area-metric entries.
Tie-free cases are held against the host path and the golden file, tie-heavy ones against voc_eval_util.restate, which
fixes the tie order the way the kernels define it (processing order)."""
import importlib

import numpy as np
import pytest
import torch

import golden_util as G
import voc_eval_util as U
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def ops():
    load_package()
    return importlib.import_module("drn_wsod_pytorch_amd.ops")


@pytest.fixture(scope="module")
def E():
    load_package()
    return importlib.import_module("drn_wsod_pytorch_amd.evaluation")


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).cuda()


def run_ops(ops, case, year):
    f = U.flat_inputs(case)
    max_gt = int(np.diff(f["gt_off"]).max())
    m = ops.voc_match(dev(f["det_box"]), dev(f["det_score"]), dev(f["det_pair"]), dev(f["gt_box"]), dev(f["gt_diff"]),
                      dev(f["gt_off"]), f["K"], max_gt, dev(U.THRS))
    acc = ops.voc_accumulate(m["tp"], m["fp"], m["cls_off"], m["hit"], dev(f["npos"]), dev(f["npos_im"]), len(U.THRS),
                             dev(U.REC_THRS), year == 2007, curve_at=0)
    got = {k: v.cpu().numpy() for k, v in m.items() if k != "ws"}
    got.update({k: v.cpu().numpy() for k, v in acc.items()})
    return got


def check_ops(got, want, year):
    """want: per class dicts like voc_eval_util.restate returns (order / score / ovmax / jmax / tp / fp may be absent)"""
    assert got["cls_off"][0] == 0 and got["cls_off"][-1] == len(got["order"])
    for k, w in enumerate(want):
        seg = slice(got["cls_off"][k], got["cls_off"][k + 1])
        nd = seg.stop - seg.start
        assert nd == w["rec"].shape[1], k
        for key, mine in (("order", "order"), ("score", "s_score"), ("ovmax", "ovmax"), ("jmax", "jmax")):
            if key in w:
                assert np.array_equal(got[mine][seg], w[key]), (k, key)
        for ti in range(len(U.THRS)):
            for key in ("tp", "fp"):
                if key in w:
                    assert np.array_equal((got[key][seg] >> ti) & 1, w[key][ti].astype(np.int64)), (k, key, ti)
            assert got["corloc"][ti, k] == w["corloc"][ti], (k, ti)
            if year == 2007:
                assert got["ap"][ti, k] == w["ap07"][ti], (k, ti)
            else:
                assert abs(got["ap"][ti, k] - w["ap12"][ti]) <= nd * EPS, (k, ti)
        assert np.array_equal(got["rec"][seg], w["rec"][0]) and np.array_equal(got["prec"][seg], w["prec"][0]), k


def check_dict(got, want, year, nd_max):
    assert list(got) == ["bbox", "bbox CorLoc", "per_class"]
    assert got["bbox CorLoc"] == want["bbox CorLoc"] and got["per_class"]["CL50"] == want["per_class"]["CL50"]
    tol = 0.0 if year == 2007 else (nd_max + 16) * 100 * EPS
    assert list(got["per_class"]["AP50"]) == list(want["per_class"]["AP50"])
    for a, b in [(got["bbox"][k], want["bbox"][k]) for k in ("AP", "AP50", "AP75")] + \
            [(got["per_class"]["AP50"][n], want["per_class"]["AP50"][n]) for n in want["per_class"]["AP50"]]:
        assert abs(a - b) <= tol, (a, b)


def run_evaluator(E, case, year, **kw):
    ev = E.PascalVOCDetectionEvaluator(case["classes"], annotations=case["annos"], year=year, device="cuda", **kw)
    U.feed(ev, case, device="cuda")
    return ev.evaluate()


def nd_max(case):
    return int(np.bincount(U.flat_inputs(case)["det_cls"], minlength=1).max())


def host_reference(E, case):
    """the host path's own functions on the case's lines, per class like restate() (curves, APs, CorLoc)"""
    lines, out = U.host_lines(case, E), []
    for k, name in enumerate(case["classes"]):
        nd = len(lines[k])
        w = dict(rec=np.zeros((10, nd)), prec=np.zeros((10, nd)), ap07=np.zeros(10), ap12=np.zeros(10), corloc=np.zeros(10))
        for ti, thr in enumerate(range(50, 100, 5)):
            if nd:
                w["rec"][ti], w["prec"][ti], w["ap07"][ti] = E.voc_eval(lines[k], case["annos"], name, thr / 100.0, True)
                w["ap12"][ti] = E.voc_eval(lines[k], case["annos"], name, thr / 100.0, False)[2]
            w["corloc"][ti] = E.voc_eval_corloc(lines[k], case["annos"], name, thr / 100.0, True)
        out.append(w)
    return out


@pytest.fixture(scope="module")
def tie_free(E):
    case = U.tie_free_case()
    assert 1200 <= len(U.flat_inputs(case)["det_score"]) <= 1800
    return case, host_reference(E, case)


@pytest.fixture(scope="module")
def edge():
    case = U.edge_case()
    return case, U.restate(case)


@pytest.mark.parametrize("year", [2007, 2012])
def test_golden_fixture(year, ops, E):
    d = G.load("voc_eval")
    classes, annos, dets = G.voc_fixture(int(d["seed"]))
    case = U.golden_case(classes, annos, dets)
    U.assert_tie_free(case)
    tag = "y07" if year == 2007 else "y12"
    got = run_ops(ops, case, year)
    for ci, name in enumerate(classes):
        seg = slice(got["cls_off"][ci], got["cls_off"][ci + 1])
        assert np.array_equal(got["rec"][seg], d["rec_%d_%s" % (year == 2007, name)])
        assert np.array_equal(got["prec"][seg], d["prec_%d_%s" % (year == 2007, name)])
    assert np.abs(got["ap"] * 100 - d["ap_" + tag]).max() < 1e-9
    assert np.abs(got["corloc"] * 100 - d["corloc_" + tag]).max() < 1e-9
    check_ops(got, U.restate(case), year)
    res = run_evaluator(E, case, year)
    assert abs(res["bbox"]["AP50"] - np.mean(d["ap_" + tag][0])) < 1e-9
    assert abs(res["bbox"]["AP"] - np.mean(np.mean(d["ap_" + tag], 1))) < 1e-9
    assert abs(res["bbox CorLoc"]["CL75"] - np.mean(d["corloc_" + tag][5])) < 1e-9
    check_dict(res, U.results_dict(case, U.restate(case), year), year, 9)


@pytest.mark.parametrize("year", [2007, 2012])
def test_tie_free_random_equals_host_path(year, ops, E, tie_free):
    case, host = tie_free
    check_ops(run_ops(ops, case, year), host, year)
    check_ops(run_ops(ops, case, year), U.restate(case), year)  # and the per-detection records
    ev = E.PascalVOCDetectionEvaluator(case["classes"], annotations=case["annos"], year=year)
    U.feed(ev, case)
    check_dict(run_evaluator(E, case, year), ev.evaluate(), year, nd_max(case))


@pytest.mark.parametrize("year", [2007, 2012])
def test_tie_heavy_and_edge_cases(year, ops, E, edge):
    case, want = edge
    got = run_ops(ops, case, year)
    check_ops(got, want, year)
    assert got["ovmax"][got["cls_off"][0]] == 0.5 and not (got["tp"][got["cls_off"][0]] & 1)  # IoU 0.5 exactly: strict >
    check_dict(run_evaluator(E, case, year), U.results_dict(case, want, year), year, nd_max(case))


def test_sort_across_tile_boundaries(ops, E):
    case = U.tile_case()
    f = U.flat_inputs(case)
    assert np.bincount(f["det_cls"])[0] == 2 * 4096 + 37 and len(np.unique(U.quant_score(f["det_score"]))) < 100
    want = U.restate(case)
    for year in (2007, 2012):
        check_ops(run_ops(ops, case, year), want, year)
        check_dict(run_evaluator(E, case, year), U.results_dict(case, want, year), year, nd_max(case))


def test_cap(ops, E):
    C = importlib.import_module("drn_wsod_pytorch_amd._cabi")
    case = U.cap_case(ops.VOC_MAX_GT)
    want = U.restate(case)
    for year in (2007, 2012):
        check_ops(run_ops(ops, case, year), want, year)
        check_dict(run_evaluator(E, case, year), U.results_dict(case, want, year), year, nd_max(case))
    assert want[1]["tp"].any() and (want[1]["jmax"] >= 64).any()
    over = U.cap_case(ops.VOC_MAX_GT + 1)
    ev = E.PascalVOCDetectionEvaluator(over["classes"], annotations=over["annos"], device="cuda")
    with pytest.raises(C.DrnError, match=r"image img9 / class b has %d ground-truth boxes.*at most %d"
                       % (ops.VOC_MAX_GT + 1, ops.VOC_MAX_GT)):
        ev.evaluate()
    with pytest.raises(C.DrnError, match="unsupported"):
        run_ops(ops, over, 2007)


@pytest.mark.parametrize("year", [2007, 2012])
def test_empty(year, E, edge):
    case, _ = edge
    layout = U.results_dict(case, U.restate(dict(case, calls=[])), year)
    empty_call = (case["calls"][0][0], np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64))
    for calls in ([], [empty_call, empty_call]):
        res = run_evaluator(E, dict(case, calls=calls), year)
        assert list(res) == list(layout) and all(list(res[k]) == list(layout[k]) for k in res)
        assert all(v == 0.0 for k in ("bbox", "bbox CorLoc") for v in res[k].values())
        assert all(v == 0.0 for k in ("AP50", "CL50") for v in res["per_class"][k].values())
        assert list(res["per_class"]["AP50"]) == case["classes"]


def test_gather(E, edge):
    case, want = edge
    single = run_evaluator(E, case, 2007)
    cut = sum(len(c[2]) for c in case["calls"][:17])  # an image boundary
    seen = []

    def gather(part):
        seen.append(part)
        assert all(isinstance(v, np.ndarray) for v in part.values())
        return [{k: v[:cut] for k, v in part.items()}, {k: v[cut:] for k, v in part.items()}]

    res = run_evaluator(E, case, 2007, gather=gather)
    assert len(seen) == 1 and res == single
    check_dict(res, U.results_dict(case, want, 2007), 2007, 0)
    assert run_evaluator(E, case, 2007, gather=lambda part: None) is None


def test_default_path_is_unchanged(E, tie_free):
    """device=None with CUDA Instances: the host path's numbers, from voc_eval / voc_eval_corloc called directly"""
    case, host = tie_free
    for year, key in ((2007, "ap07"), (2012, "ap12")):
        ev = E.PascalVOCDetectionEvaluator(case["classes"], annotations=case["annos"], year=year)
        U.feed(ev, case, device="cuda")
        res = ev.evaluate()
        want = U.results_dict(case, [dict(w, ap07=w[key], ap12=w[key]) for w in host], year)
        assert res["bbox"] == want["bbox"] and res["bbox CorLoc"] == want["bbox CorLoc"]
        assert res["per_class"] == want["per_class"]


def test_process_does_not_synchronise(E, tie_free):
    case, _ = tie_free
    ev = E.PascalVOCDetectionEvaluator(case["classes"], annotations=case["annos"], device="cuda")
    from drn_wsod_pytorch_amd.structures import Boxes, Instances

    staged = []
    for iid, box, score, cls in case["calls"]:
        inst = Instances((500, 500))
        inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(dev(box)), dev(score), dev(cls)
        staged.append(([{"image_id": iid}], [{"instances": inst}]))
    torch.cuda.synchronize()
    try:
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:  # this build may not implement the mode
        pytest.skip("torch.cuda.set_sync_debug_mode is not usable here: %r" % (e,))
    try:
        for inputs, outputs in staged:
            ev.process(inputs, outputs)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert len(ev._boxes) == len(case["calls"])
