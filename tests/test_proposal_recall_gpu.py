"""GPU tests of the box-proposal recall kernels (csrc/proprecall.hip), of ProposalRecallEvaluator and of COCOEvaluator's
box_proposals branch.  Every comparison is np.array_equal: the reference computes single IEEE fp32 operations, compares
and counts, and so do the kernels - there is no tolerance to choose."""
import importlib

import numpy as np
import pytest
import torch

import coco_eval_util as CU
import proposal_recall_util as U
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

THR = U.default_thresholds().numpy()


@pytest.fixture(scope="module")
def ops():
    load_package()
    return importlib.import_module("drn_wsod_pytorch_amd.ops")


@pytest.fixture(scope="module")
def ev_mod():
    load_package()
    return importlib.import_module("drn_wsod_pytorch_amd.evaluation")


@pytest.fixture(scope="module")
def structures():
    load_package()
    return importlib.import_module("drn_wsod_pytorch_amd.structures")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_op(ops, f, areas, limits, thr=THR):
    ngt, npr = np.diff(f["gt_off"]), np.diff(f["prop_off"])
    cut = None if None in limits else max(limits)
    max_prop = int(npr.max() if cut is None else np.minimum(npr, cut).max()) if len(npr) else 0
    out = ops.proposal_recall(dev(f["prop_box"]), dev(f["prop_logit"]), dev(f["prop_off"]), dev(f["gt_box"]),
                              dev(f["gt_area"]), dev(f["gt_off"]), dev(U.area_array(areas)), dev(U.limit_array(limits)),
                              dev(np.asarray(thr, np.float32)), int(ngt.max()) if len(ngt) else 0, max_prop)
    return tuple(out[k].cpu().numpy() for k in ("overlaps", "counts", "num_pos"))


def check_op(ops, f, areas, limits):
    got, want = run_op(ops, f, areas, limits), U.device_layout(f, areas, limits, THR)
    for g, w, k in zip(got, want, ("overlaps", "counts", "num_pos")):
        assert g.dtype == w.dtype and np.array_equal(g, w), k
    return got


@pytest.mark.parametrize("name", U.CASES)
def test_op_equals_golden(name, ops):
    c = U.load_case(name)
    ov, counts, num_pos = check_op(ops, U.flat_inputs(c), U.AREA_NAMES, U.LIMITS)
    for a, area in enumerate(U.AREA_NAMES):
        for l, limit in enumerate(U.LIMITS):
            want = U.golden_pair(c, area, limit)
            assert np.array_equal(np.sort(ov[a, l][ov[a, l] >= 0]), want["gt_overlaps"]), (area, limit)
            assert num_pos[a] == want["num_pos"]
            assert np.array_equal(counts[a, l], (want["gt_overlaps"][None, :] >= THR[:, None]).sum(1))


def feed(e, c, structures, image_order, device, calls=2):
    """process() in `calls` calls of several images each"""
    for chunk in np.array_split(np.asarray(image_order), calls):
        e.process([{"image_id": int(i)} for i in chunk],
                  [{"proposals": U.proposals_of(c, i, structures, device)} for i in chunk])


def check_results(e, c, areas, limits):
    for area in areas:
        for limit in limits:
            want, got = U.golden_pair(c, area, limit), e.results[(area, limit)]
            for k in ("gt_overlaps", "recalls", "ar"):
                assert not got[k].is_cuda and got[k].dtype == torch.float32
                assert np.array_equal(got[k].numpy(), want[k], equal_nan=True), (area, limit, k)
            assert got["num_pos"] == want["num_pos"] and np.array_equal(got["thresholds"].numpy(), THR)
            assert np.array_equal(e.counts[(area, limit)].numpy(), (want["gt_overlaps"][None, :] >= THR[:, None]).sum(1))


@pytest.mark.parametrize("name", U.CASES)
def test_evaluator_equals_golden(name, ev_mod, structures):
    c = U.load_case(name)
    e = ev_mod.ProposalRecallEvaluator(U.annotations_of(c), limits=U.LIMITS, areas=U.AREA_NAMES)
    feed(e, c, structures, np.random.default_rng(1).permutation(c["img_ids"]), "cuda")
    res = e.evaluate()["box_proposals"]
    check_results(e, c, U.AREA_NAMES, U.LIMITS)
    assert list(res) == [ev_mod.proposal_recall_key(a, l) for l in U.LIMITS for a in U.AREA_NAMES]
    for area, key in (("all", "AR@20"), ("small", "ARs@20"), ("512-inf", "AR[512-inf]@all")):
        want = float(float(U.golden_pair(c, area, 20 if "20" in key else None)["ar"]) * 100)  # :235: ar.item() * 100, in fp64
        assert res[key] == want or (np.isnan(want) and np.isnan(res[key])), key  # (NaN: no box of that area, 0 / 0)
    one = ev_mod.evaluate_box_proposals([{"image_id": int(i), "proposals": U.proposals_of(c, i, structures)} for i in c["img_ids"]],
                                        U.annotations_of(c), area="medium", limit=4)
    want = U.golden_pair(c, "medium", 4)
    assert np.array_equal(one["gt_overlaps"].numpy(), want["gt_overlaps"]) and one["num_pos"] == want["num_pos"]
    assert np.array_equal(one["ar"].numpy(), want["ar"], equal_nan=True)


def test_host_and_device_resident_and_two_runs(ev_mod, structures, ops):
    c = U.load_case("ties")
    runs = []
    for device in ("cuda", "cpu", "cuda"):
        e = ev_mod.ProposalRecallEvaluator(U.annotations_of(c))
        feed(e, c, structures, c["img_ids"], device)
        res = e.evaluate()
        runs.append((res, e.results))
    for res, results in runs[1:]:
        assert res == runs[0][0]
        for key, r in results.items():
            assert np.array_equal(r["gt_overlaps"].numpy(), runs[0][1][key]["gt_overlaps"].numpy())
    f = U.flat_inputs(c)
    a, b = run_op(ops, f, U.AREA_NAMES, U.LIMITS), run_op(ops, f, U.AREA_NAMES, U.LIMITS)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def quarter_image(rng, ng, npr):
    """quarter-pixel boxes; proposals jittered from boxes (ties in IoU occur), copies, or at random -> flat-input pieces"""
    gb = np.concatenate([rng.integers(0, 1600, (ng, 2)) / 4, rng.integers(16, 700, (ng, 2)) / 4], 1)
    pb = np.concatenate([rng.integers(0, 1600, (npr, 2)) / 4, rng.integers(16, 700, (npr, 2)) / 4], 1)
    near = rng.random(npr) < 0.7
    src = gb[rng.integers(0, ng, npr)] + rng.integers(-2, 3, (npr, 4)) * rng.integers(0, 2, (npr, 1)) * 4.0
    pb[near] = src[near]
    pb[:, 2:] = np.maximum(pb[:, 2:], 1)
    xyxy = lambda b: np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1).astype(np.float32)
    return xyxy(pb), rng.permutation(npr).astype(np.float32), xyxy(gb), (gb[:, 2] * gb[:, 3]).astype(np.float32)


def flat_of(images):
    off = lambda k: np.concatenate([[0], np.cumsum([len(im[k]) for im in images])]).astype(np.int32)
    return dict(prop_box=np.concatenate([im[0] for im in images]).reshape(-1, 4), prop_logit=np.concatenate([im[1] for im in images]),
                prop_off=off(1), gt_box=np.concatenate([im[2] for im in images]).reshape(-1, 4),
                gt_area=np.concatenate([im[3] for im in images]), gt_off=off(3))


def test_block_edges(ops):
    """G' in {1, 63, 64, 65} against P' in {1, 63, 64, 65, 257}: one wave's width either side, more proposals than a
    workgroup has threads; one image at the cap of boxes; limits that cut inside and outside a wave"""
    rng = np.random.default_rng(5)
    images = [quarter_image(rng, g, p) for g in (1, 63, 64, 65) for p in (1, 63, 64, 65, 257)]
    images.append(quarter_image(rng, ops.PROPOSAL_MAX_GT, 300))
    f = flat_of(images)
    assert np.diff(f["gt_off"]).max() == ops.PROPOSAL_MAX_GT
    ov, counts, num_pos = check_op(ops, f, ("all", "small", "medium", "large"), (None, 64, 65))
    assert num_pos[0] == len(f["gt_area"]) and num_pos[1] > 0 and num_pos[2] > 0 and num_pos[3] > 0
    top = ov[0, 0]
    assert (top >= 0).all() and 0.2 < (top >= 0.5).mean() < 0.95 and (top == 0).any()


def test_stable_order_at_the_cut(ops):
    """equal logits straddling the cut: the earlier row is kept.  Rows 1 and 2 tie; with limit 2 only row 1 (no overlap)
    stays, so the box's entry is row 0's IoU and not the exact copy's 1.0"""
    box = np.array([[0, 0, 32, 32]], np.float32)
    props = np.array([[0, 0, 32, 16], [100, 100, 120, 120], [0, 0, 32, 32], [0, 0, 16, 16]], np.float32)
    logits = np.array([9, 5, 5, 1], np.float32)
    f = dict(prop_box=props, prop_logit=logits, prop_off=np.array([0, 4], np.int32), gt_box=box,
             gt_area=np.array([1024], np.float32), gt_off=np.array([0, 1], np.int32))
    ov, _, _ = check_op(ops, f, ("all",), (2, 3, None))
    assert ov[0, :, 0].tolist() == [0.5, 1.0, 1.0]
    rng = np.random.default_rng(3)  # and at random: logits from five values, cuts everywhere
    images = []
    for _ in range(6):
        pb, _, gb, ga = quarter_image(rng, int(rng.integers(1, 9)), 40)
        images.append((pb, rng.integers(0, 5, 40).astype(np.float32), gb, ga))
    check_op(ops, flat_of(images), ("all", "medium"), (1, 2, 3, 5, 8, 13, 21, 34))


def test_first_index_wins(ops):
    """two boxes and one proposal that covers both equally: the lower annotation index takes it"""
    one = lambda rows: np.array(rows, np.float32).reshape(-1, 4)
    f = dict(prop_box=one([[40, 0, 48, 32], [16, 0, 48, 32]]), prop_logit=np.array([1, 2], np.float32),
             prop_off=np.array([0, 2], np.int32), gt_box=one([[0, 0, 32, 32], [32, 0, 64, 32]]),
             gt_area=np.array([1024, 1024], np.float32), gt_off=np.array([0, 2], np.int32))
    ov, _, _ = check_op(ops, f, ("all",), (None,))
    third = np.float32(512) / np.float32(1536)
    assert ov[0, 0].tolist() == [float(third), 0.25]  # (box 1 taking it would leave box 0 with 0)
    # two equal boxes share one exact copy; the second is left with the best of the rest, among equal IoUs the first
    f = dict(prop_box=one([[0, 0, 16, 32], [0, 0, 32, 32], [16, 0, 32, 32], [0, 0, 32, 32]]),
             prop_logit=np.array([4, 3, 2, 1], np.float32), prop_off=np.array([0, 4], np.int32),
             gt_box=one([[0, 0, 32, 32], [0, 0, 32, 32]]), gt_area=np.array([1024, 1024], np.float32),
             gt_off=np.array([0, 2], np.int32))
    ov, _, _ = check_op(ops, f, ("all",), (None, 3, 1))
    assert ov[0].tolist() == [[1.0, 1.0], [1.0, 0.5], [0.5, 0.0]]


def test_sorted_input_equals_shuffled(ops):
    c = U.load_case("ties")
    f = U.flat_inputs(c)
    s = {k: v.copy() for k, v in f.items()}
    for i in range(len(f["prop_off"]) - 1):
        p0, p1 = f["prop_off"][i], f["prop_off"][i + 1]
        o = np.argsort(-f["prop_logit"][p0:p1], kind="stable")
        s["prop_box"][p0:p1], s["prop_logit"][p0:p1] = f["prop_box"][p0:p1][o], f["prop_logit"][p0:p1][o]
    assert not np.array_equal(s["prop_logit"], f["prop_logit"])
    a, b = run_op(ops, f, U.AREA_NAMES, U.LIMITS), run_op(ops, s, U.AREA_NAMES, U.LIMITS)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_no_proposals_and_caps(ops):
    c = U.load_case("plain")
    f = U.flat_inputs(c)
    f.update(prop_box=np.zeros((0, 4), np.float32), prop_logit=np.zeros(0, np.float32), prop_off=np.zeros_like(f["prop_off"]))
    ov, counts, num_pos = run_op(ops, f, U.AREA_NAMES, (100, None))
    assert (ov == -1).all() and not counts.any() and not num_pos.any()
    C = importlib.import_module("drn_wsod_pytorch_amd._cabi")
    args = [dev(f[k]) for k in ("prop_box", "prop_logit", "prop_off", "gt_box", "gt_area", "gt_off")]
    args += [dev(U.area_array(("all",))), dev(U.limit_array((None,))), dev(THR)]
    with pytest.raises(C.DrnError, match="unsupported"):
        ops.proposal_recall(*args, ops.PROPOSAL_MAX_GT + 1, 0)
    with pytest.raises(C.DrnError, match="unsupported"):
        ops.proposal_recall(*args, 1, ops.PROPOSAL_MAX_PER_IMAGE + 1)


def test_through_coco_evaluator(ev_mod, structures):
    """outputs with both keys: bbox as without the proposals, box_proposals in front of it"""
    c = CU.load_case("plain")
    ann = CU.annotations_of(c)
    plain = ev_mod.COCOEvaluator(ann)
    CU.feed(plain, c, c["img_ids"], device="cuda")
    want = plain.evaluate()
    assert list(want) == ["bbox"] and np.array_equal(plain.eval["precision"], c["precision"])

    def outputs(iid, keys):
        sel = np.nonzero(c["dt_img"] == iid)[0]
        t = lambda a: torch.from_numpy(a[sel]).cuda()
        out = {"instances": structures.Instances((480, 640), pred_boxes=structures.Boxes(t(c["dt_box"])), scores=t(c["dt_score"]),
                                                 pred_classes=t(c["dt_cls"])),
               "proposals": structures.Instances((480, 640), proposal_boxes=structures.Boxes(t(c["dt_box"])),
                                                 objectness_logits=t(c["dt_score"]))}
        return {k: out[k] for k in keys}

    both, alone, only = ev_mod.COCOEvaluator(ann), ev_mod.ProposalRecallEvaluator(ann), ev_mod.COCOEvaluator(ann)
    for iid in c["img_ids"]:
        both.process([{"image_id": int(iid)}], [outputs(iid, ("instances", "proposals"))])
        alone.process([{"image_id": int(iid)}], [outputs(iid, ("proposals",))])
        only.process([{"image_id": int(iid)}], [outputs(iid, ("proposals",))])
    res = both.evaluate()
    assert list(res) == ["box_proposals", "bbox"]
    assert res["bbox"].keys() == want["bbox"].keys()
    assert all(res["bbox"][k] == want["bbox"][k] or (np.isnan(res["bbox"][k]) and np.isnan(want["bbox"][k])) for k in want["bbox"])
    for k in ("precision", "recall", "scores"):
        assert np.array_equal(both.eval[k], c[k]), k
    props = alone.evaluate()["box_proposals"]
    assert res["box_proposals"] == props and 5.0 < props["AR@100"] < 95.0
    assert list(props) == ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]
    res = only.evaluate()
    assert list(res) == ["box_proposals"] and res["box_proposals"] == props
    both.reset()
    assert list(both.evaluate()) == ["bbox"]
