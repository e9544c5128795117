"""CPU tests of the box-proposal recall evaluator: the numpy restatement against the golden file (the unmodified
reference's results), the golden file's non-degeneracy conditions, the result keys, the area default of
from_dataset_dicts and the host refusals.  No kernel runs here."""
import importlib

import numpy as np
import pytest
import torch

import proposal_recall_util as U
from __graft_entry__ import load_package


@pytest.fixture(scope="module")
def ev_mod():
    load_package()
    return importlib.import_module("drn_wsod_pytorch_amd.evaluation")


@pytest.fixture(scope="module")
def structures():
    load_package()
    return importlib.import_module("drn_wsod_pytorch_amd.structures")


@pytest.mark.parametrize("name", U.CASES)
def test_restatement_equals_golden(name):
    c = U.load_case(name)
    assert len(np.unique(c["pr_logit"])) == len(c["pr_logit"])
    for area in U.AREA_NAMES:
        for limit in U.LIMITS:
            want, got = U.golden_pair(c, area, limit), U.evaluate_numpy(c, area, limit)
            for k in ("gt_overlaps", "recalls", "ar"):
                assert np.array_equal(got[k], want[k], equal_nan=True) and got[k].dtype == np.float32, (area, limit, k)
            assert got["num_pos"] == want["num_pos"], (area, limit)


def test_golden_is_not_degenerate():
    c = U.load_case("ties")
    top = U.golden_pair(c, "all", None)
    ov = top["gt_overlaps"]
    assert 0.15 <= float(top["ar"]) <= 0.85
    for v in (0.5, 0.75, 1.0):
        assert int((ov == np.float32(v)).sum()) >= 5, v
    # entries that are 0 because the image ran out of proposals: G' - P' of them per image, and they are there
    short = sum(max(0, len(gb) - len(pb)) for pb, _, gb, _ in U.images_of(c) if len(pb) and len(gb))
    assert short >= 1 and int((ov == 0).sum()) >= short
    parts = sum(U.golden_pair(c, a, None)["num_pos"] for a in ("small", "medium", "large"))
    assert parts > top["num_pos"]  # a box of area exactly 32^2 or 96^2 counts twice: both ends are inclusive
    for a in U.AREA_NAMES:
        assert U.golden_pair(c, a, None)["num_pos"] > 0, a
    sizes = [(len(gb), len(pb)) for pb, _, gb, _ in U.images_of(c)]
    assert any(g == 0 and p > 0 for g, p in sizes) and any(p == 0 and g > 0 for g, p in sizes)
    assert c["gt_crowd"].any()
    w = U.images_of(U.load_case("wide"))
    assert len(w) == 1 and len(w[0][2]) == 70 and len(w[0][0]) == 90
    p = U.load_case("plain")
    assert not np.array_equal(p["gt_area"], p["gt_box"][:, 2] * p["gt_box"][:, 3])


def test_result_keys_and_order(ev_mod):
    keys = [ev_mod.proposal_recall_key(a, l) for l in (100, 1000) for a in ("all", "small", "medium", "large")]
    assert keys == ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]
    assert list(ev_mod.PROPOSAL_AREAS) == list(U.AREA_NAMES)
    for a in U.AREA_NAMES:
        assert [float(v) for v in ev_mod.PROPOSAL_AREAS[a]] == [float(v) for v in U.AREA_RANGES[a]]
    # an evaluation without a processed image touches no device and keeps the keys and their order
    e = ev_mod.ProposalRecallEvaluator(U.annotations_of(U.load_case("plain")))
    res = e.evaluate()
    assert list(res) == ["box_proposals"] and list(res["box_proposals"]) == keys
    assert all(np.isnan(v) for v in res["box_proposals"].values())  # 0 / 0, as in the reference
    assert list(e.results) == [(a, l) for l in (100, 1000) for a in ("all", "small", "medium", "large")]
    with pytest.raises(AssertionError, match="Unknown area range"):
        ev_mod.ProposalRecallEvaluator(U.annotations_of(U.load_case("plain")), areas=("huge",))


def test_from_dataset_dicts_area_default(ev_mod):
    w, h = np.float32(10.3), np.float32(7.7)
    dicts = [{"image_id": "000005", "annotations": [
        {"bbox": [1.5, 2.5, float(w), float(h)], "bbox_mode": 1},                       # XYWH, no area: w * h in float32
        {"bbox": [1.5, 2.5, 20.25, 30.75], "bbox_mode": 0},                             # XYXY, no area
        {"bbox": [0.0, 0.0, 4.0, 4.0], "bbox_mode": 1, "area": 11.0},                   # its own area
        {"bbox": [0.0, 0.0, 4.0, 4.0], "bbox_mode": 1, "iscrowd": 1}]},                 # crowd: left out
        {"image_id": "000007", "annotations": []}]
    e = ev_mod.ProposalRecallEvaluator.from_dataset_dicts(dicts)
    box, area = e._gt["000005"]
    assert box.dtype == np.float32 and area.dtype == np.float32 and box.shape == (3, 4)
    assert area[0] == w * h and area[1] == (np.float32(20.25) - np.float32(1.5)) * (np.float32(30.75) - np.float32(2.5))
    assert area[2] == np.float32(11.0)
    assert np.array_equal(box[0], np.array([1.5, 2.5, np.float32(1.5) + w, np.float32(2.5) + h], np.float32))
    assert np.array_equal(box[1], np.array([1.5, 2.5, 20.25, 30.75], np.float32))
    assert e._gt["000007"][0].shape == (0, 4)


def _instances(structures, n):
    return structures.Instances((100, 100), proposal_boxes=structures.Boxes(torch.zeros(n, 4)),
                                objectness_logits=torch.zeros(n))


def _annotations(n_boxes):
    return {"images": [{"id": 5}, {"id": 9}], "categories": [{"id": 1, "name": "a"}],
            "annotations": [{"id": j + 1, "image_id": 9, "category_id": 1, "bbox": [j % 50, j // 50, 10, 10], "area": 100.0,
                             "iscrowd": 0} for j in range(n_boxes)]}


def test_host_refusals(ev_mod, structures):
    """cap + 1 boxes, cap + 1 proposals after the cut, an unknown image: refused on the host, no device is touched"""
    ops = importlib.import_module("drn_wsod_pytorch_amd.ops")
    C = importlib.import_module("drn_wsod_pytorch_amd._cabi")
    assert ops.PROPOSAL_MAX_GT >= 256 and ops.PROPOSAL_MAX_PER_IMAGE >= 4096
    cap = ops.PROPOSAL_MAX_GT
    e = ev_mod.ProposalRecallEvaluator(_annotations(cap + 1))
    e.process([{"image_id": 9}], [{"proposals": _instances(structures, 3)}])
    with pytest.raises(C.DrnError, match=r"image 9 has %d ground-truth boxes.*at most %d" % (cap + 1, cap)):
        e.evaluate()
    e.reset()
    e.process([{"image_id": 5}], [{"proposals": _instances(structures, 3)}])  # the crowded image was not processed: no refusal
    pcap = ops.PROPOSAL_MAX_PER_IMAGE
    e = ev_mod.ProposalRecallEvaluator(_annotations(2), limits=(100, None))
    e.process([{"image_id": 9}], [{"proposals": _instances(structures, pcap + 1)}])
    with pytest.raises(C.DrnError, match=r"image 9 has %d proposals after the cut.*at most %d" % (pcap + 1, pcap)):
        e.evaluate()
    with pytest.raises(ValueError, match="image_id 77 is not in the annotations"):
        e.process([{"image_id": 77}], [{"proposals": _instances(structures, 1)}])
    c = ev_mod.COCOEvaluator(_annotations(2))
    with pytest.raises(ValueError, match="image_id 77"):
        c.process([{"image_id": 77}], [{"proposals": _instances(structures, 1)}])
