"""GPU tests of the padded evaluation path: DetectionBatch blocks through both device evaluators, model.inference(padded=True),
GeneralizedRCNNWithTTAAVG(padded=True) and evaluation.inference_on_dataset.  The padded path must compute what the unpadded
one computes, bit for bit: the same kernels see the same numbers in the same order."""
import numpy as np
import pytest
import torch

import coco_eval_util as CU
import golden_util as G
import voc_eval_util as VU
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
load_package()
from drn_wsod_pytorch_amd import evaluation as E  # noqa: E402
from drn_wsod_pytorch_amd.modeling import GeneralizedRCNNWithTTAAVG  # noqa: E402
from drn_wsod_pytorch_amd.structures import Boxes, DetectionBatch, Instances  # noqa: E402

TOPK = 100


def padded_batches(calls, per_batch=3, seed=0):
    """calls [(image_id, boxes [n, 4], scores [n], classes [n])] -> [(inputs, DetectionBatch)]: every image's detections in
    blocks of at most TOPK slots (an image without detections is a block with count 0), per_batch blocks per DetectionBatch;
    the slots beyond the count hold the tail's fill"""
    pieces = []
    for iid, box, score, cls in calls:
        box, score, cls = np.asarray(box, np.float32).reshape(-1, 4), np.asarray(score, np.float32), np.asarray(cls, np.int32)
        for lo in range(0, max(len(score), 1), TOPK):
            pieces.append((iid, box[lo: lo + TOPK], score[lo: lo + TOPK], cls[lo: lo + TOPK]))
    out = []
    for g0 in range(0, len(pieces), per_batch):
        group = pieces[g0: g0 + per_batch]
        n = len(group)
        ob, os_ = np.zeros((n, TOPK, 4), np.float32), np.zeros((n, TOPK), np.float32)
        oc, cnt = np.full((n, TOPK), -1, np.int32), np.zeros((n,), np.int32)
        for i, (_, box, score, cls) in enumerate(group):
            k = len(score)
            ob[i, :k], os_[i, :k], oc[i, :k], cnt[i] = box, score, cls, k
        batch = DetectionBatch(*(torch.from_numpy(a).cuda() for a in (ob, os_, oc, cnt)), [(500, 500)] * n, TOPK)
        out.append(([{"image_id": iid} for iid, _, _, _ in group], batch))
    return out


def feed_lists(ev, calls):
    for iid, box, score, cls in calls:
        inst = Instances((500, 500), pred_boxes=Boxes(torch.from_numpy(np.asarray(box, np.float32).reshape(-1, 4)).cuda()),
                         scores=torch.from_numpy(np.asarray(score, np.float32)).cuda(),
                         pred_classes=torch.from_numpy(np.asarray(cls, np.int64)).cuda())
        ev.process([{"image_id": iid}], [{"instances": inst}])


def flat(res, prefix=""):
    out = []
    for k, v in res.items():
        out += flat(v, prefix + str(k) + "/") if isinstance(v, dict) else [(prefix + str(k), float(v))]
    return out


def same_results(a, b):
    fa, fb = flat(a), flat(b)
    assert [k for k, _ in fa] == [k for k, _ in fb]
    for (k, x), (_, y) in zip(fa, fb):
        assert x == y or (np.isnan(x) and np.isnan(y)), (k, x, y)


def with_empty_images(calls):
    """the same calls with two images without detections put in (count 0 blocks / empty Instances)"""
    empty = lambda iid: (iid, np.zeros((0, 4), np.float32), np.zeros((0,), np.float32), np.zeros((0,), np.int64))
    calls = list(calls)
    return calls[:2] + [empty(calls[0][0])] + calls[2:] + [empty(calls[-1][0])]


@pytest.mark.parametrize("case_fn", [VU.tie_free_case, VU.edge_case])
@pytest.mark.parametrize("year", [2007, 2012])
def test_voc_evaluator_padded_equals_lists(case_fn, year):
    case = case_fn()
    calls = with_empty_images(case["calls"])
    make = lambda: E.PascalVOCDetectionEvaluator(case["classes"], annotations=case["annos"], year=year, device="cuda")
    ev = make()
    feed_lists(ev, calls)
    want = ev.evaluate()
    ev = make()
    batches = padded_batches(calls)
    assert any(int(b.count.min()) == 0 for _, b in batches)
    for inputs, batch in batches:
        ev.process(inputs, batch)
    same_results(want, ev.evaluate())
    # mixed in one evaluation: lists, then padded blocks, then lists - processing order defines the tie order
    ev = make()
    a, b = len(calls) // 3, 2 * len(calls) // 3
    feed_lists(ev, calls[:a])
    for inputs, batch in padded_batches(calls[a:b], per_batch=4):
        ev.process(inputs, batch)
    feed_lists(ev, calls[b:])
    same_results(want, ev.evaluate())


def test_voc_host_path_accepts_a_detection_batch():
    case = VU.tie_free_case(n_img=12, per_img=9)
    make = lambda: E.PascalVOCDetectionEvaluator(case["classes"], annotations=case["annos"], year=2007)
    ev = make()
    VU.feed(ev, case, "cuda")
    want = ev.evaluate()
    ev = make()
    for inputs, batch in padded_batches(case["calls"]):
        ev.process(inputs, batch)
    same_results(want, ev.evaluate())


@pytest.mark.parametrize("name", CU.CASES)
def test_coco_evaluator_padded_equals_lists(name):
    c = CU.load_case(name)
    order = np.random.default_rng(1).permutation(c["img_ids"])
    calls = []
    for iid in order:
        sel = np.nonzero(c["dt_img"] == iid)[0]
        calls.append((int(iid), c["dt_box"][sel], c["dt_score"][sel], c["dt_cls"][sel]))
    calls = with_empty_images(calls)
    ev = E.COCOEvaluator(CU.annotations_of(c))
    feed_lists(ev, calls)
    want = ev.evaluate()
    want_eval = {k: ev.eval[k].copy() for k in ("precision", "recall", "scores")}
    ev = E.COCOEvaluator(CU.annotations_of(c))
    for inputs, batch in padded_batches(calls):
        ev.process(inputs, batch)
    same_results(want, ev.evaluate())
    for k, v in want_eval.items():
        assert np.array_equal(ev.eval[k], v), k
    ev = E.COCOEvaluator(CU.annotations_of(c))
    a = len(calls) // 2
    for inputs, batch in padded_batches(calls[:a], per_batch=5):
        ev.process(inputs, batch)
    feed_lists(ev, calls[a:])
    same_results(want, ev.evaluate())
    for k, v in want_eval.items():
        assert np.array_equal(ev.eval[k], v), k


# ---- the model surface ---------------------------------------------------------------------------------------------------

def same_instances(a, b):
    assert a.image_size == b.image_size
    assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores)
    assert a.pred_classes.dtype == b.pred_classes.dtype and torch.equal(a.pred_classes, b.pred_classes)


@pytest.fixture(scope="module")
def tiny():
    ocfg = G.MODEL_CASES["model_r50c4_tiny"]
    d = G.load("model_r50c4_tiny")
    cfg, model = G.drn_model(ocfg, int(d["seed"]), "cuda", 5, "fp32")
    model.eval()
    yield ocfg, d, cfg, model
    load_package().set_precision("fp32")


def test_plain_model_padded_equals_unpadded(tiny):
    ocfg, d, cfg, model = tiny
    batch = G.drn_inputs(G.batch_from(d), False)[:2]
    assert len(batch) == 2 and batch[0]["image"].shape != batch[1]["image"].shape
    for k, inp in enumerate(batch):  # output sizes that are not the input sizes, non-dyadic ratios
        inp["height"], inp["width"] = inp["height"] * 3 + 7 + k, inp["width"] * 2 - 5 - k
    want = model.inference(batch)
    got = model.inference(batch, padded=True)
    assert isinstance(got, DetectionBatch) and len(got) == 2 and got.topk == cfg.TEST.DETECTIONS_PER_IMAGE
    assert got.image_sizes == [(inp["height"], inp["width"]) for inp in batch]
    assert sum(len(w["instances"]) for w in want) > 0
    for w, g in zip(want, got.to_outputs()):
        same_instances(w["instances"], g["instances"])
    res, scores, boxes = model.inference(batch, do_postprocess=False)
    pres, pscores, pboxes = model.inference(batch, do_postprocess=False, padded=True)
    assert isinstance(pres, DetectionBatch) and pres.image_sizes == [r.image_size for r in res]
    for w, g in zip(res, pres.to_instances()):
        same_instances(w, g)
    for a, b in zip(scores + boxes, pscores + pboxes):
        assert torch.equal(a, b)
    assert model.roi_heads.padded_tail is None  # the opt-in does not stick
    same_instances(model.inference(batch)[0]["instances"], want[0]["instances"])


def tta_inputs(n):
    d = G.load("tta_r50c4_tiny")
    img = torch.from_numpy(d["image_u8"])
    H, W = img.shape[1:]
    out = []
    for i in range(n):
        prop = Instances((H, W))
        prop.proposal_boxes = Boxes(torch.from_numpy(d["proposal_boxes"][i::n].copy()))
        prop.objectness_logits = torch.from_numpy(d["objectness_logits"][i::n].copy())
        im = torch.flip(img, dims=[2]) if i % 2 else img
        out.append({"image": im.contiguous(), "proposals": prop, "height": H, "width": W, "image_id": "%06d" % (i + 1)})
    return out


def tta_cfg(cfg):
    cfg = cfg.clone()
    cfg.merge_from_list(["TEST.AUG.MIN_SIZES", "(48, 72)", "TEST.AUG.MAX_SIZE", "96", "TEST.AUG.FLIP", "True",
                         "DATASETS.PRECOMPUTED_PROPOSAL_TOPK_TEST", "40"])
    return cfg


def test_tta_padded_equals_unpadded(tiny):
    ocfg, d, cfg, model = tiny
    cfg = tta_cfg(cfg)
    inp = tta_inputs(1)[0]
    want = GeneralizedRCNNWithTTAAVG(cfg, model)([inp])[0]["instances"]
    got = GeneralizedRCNNWithTTAAVG(cfg, model, padded=True)([inp])
    assert isinstance(got, DetectionBatch) and len(got) == 1 and len(want) > 0
    same_instances(want, got.to_outputs()[0]["instances"])


def test_inference_on_dataset_padded_tta_equals_the_hand_written_loop(tiny):
    ocfg, d, cfg, model = tiny
    cfg = tta_cfg(cfg)
    inputs = tta_inputs(4)
    loader = [[x] for x in inputs[:2]] + [inputs[2:]]  # two single-image elements and one with two images
    names = ["c%d" % i for i in range(ocfg.num_classes)]
    H, W = inputs[0]["height"], inputs[0]["width"]
    annos = {x["image_id"]: [(names[(i + j) % len(names)], j % 2, [1 + 3 * i, 2 + j, W // 2 + 5 * j, H // 2 + 7 * i])
                             for j in range(3)] for i, x in enumerate(inputs)}
    plain = GeneralizedRCNNWithTTAAVG(cfg, model)
    ev = E.PascalVOCDetectionEvaluator(names, annotations=annos, year=2007, device="cuda")
    ev.reset()
    for el in loader:
        ev.process(el, plain(el))
    want = ev.evaluate()
    padded = GeneralizedRCNNWithTTAAVG(cfg, model, padded=True)
    padded.train()  # the loop puts the model into eval mode and restores the mode it found
    ev2 = E.PascalVOCDetectionEvaluator(names, annotations=annos, year=2007, device="cuda")
    got = E.inference_on_dataset(padded, loader, ev2)
    assert padded.training and ev2._padded and not ev2._boxes  # the blocks stayed padded until evaluate()
    padded.eval()
    same_results(want, got)
    same_results(want, E.inference_on_dataset(plain, loader, E.PascalVOCDetectionEvaluator(names, annotations=annos, year=2007,
                                                                                          device="cuda")))
