"""CPU side of the annotated-box block of the per-step metrics (include/drn_wsod.h "per-step metrics"): the restatement
of tests/annot_metrics_util.py against the unmodified reference (tests/golden/metrics_annot_r50c4_tiny.npz), decode_record with and
without the block, the host-side refusals, and the boundary (header, signature table, exported symbols)."""
import os
import re
import subprocess
import types
import weakref

import numpy as np
import pytest
import torch

import annot_metrics_util as AU
import golden_util as G
import metrics_util as MU
from __graft_entry__ import build, load_package

NAMES = ("drn_label_proposals", "drn_mil_metrics", "drn_metrics_record_annot")
W = 72


@pytest.fixture(scope="module")
def pkg():
    return build()


def _mods():
    load_package()
    import importlib

    return (importlib.import_module("drn_wsod_pytorch_amd.metrics"), importlib.import_module("drn_wsod_pytorch_amd.ops"),
            importlib.import_module("drn_wsod_pytorch_amd.modeling.roi_heads"))


# ------------------------------------------------------------------------------------------ the restatement against the reference
def test_restatement_equals_the_reference_fixture():
    """the fixture's own inputs through the restatement: the labels equal the reference's row for row, and with the reference's MIL
    scores every stored scalar comes out (ratios of small integers: 1e-12), present exactly where the reference logged it"""
    gold = G.load("metrics_annot_r50c4_tiny")
    assert float(gold["min_margin"]) >= 1e-3
    assert [str(k) for k in gold["names"]] == list(AU.NAMES)
    batch = G.batch_from(gold)
    n_img, K = len(batch), int(gold["num_classes"])
    props = np.concatenate([b["proposal_boxes"].numpy() for b in batch])
    off = np.cumsum([0] + [len(b["proposal_boxes"]) for b in batch])
    gb, gc, cnt = AU.pack([b["gt_boxes"].numpy() for b in batch], [b["gt_classes"].numpy() for b in batch], 8)
    thr, lab = [float(t) for t in gold["iou_thresholds"]], [int(v) for v in gold["iou_labels"]]
    labels, matched, counts = AU.label_proposals(props, off, gb, gc, cnt, K, thr, lab)
    M = props.shape[0]
    assert counts.sum() == M and counts[2] > 0  # the annotated boxes are proposals: each matches itself
    for s in range(int(gold["steps"])):
        assert np.array_equal(labels, gold["labels%d" % s]), s
        want = AU.scalars(counts, AU.mil_counts(gold["mil_scores%d" % s], labels, M), M, n_img)
        for k, v, p in zip(AU.NAMES, gold["step%d" % s], gold["present%d" % s]):
            assert (k in want) == bool(p), (k, s)
            if p:
                assert abs(want[k] - float(v)) <= 1e-12, (k, s, want[k], float(v))


def test_restatement_on_hand_made_cases():
    """IoU exactly at a threshold, identical boxes (the lower index wins), zero-area boxes, no annotated box"""
    props = np.array([[0, 0, 2, 2], [0, 0, 2, 1], [5, 5, 5, 9], [0, 0, 10, 1], [20, 20, 30, 30]], dtype=np.float32)
    gb, gc, cnt = AU.pack([[[0, 0, 2, 1], [0, 0, 2, 1], [0, 0, 1, 1]]], [[3, 1, 2]], 4)
    iou = AU.pairwise_iou(gb[0, :3], props).numpy()
    assert iou[0, 0] == np.float32(0.5) and iou[0, 1] == 1.0 and iou[0, 2] == 0.0 and iou[2, 3] == np.float32(0.1)
    labels, matched, counts = AU.label_proposals(props, [0, 5], gb, gc, cnt, 7, (0.5,), (0, 1))
    assert labels.tolist() == [3, 3, 7, 7, 7] and matched.tolist() == [0, 0, 0, 0, 0]  # 0.5 >= 0.5: foreground; ties: index 0
    labels, matched, counts = AU.label_proposals(props, [0, 5], gb, gc, cnt, 7, (0.1, 0.5), (-1, 0, 1))
    assert labels.tolist() == [3, 3, -1, 7, -1] and counts.tolist() == [2, 1, 2]  # 0.1 <= 0.2 < 0.5 is background, < 0.1 ignored
    gb0, gc0, cnt0 = AU.pack([[]], [[]], 4)
    labels, matched, counts = AU.label_proposals(props, [0, 5], gb0, gc0, cnt0, 7, (0.1, 0.5), (-1, 0, 1))
    assert labels.tolist() == [7] * 5 and matched.tolist() == [0] * 5 and counts.tolist() == [0, 5, 0]
    # the MIL statistics' background is the LAST column: label K - 1 is no foreground there, label K never accurate
    sc = np.array([[.1, .9, .0], [.9, .1, .0], [.0, .1, .9], [.2, .2, .1], [.1, .1, .8]], dtype=np.float32)
    assert AU.mil_counts(sc, [1, 1, 2, 0, 0], 5).tolist() == [3, 2, 1, 4]
    assert AU.mil_counts(sc[:, :1], [0, 0, 1, -1, 0], 5).tolist() == [3, 0, 0, 0]  # one column: no foreground at all


# --------------------------------------------------------------------------------------------------------------- decode_record
def _record(idx, losses, counts=(), M=0, block=None):
    r = [0] * W
    r[0], r[1], r[2], r[3] = idx, len(losses), len(counts), M
    for i, v in enumerate(losses):
        r[4 + i] = MU.f32_bits(v)
    for k, row in enumerate(counts):
        r[20 + 6 * k: 26 + 6 * k] = list(row)
    if block is not None:  # n_ig, n_bg, n_fg, n_acc, n_fg_acc, n_fneg, mil_fg
        r[62:68], r[68], r[70] = list(block[:6]), block[6], 1
    r[W - 1] = idx
    return r


def test_decode_record_without_and_with_the_block():
    M_, ops, _ = _mods()
    assert (ops.METRICS_ANNOT_ROW, ops.METRICS_ANNOT_WORD_FG, ops.METRICS_ANNOT_WORD_FLAG, ops.METRICS_ANNOT_FLAG) == (7, 68, 70, 1)
    assert ops.METRICS_RECORD_WORDS == W
    names = ["loss_cls", "loss_cls_r0"]
    counts = [(3, 30, 15, 20, 9, 4), (8, 40, 0, 40, 0, 0)]
    plain = M_.decode_record(_record(5, [0.25, 1.5], counts, M=48), names, 2)
    assert plain == dict(MU.scalars(counts, 48, 2), loss_cls=0.25, loss_cls_r0=1.5, total_loss=1.75)  # exactly as before
    assert not any(k in plain for k in AU.NAMES)
    # words in the block's place without the flag word are not a block
    r = _record(5, [0.25, 1.5], counts, M=48)
    r[62:68] = [1, 2, 3, 4, 5, 6]
    assert M_.decode_record(r, names, 2) == plain
    block = (4, 40, 4, 7, 2, 1, 3)
    got = M_.decode_record(_record(5, [0.25, 1.5], counts, M=48, block=block), names, 2)
    want = AU.scalars(block[:3], (7, 2, 1, 3), 48, 2)
    assert len(want) == 6 and {k: got[k] for k in AU.NAMES} == want
    assert {k: v for k, v in got.items() if k not in AU.NAMES} == plain
    assert got["roi_head/num_fg_samples"] == 2.0 and got["fast_rcnn/fg_cls_accuracy"] == 2 / 3 and got["fast_rcnn/cls_accuracy"] == 7 / 48
    # the omission rules: no MIL foreground -> no fg ratios; M == 0 -> no accuracy at all
    got = M_.decode_record(_record(6, [0.5, 0.5], counts, M=48, block=(0, 44, 4, 7, 0, 0, 0)), names, 2)
    assert "fast_rcnn/cls_accuracy" in got and "fast_rcnn/fg_cls_accuracy" not in got and "fast_rcnn/false_negative" not in got
    got = M_.decode_record(_record(7, [0.5, 0.5], [(0,) * 6] * 2, M=0, block=(0,) * 7), names, 2)
    assert not any(k.startswith("fast_rcnn/") for k in got) and got["roi_head/num_bg_samples"] == 0.0


# ------------------------------------------------------------------------------------------------------------------- refusals
def _targets(n_boxes):
    load_package()
    from drn_wsod_pytorch_amd.structures import Boxes, Instances

    out = []
    for n in n_boxes:
        t = Instances((64, 64))
        t.gt_boxes = Boxes(torch.arange(4 * n, dtype=torch.float32).view(n, 4))
        t.gt_classes = torch.arange(n) % 3
        out.append(t)
    return out


def test_pack_annotated_and_max_gt_exceeded():
    _, _, RH = _mods()
    from drn_wsod_pytorch_amd._cabi import DrnError

    words = RH.pack_annotated(_targets([2, 0, 3]), 3)
    assert words.dtype == torch.int32 and words.numel() == RH.annotated_words(3, 3) == 3 * 3 * 5 + 3
    v = RH.annotated_views(words, 3, 3)
    assert v["ann_count"].tolist() == [2, 0, 3] and v["ann_classes"].tolist() == [[0, 1, 0], [0, 0, 0], [0, 1, 2]]
    assert v["ann_boxes"][2].reshape(-1).tolist() == list(range(12)) and not v["ann_boxes"][1].any()
    with pytest.raises(DrnError, match="has 4 annotated boxes"):
        RH.pack_annotated(_targets([1, 4]), 3)


def _stub(append_gt=False, refine_K=3, owner=None):
    eng = types.SimpleNamespace(captured_by=owner, arena_w=torch.zeros(1), ensure=lambda dev: None, metrics=None)
    return types.SimpleNamespace(_engine=eng, parameters=lambda: iter([torch.zeros(1)]), proposal_append_gt=append_gt,
                                 refine_K=refine_K, refine_mode="oicr")


def test_enable_metrics_refusals():
    _, ops, RH = _mods()
    from drn_wsod_pytorch_amd._cabi import DrnError

    heads = _stub()
    ring = RH.OICRROIHeads.enable_metrics(heads, slots=5, annotated=True, max_gt=9)
    assert heads._engine.metrics is ring and ring.annotated and ring.max_gt == 9
    ring = RH.OICRROIHeads.enable_metrics(heads, slots=5)
    assert not ring.annotated
    heads = _stub(append_gt=True)
    with pytest.raises(DrnError, match="PROPOSAL_APPEND_GT"):
        RH.OICRROIHeads.enable_metrics(heads, annotated=True)
    assert heads._engine.metrics is None
    assert RH.OICRROIHeads.enable_metrics(heads) is not None  # the option off: as before
    with pytest.raises(DrnError, match="last head slot"):
        RH.OICRROIHeads.enable_metrics(_stub(refine_K=8), annotated=True)
    with pytest.raises(DrnError, match="max_gt"):
        RH.OICRROIHeads.enable_metrics(_stub(), annotated=True, max_gt=ops.LABEL_MAX_GT + 1)

    class Step:
        pass

    step = Step()
    heads = _stub(owner=weakref.ref(step))
    with pytest.raises(DrnError, match="after a graphed step was primed"):
        RH.OICRROIHeads.enable_metrics(heads, annotated=True)
    assert heads._engine.metrics is None


def test_ring_refuses_a_block_beside_eight_branches():
    M_, ops, _ = _mods()
    from drn_wsod_pytorch_amd._cabi import DrnError

    ring = M_.MetricsRing(4, "cpu", annotated=True, max_gt=4)
    with pytest.raises(DrnError):
        ops.metrics_record([torch.zeros(1)], ring.counts, 8, 1, ring.ring, ring.state, annot=True)


# ------------------------------------------------------------------------------------------------------------------ the boundary
def test_header_signatures_and_exports_agree(pkg):
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg._cabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines()}
    emap = open(os.path.join(G.ROOT, "drn-wsod-pytorch_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*drn_\*;", emap)  # the map exports the C ABI by its prefix: every drn_ symbol, nothing else
    kind = {"p": "*", "i": "int", "l": "long"}
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S)
        assert m, "include/drn_wsod.h does not declare %s" % name
        args = [a.strip() for a in m.group(1).split(",")]
        sig = pkg._cabi._SIGS[name]
        assert len(args) == len(sig), (name, args, sig)
        for a, c in zip(args, sig):
            if c == "p":
                assert "*" in a, (name, a)
            else:
                assert "*" not in a and re.match(r"(unsigned\s+)?%s\b" % kind[c], a), (name, a, c)
        assert name in exported and name in pkg._cabi.exported_symbols()
        assert hasattr(pkg._cabi.lib(), name)
    _, ops, _ = _mods()
    for macro, val in (("LABEL_MAX_GT", ops.LABEL_MAX_GT), ("METRICS_ANNOT_ROW", ops.METRICS_ANNOT_ROW),
                       ("METRICS_ANNOT_WORD_FG", ops.METRICS_ANNOT_WORD_FG), ("METRICS_ANNOT_WORD_FLAG", ops.METRICS_ANNOT_WORD_FLAG)):
        assert re.search(r"#define DRN_%s %d\b" % (macro, val), hdr), macro
    assert re.search(r"#define DRN_METRICS_ANNOT_FLAG %du\b" % ops.METRICS_ANNOT_FLAG, hdr)
