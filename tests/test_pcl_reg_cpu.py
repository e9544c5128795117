"""CPU side of the reg/pcl recipes (PCLROIHeads with a box-regression branch; include/drn_wsod.h "box regression of the PCL heads",
DESIGN 4.12): the restatement of tests/pcl_reg_util.py against the unmodified reference (tests/golden/model_pcl_reg_r50c4_tiny.npz),
the four recorded recipes, the host-side packing / capacity rule / refusals, and the boundary (header, signature table, exports)."""
import json
import os
import re
import subprocess
import types
import weakref

import numpy as np
import pytest
import torch
import yaml

import golden_util as G
import pcl_reg_util as PR
from __graft_entry__ import build, load_package

O = G.O
NAMES = ("drn_annot_box_reg", "drn_apply_deltas_mean")


@pytest.fixture(scope="module")
def pkg():
    return build()


@pytest.fixture(scope="module")
def gold():
    return G.load(PR.NAME)


def _replay(d):
    """the reference's recorded k-means / pick decisions (tests/test_oracle_golden.py does the same for model_pcl_r50c4_tiny)"""
    from oracle import pcl_oracle as PO

    km, picks = iter(d["pcl_km_log"].tolist()), iter(d["pcl_pick_log"].tolist())
    keep = PO.kmeans_top_threshold, PO._argmax_last
    PO.kmeans_top_threshold = lambda v: np.float32(next(km))
    PO._argmax_last = lambda x: int(next(picks))

    def undo():
        PO.kmeans_top_threshold, PO._argmax_last = keep

    return undo


# ------------------------------------------------------------------------------------------ the restatement against the reference
def test_fixture_conditions(gold):
    """what the generator asserted before it wrote: enough foreground and background, two classes, the duplicate box loses"""
    K, lab = 5, gold["labels"]
    fg = (lab >= 0) & (lab < K)
    assert fg.sum() >= 8 and (lab == K).sum() >= 8 and len(set(lab[fg].tolist())) >= 2
    gb, gc = gold["in0_gt_boxes"], gold["in0_gt_classes"]
    assert np.array_equal(gb[3], gb[0]) and gc[3] != gc[0] and (lab == gc[0]).sum() >= 1 and (lab == gc[3]).sum() == 0
    assert [str(k) for k in gold["loss_names"]] == ["loss_cls", "loss_cls_r0", "loss_cls_r1", "loss_cls_r2", "loss_cls_r3",
                                                    "loss_box_reg_r3"]
    assert all(("gradnone0.roi_heads.box_refinery_%d.bbox_pred.weight" % k) in gold for k in range(3))
    assert gold["wrong_rule_miss"].min() >= 0.25


def test_restatement_two_steps_equal_the_reference(gold):
    """losses of both steps and step 0's bbox_pred gradients within 1e-4 relative, the labels row for row"""
    cfg = PR.ocfg()
    seed = int(gold["seed"])
    p = O.seeded_params(O.param_shapes(cfg), seed)
    batch = G.batch_from(gold)
    opt = O.SGDState(cfg)
    undo = _replay(gold)
    try:
        for step in range(2):
            losses, grads, aux = PR.train_step(p, batch, cfg, opt, None, 5, return_aux=True)
            assert list(losses) == [str(k) for k in gold["loss_names"]]
            for k, v in losses.items():
                ref = float(gold["step%d_%s" % (step, k)])
                assert abs(v - ref) <= 1e-4 * max(1.0, abs(ref)), (step, k, v, ref)
            if step == 0:
                assert np.array_equal(aux["labels"].numpy(), gold["labels"])
                fg = (gold["labels"] >= 0) & (gold["labels"] < cfg.num_classes)
                assert np.array_equal(aux["gt_boxes"].numpy()[fg], gold["label_boxes"][fg])
                for n in ("weight", "bias"):
                    key = "roi_heads.box_refinery_3.bbox_pred." + n
                    g, rg = grads[key].numpy(), gold["grad0." + key]
                    assert np.abs(g - rg).max() <= 1e-4 * np.abs(rg).max(), key
    finally:
        undo()
    for n in O.trainable_names(p, cfg, 5):
        got, ref = p[n].reshape(-1)[:2048].numpy(), gold["after2.head." + n]
        assert np.abs(got - ref).max() <= 5e-3 * (np.abs(ref).max() + 1e-6), n


def test_restatement_inference_equals_the_reference(gold):
    """boxes from the mean over ALL four branches' deltas (the regressing branch's divided by 4), scores rotated; the two wrong
    rules miss the golden by more than a quarter pixel"""
    cfg = PR.ocfg()
    batch = G.batch_from(gold)
    R, K = batch[0]["proposal_boxes"].shape[0], cfg.num_classes
    p0 = PR.scale_bbox_pred(O.seeded_params(O.param_shapes(cfg), int(gold["seed"])), float(gold["bbox_scale"]), cfg)
    ref_boxes = torch.from_numpy(gold["all_boxes0"]).reshape(R, 4 * K)
    ref_scores = torch.from_numpy(gold["all_scores0"]).reshape(R, K + 1)
    res, sc, bx = PR.model_inference(p0, batch, cfg)
    assert torch.allclose(bx[0], ref_boxes, rtol=1e-4, atol=1e-3)
    assert torch.allclose(sc[0], ref_scores, rtol=1e-4, atol=1e-6)
    assert float((ref_boxes.view(R, K, 4) - batch[0]["proposal_boxes"][:, None, :]).abs().max()) >= 1.0
    rb, rs, rc, _ = res[0]
    n = min(len(rs), len(gold["det0_scores"]))
    assert abs(len(rs) - len(gold["det0_scores"])) <= 2 and n > 0
    assert torch.allclose(rs[:n], torch.from_numpy(gold["det0_scores"])[:n], rtol=1e-3, atol=1e-6)
    for rule in ("last", "all_layers"):
        _, _, wb = PR.model_inference(p0, batch, cfg, rule=rule)
        assert float((wb[0] - ref_boxes).abs().max()) >= 0.25, rule


def test_kernel_level_restatement_agrees_with_the_model_level_one(gold):
    """PR.annot_box_reg (what the GPU kernel tests run in fp64) on the reference's own labels and boxes: the fixture's labels,
    and for random deltas the loss O.oicr_box_reg_loss gives on the reference's gathered boxes"""
    import annot_metrics_util as AU

    K, W4 = 5, (10.0, 10.0, 5.0, 5.0)
    props = gold["in0_proposal_boxes"]
    gb, gc, cnt = AU.pack([gold["in0_gt_boxes"]], [gold["in0_gt_classes"]], 8)
    M = props.shape[0]
    lg = torch.from_numpy(np.random.RandomState(3).randn(M, 4 * K + 3)).double()
    r = PR.annot_box_reg(lg, [3], K, props, [0, M], gb, gc, cnt, (0.5,), (0, 1), W4)
    assert np.array_equal(r["labels"], gold["labels"])
    lab = torch.from_numpy(gold["labels"])
    want = O.oicr_box_reg_loss(lg[:, 3:], lab, torch.from_numpy(props).double(), torch.from_numpy(gold["label_boxes"]).double(), K,
                               PR._W(W4))
    assert abs(r["loss"][0] - float(want)) <= 1e-12 * abs(float(want))
    assert abs(r["terms"][0] / M - r["loss"][0]) <= 1e-12 * r["loss"][0]


# ------------------------------------------------------------------------------------------------------------ the recorded recipes
def _recorded_cfg(yaml_rel, tmp_path, opts=()):
    load_package()
    from drn_wsod_pytorch_amd.config import add_wsl_config, get_cfg

    with open(os.path.join(G.GOLDEN, "ref_yaml_cfgs_pcl_reg.json")) as f:
        rec = json.load(f)[yaml_rel]
    path = tmp_path / os.path.basename(yaml_rel)
    path.write_text(yaml.safe_dump(rec))
    cfg = get_cfg()
    add_wsl_config(cfg)
    cfg.merge_from_file(str(path))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.WEIGHTS", ""] + [str(o) for o in opts])
    return cfg


@pytest.mark.parametrize("yaml_rel", PR.REG_YAMLS)
def test_recorded_recipes_build_regressing_pcl_heads(pkg, yaml_rel, tmp_path):
    """each reg/pcl_*.yaml (its recorded merged settings; the neck narrowed to keep the CPU build small): PCLROIHeads, four
    branches, only box_refinery_3 regresses - its deltas are the only b-columns of the packed predictor"""
    from drn_wsod_pytorch_amd.modeling import build_model

    cfg = _recorded_cfg(yaml_rel, tmp_path, ["MODEL.ROI_BOX_HEAD.DAN_DIM", "[48, 64]"])
    assert cfg.MODEL.ROI_HEADS.NAME == "PCLROIHeads" and cfg.WSL.REFINE_NUM == 4
    assert list(cfg.WSL.REFINE_REG) == [False, False, False, True] and cfg.MODEL.ROI_HEADS.PROPOSAL_APPEND_GT is False
    assert list(cfg.MODEL.ROI_HEADS.IOU_THRESHOLDS) == [0.5] and list(cfg.MODEL.ROI_HEADS.IOU_LABELS) == [0, 1]
    heads = build_model(cfg).roi_heads
    assert type(heads).__name__ == "PCLROIHeads" and heads.refine_K == 4 and heads.refine_reg == [False, False, False, True]
    assert heads.regresses and heads.refine_mode == "pcl"
    cols, NH = heads._engine._layout()
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    assert [c[0] for c in cols] == ["cls", "det", "r0", "r1", "r2", "r3", "b3"] and NH == 2 * K + 4 * (K + 1) + 4 * K
    assert cols[-1][1] is heads.box_refinery[3].bbox_pred
    assert heads._annot_capacity() == 64


# --------------------------------------------------------------------------------------------- packing, capacity rule, refusals
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


def _pcl_heads(refine_reg=(False, False, False, True), append_gt=False, ring=None, owner=None):
    load_package()
    from drn_wsod_pytorch_amd.modeling import roi_heads as RH

    h = RH.PCLROIHeads.__new__(RH.PCLROIHeads)
    torch.nn.Module.__init__(h)
    object.__setattr__(h, "_engine", types.SimpleNamespace(captured_by=owner, metrics=ring))
    h.proposal_append_gt, h.refine_K, h.refine_reg = append_gt, len(refine_reg), list(refine_reg)
    return h, RH


def test_capacity_rule_and_refusals():
    from drn_wsod_pytorch_amd._cabi import DrnError

    ring = lambda gt: types.SimpleNamespace(annotated=True, max_gt=gt)
    h, RH = _pcl_heads()
    assert h.regresses and h._annot_capacity() == 64            # the default
    assert h.set_annotated_capacity(7) is h and h._annot_capacity() == 7
    # without a regressing branch nothing is packed unless the ring's block is on - as before
    h, _ = _pcl_heads(refine_reg=(False,) * 4)
    assert not h.regresses and h._annot_capacity() == 0
    h, _ = _pcl_heads(refine_reg=(False,) * 4, ring=ring(9))
    assert h._annot_capacity() == 9
    # both on: ONE block, the ring's max_gt is the capacity; a contradicting explicit capacity is refused loudly
    h, _ = _pcl_heads(ring=ring(9))
    assert h._annot_capacity() == 9
    h.set_annotated_capacity(9)
    with pytest.raises(DrnError, match="contradicts"):
        h.set_annotated_capacity(10)
    h, _ = _pcl_heads()
    h.set_annotated_capacity(10)
    h._engine.metrics = ring(9)
    with pytest.raises(DrnError, match="contradicts"):
        h._annot_capacity()
    # out of range
    h, _ = _pcl_heads()
    for bad in (0, 257):
        with pytest.raises(DrnError, match="annotated boxes per image are built"):
            h.set_annotated_capacity(bad)
    # PROPOSAL_APPEND_GT with a regressing branch
    h, _ = _pcl_heads(append_gt=True)
    with pytest.raises(DrnError, match="PROPOSAL_APPEND_GT"):
        h._annot_capacity()
    h, _ = _pcl_heads(refine_reg=(False,) * 4, append_gt=True)
    assert h._annot_capacity() == 0  # (no regression: the option is none of this feature's business)

    # after a graphed step was primed the capacity is frozen (the same value is no change)
    class Step:
        pass

    step = Step()
    h, _ = _pcl_heads(owner=weakref.ref(step))
    h.set_annotated_capacity(64)
    with pytest.raises(DrnError, match="after a graphed step was primed"):
        h.set_annotated_capacity(32)
    assert h._annot_capacity() == 64


def test_packing_and_too_many_boxes():
    from drn_wsod_pytorch_amd._cabi import DrnError

    h, RH = _pcl_heads()
    h.set_annotated_capacity(3)
    words = RH.pack_annotated(_targets([2, 3]), h._annot_capacity(), h._annot_setter())
    v = RH.annotated_views(words, 2, 3)
    assert v["ann_count"].tolist() == [2, 3] and v["ann_classes"].tolist() == [[0, 1, 0], [0, 1, 2]]
    assert v["ann_boxes"][1].reshape(-1).tolist() == list(range(12))
    with pytest.raises(DrnError, match=r"has 4 annotated boxes, PCLROIHeads.set_annotated_capacity\(3\) holds at most 3"):
        RH.pack_annotated(_targets([1, 4]), h._annot_capacity(), h._annot_setter())
    h._engine.metrics = types.SimpleNamespace(annotated=True, max_gt=3)
    with pytest.raises(DrnError, match=r"enable_metrics\(max_gt=3\)"):
        RH.pack_annotated(_targets([4]), h._annot_capacity(), h._annot_setter())


def test_graphed_label_buffer_holds_the_annotated_words():
    """_StaticInputs sizes its label block by the heads' capacity (graphed.py _annot_max_gt / _layout_labels)"""
    load_package()
    from drn_wsod_pytorch_amd import graphed

    h, RH = _pcl_heads()
    h.set_annotated_capacity(5)
    st = graphed._StaticInputs.__new__(graphed._StaticInputs)
    st.heads, st.engine = h, h._engine
    st.n_img, st.K, st.nper = 2, 4, [3, 2]
    st.model = types.SimpleNamespace(device="cpu")
    st.props = torch.zeros((5, 4))
    st._layout_labels()
    assert st._ann_gt == 5 and st._gt_block.numel() == 2 * 2 * 4 + 2 + RH.annotated_words(2, 5)
    assert st.gt["ann_boxes"].shape == (2, 5, 4) and st.gt["ann_count"].numel() == 2


def test_refusal_string_is_gone():
    src = open(os.path.join(G.ROOT, "drn-wsod-pytorch_amd", "modeling", "head_engine.py")).read()
    assert "PCL with box regression branches is not on the built path" not in src


# ------------------------------------------------------------------------------------------------------------------ the boundary
def test_header_signatures_and_exports_agree(pkg):
    hdr = open(os.path.join(G.ROOT, "include", "drn_wsod.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg._cabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines()}
    emap = open(os.path.join(G.ROOT, "drn-wsod-pytorch_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*drn_\*;", emap)  # the map exports the C ABI by its prefix
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        sig = pkg._cabi._SIGS[name]
        assert len(args) == len(sig), (name, len(args), len(sig))
        for a, c in zip(args, sig):
            if c == "p":
                assert "*" in a, (name, a)
            elif c == "i":
                assert re.match(r"int\s+\w+$", a), (name, a)
            elif c == "l":
                assert re.match(r"long\s+\w+$", a), (name, a)
            elif c == "f":
                assert re.match(r"float\s+\w+$", a), (name, a)
        assert name in exported and name in pkg._cabi.exported_symbols()
    for macro, val in (("DRN_BOXREG_MAX_HEADS", 8), ("DRN_BOXREG_MAX_IMAGES", 16)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, val), code)
    assert (pkg.ops.BOXREG_MAX_HEADS, pkg.ops.BOXREG_MAX_IMAGES) == (8, 16)
    mk = open(os.path.join(G.ROOT, "drn-wsod-pytorch_amd", "csrc", "Makefile")).read()
    assert "build/boxreg.o" in mk and "boxreg" not in mk.split("CONTRACT_OBJS =")[1].split("\n")[0]  # built with -ffp-contract=off
