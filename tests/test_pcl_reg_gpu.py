"""The reg/pcl recipes on the GPU (include/drn_wsod.h "box regression of the PCL heads").

Kernel level - drn_annot_box_reg and drn_apply_deltas_mean against the fp64 restatement of tests/pcl_reg_util.py on the same fp32
inputs (kernel_case: every coordinate a multiple of 1/4, so an fp32 target is within a few ulp of the fp64 one), against
drn_label_proposals (labels, bit for bit) and against the composition drn_label_proposals -> gather -> drn_box_reg_loss (the
gradient, bit for bit).  Model level - the reference-generated fixture model_pcl_reg_r50c4_tiny: two training steps, inference,
the graphed step, image batches.

u = 2^-24; an fp32 sum of n terms in any order is within gamma_n sum|x_i| of the exact one, gamma_n = n u / (1 - n u)."""
import numpy as np
import pytest
import torch

import golden_util as G
import pcl_reg_util as PR
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
O = G.O
DEV = "cuda"
U = 2.0 ** -24
NAN = float("nan")
W4 = (10.0, 10.0, 5.0, 5.0)


def gamma(n):
    return n * U / (1 - n * U)


@pytest.fixture(scope="module")
def drn():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    pkg = load_package()
    pkg._cabi.lib()  # raises if the HIP library is missing: no fallback
    import importlib

    return importlib.import_module("drn_wsod_pytorch_amd.ops")


def _relerr(a, b, floor=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + floor))


def _dev(c):
    return dict(logits=c["logits"].to(DEV), props=c["props"].to(DEV), img_off=torch.from_numpy(c["img_off"]).to(DEV),
                gt_boxes=torch.from_numpy(c["gt_boxes"]).to(DEV), gt_classes=torch.from_numpy(c["gt_classes"]).to(DEV),
                gt_count=torch.from_numpy(c["gt_count"]).to(DEV))


def _loss_bound(c, r, h, K):
    """|fp32 loss - fp64 loss| of head h.  Per foreground entry: the fp32 target differs from the fp64 one by eps = |t32 - t64| + 6 u |t|
    (the same IEEE operations as torch's fp32 get_deltas but for logf, <= 1 ulp either side, then the weight's multiply), the
    subtraction rounds once (u t); an image's sum of its n_i = 4 #fg terms (row sums, the 256-row tree and the ascending combine: n_i
    - 1 additions in SOME order) is within gamma_{n_i} of exact, the division by M_i rounds once; the mean over the images is an fp64
    sum rounded once (u |loss|).  The derivation of tests/test_heads_ref_gpu.py::test_box_reg_loss, per image."""
    M = c["props"].shape[0]
    fg = torch.from_numpy(r["fg"])
    img_off = c["img_off"].tolist()
    n_img = len(img_off) - 1
    t64 = r["target"]
    # the fp32 targets by torch's fp32 get_deltas on the same boxes
    img_of = np.zeros(M, dtype=np.int64)
    for i in range(n_img):
        img_of[img_off[i]: img_off[i + 1]] = i
    tb = torch.from_numpy(c["gt_boxes"][img_of, r["matched"]])
    t32 = torch.zeros((M, 4), dtype=torch.float64)
    if fg.any():
        t32[fg] = O.get_deltas(c["props"][fg], tb[fg], W4).double()
    eps = torch.where(fg[:, None], (t32 - t64).abs() + 6 * U * t64.abs(), torch.zeros_like(t64))
    t = r["absdiff"][h]
    bound = 0.0
    for i in range(n_img):
        a, b = img_off[i], img_off[i + 1]
        if b == a:
            continue
        n = max(4 * int(fg[a:b].sum()), 1)
        s = float((eps[a:b] * (1 + U) + U * t[a:b]).sum() + gamma(n) * (t[a:b] + 2 * eps[a:b]).sum())
        bound += (s / (b - a) + 2 * U * float(t[a:b].sum()) / (b - a)) / n_img
    return bound + U * abs(r["loss"][h])


@pytest.mark.parametrize("n_img", PR.KERNEL_NIMG)
@pytest.mark.parametrize("K", PR.KERNEL_K)
@pytest.mark.parametrize("M", PR.KERNEL_M)
def test_annot_box_reg_kernel(drn, M, K, n_img):
    """every (max_gt, threshold set, number of heads) of the issue's grid at this (M, K, n_img): labels and matched bit-equal to
    drn_label_proposals and equal to the restatement; the loss within the derived bound; the gradient exact - sign, 1 / M_i,
    1 / n_img, scale - on every checked foreground entry and exactly zero in every other column of the heads' 4K; nothing written
    outside the heads' windows; for one image the composition drn_label_proposals -> gather -> drn_box_reg_loss gives the same
    dlogits bit for bit."""
    scale = 0.37
    for max_gt in PR.KERNEL_MAX_GT:
        for n_heads in PR.KERNEL_HEADS:
            c = PR.kernel_case(M, K, n_img, max_gt, n_heads)
            d = _dev(c)
            ld_d = c["ld"] + 3
            for thr, lab in PR.KERNEL_THR:
                tag = (M, K, n_img, max_gt, n_heads, thr)
                r = PR.kernel_reference(c, K, thr, lab, W4, scale)
                dl = torch.full((M + 1, ld_d), NAN, device=DEV)
                max_rows = max(c["rows"])
                loss, labels, matched = drn.annot_box_reg(d["logits"], c["col0s"], K, d["props"], d["img_off"], n_img, d["gt_boxes"],
                                                          d["gt_classes"], d["gt_count"], thr, lab, W4, dlogits=dl,
                                                          loss_scale=scale, max_rows=max_rows, want_labels=True)
                lp = drn.label_proposals(d["props"], d["img_off"], n_img, d["gt_boxes"], d["gt_classes"], d["gt_count"], K, thr,
                                         lab, max_rows=max_rows)
                assert torch.equal(labels, lp["labels"]) and torch.equal(matched, lp["matched"]), tag
                assert np.array_equal(labels.cpu().numpy(), r["labels"]) and np.array_equal(matched.cpu().numpy(), r["matched"]), tag
                lc, dlc = loss.cpu(), dl.cpu()
                win = torch.zeros(dl.shape, dtype=torch.bool)
                for h, c0 in enumerate(c["col0s"]):
                    bound = _loss_bound(c, r, h, K)
                    print(tag, "head", h, "loss %.9g ref %.9g err %.3e bound %.3e" % (float(lc[h]), r["loss"][h],
                                                                                      abs(float(lc[h]) - r["loss"][h]), bound))
                    assert abs(float(lc[h]) - r["loss"][h]) <= bound, (tag, h, float(lc[h]), r["loss"][h], bound)
                    win[:M, c0: c0 + 4 * K] = True
                    got = dlc[:M, c0: c0 + 4 * K].reshape(M, K, 4)
                    fg = torch.from_numpy(r["fg"])
                    own = torch.zeros((M, K, 4), dtype=torch.bool)
                    cls = torch.from_numpy(np.where(r["fg"], r["labels"], 0))
                    own[torch.arange(M), cls] = fg[:, None]
                    assert bool((got[~own] == 0).all()), tag  # (NaN would fail too)
                    gf = got[torch.arange(M), cls]  # [M, 4]: the row's own class' four
                    want = r["sign"][h].float() * torch.from_numpy(r["grad_scale"])[:, None]
                    chk = r["checked"][h]
                    assert torch.equal(gf[chk], want[chk]), tag
                    gs = torch.from_numpy(r["grad_scale"])[:, None].expand(M, 4)
                    rest = fg[:, None] & ~chk
                    assert bool(((gf[rest] == gs[rest]) | (gf[rest] == -gs[rest]) | (gf[rest] == 0)).all()), tag
                    assert int(rest.sum()) <= 0.01 * max(r["n_fg_entries"], 1), tag
                rest = dlc[~win]
                assert bool(torch.isnan(rest).all()), tag  # nothing outside the heads' windows, no row past M
                if n_img == 1:
                    gathered = d["gt_boxes"][0][lp["matched"].long()].contiguous()
                    for h, c0 in enumerate(c["col0s"]):
                        dl2 = torch.full((M + 1, ld_d), NAN, device=DEV)
                        l2 = drn.box_reg_loss(d["logits"][:M], c0, K,  # (the wrapper takes M from the rows)
                                              lp["labels"], d["props"], gathered, W4, dlogits=dl2,
                                              loss_scale=scale)
                        assert torch.equal(dl2[:M, c0: c0 + 4 * K], dl[:M, c0: c0 + 4 * K]), tag
                        # the same terms in a sum of another order at most: gamma_n sum|terms| / M (+ the division's rounding)
                        n = max(r["n_fg_entries"], 1)
                        assert abs(float(l2.cpu()[0]) - float(lc[h])) <= 2 * gamma(n) * r["terms"][h] / M + 2 * U * abs(r["loss"][h]), tag


def test_annot_box_reg_shape_class(drn):
    """out of class: refused before any launch; empty M / n_img: nothing launched, nothing written"""
    cabi = load_package()._cabi
    c = PR.kernel_case(5, 4, 1, 1, 1)
    d = _dev(c)
    with pytest.raises(cabi.DrnError):
        drn.annot_box_reg(d["logits"], list(range(3, 3 + 9)), 4, d["props"], d["img_off"], 1, d["gt_boxes"], d["gt_classes"],
                          d["gt_count"])
    with pytest.raises(cabi.DrnError):  # a head's columns past the row
        drn.annot_box_reg(d["logits"], [c["ld"] - 3], 4, d["props"], d["img_off"], 1, d["gt_boxes"], d["gt_classes"], d["gt_count"])
    empty = torch.zeros((0, 4), device=DEV)
    loss = drn.annot_box_reg(d["logits"][:0], c["col0s"], 4, empty, torch.zeros(2, dtype=torch.int32, device=DEV), 1, d["gt_boxes"],
                             d["gt_classes"], d["gt_count"])
    assert float(loss.cpu()[0]) == 0.0


@pytest.mark.parametrize("M", [1, 257])
@pytest.mark.parametrize("heads,div", [(1, 1), (1, 4), (2, 3), (0, 4)])
def test_apply_deltas_mean(drn, M, heads, div):
    """bit-equal to drn_apply_deltas on the fp32 mean torch computes, ((+0 + d_0) + d_1) / div; no head: the zero-delta decode"""
    K = 5
    rs = np.random.RandomState(100 * M + 10 * heads + div)
    ld = 3 + max(heads, 1) * (4 * K + 1) + 2
    col0s = [3 + h * (4 * K + 1) for h in range(heads)]
    logits = torch.full((M, ld), NAN)
    for c0 in col0s:
        logits[:, c0: c0 + 4 * K] = torch.from_numpy(rs.standard_normal((M, 4 * K)).astype(np.float32) * 3)
    xy = rs.uniform(0, 600, (M, 2))
    boxes = torch.from_numpy(np.concatenate([xy, xy + np.exp(rs.uniform(0, 6, (M, 2)))], 1).astype(np.float32)).to(DEV)
    mean = PR.mean_deltas(logits, col0s, K, div)
    got = drn.apply_deltas_mean(logits.to(DEV), col0s, div, boxes, K, W4)
    want = drn.apply_deltas(mean.to(DEV), boxes, K, W4)
    assert got.shape == (M, 4 * K) and torch.equal(got, want)
    if heads == 0:
        assert torch.equal(got, drn.apply_deltas(None, boxes, K, W4))


# ------------------------------------------------------------------------------------------------------------------- model level
def _setup(bbox_scale=None):
    """tests/test_model_gpu.py::_setup for the fp32 reg/pcl fixture; bbox_scale: the inference record's parameters"""
    assert torch.cuda.is_available()
    load_package()
    ocfg = PR.ocfg()
    d = G.load(PR.NAME)
    cfg, model = G.drn_model(ocfg, int(d["seed"]), "cuda", 5, "fp32")
    if bbox_scale is not None:
        sd = model.state_dict()
        for k in range(ocfg.refine_num):
            n = "roi_heads.box_refinery_%d.bbox_pred.weight" % k
            sd[n] = sd[n] * bbox_scale
        model.load_state_dict(sd)
    model.roi_heads.box_head.dropout_p = 0.0  # the fixture was generated with dropout patched to identity
    return ocfg, d, cfg, model


def test_two_training_steps():
    """step 0's loss_box_reg_r3 and bbox_pred gradients against the REFERENCE golden within 1e-4 (they do not depend on the
    clustering); every other loss, every gradient and the updated parameters against the restatement with the tolerances of
    tests/test_model_gpu.py::test_pcl_heads_two_steps_vs_oracle_fp32 (1e-4 step 0, 2e-2 step 1; 2e-3 gradients; 5e-3 parameters)"""
    from drn_wsod_pytorch_amd.engine import build_optimizer

    ocfg, d, cfg, model = _setup()
    heads = model.roi_heads
    assert type(heads).__name__ == "PCLROIHeads" and heads.refine_reg == [False, False, False, True]
    batch = G.batch_from(d)
    p = O.seeded_params(O.param_shapes(ocfg), int(d["seed"]))
    opt_o = O.SGDState(ocfg)
    model.train()
    opt = build_optimizer(cfg, model)
    for step in range(2):
        ref_losses, ref_grads = PR.train_step(p, batch, ocfg, opt_o)
        opt.zero_grad()
        losses = model(G.drn_inputs(batch))
        sum(losses.values()).backward()
        got = {k: float(v.detach()) for k, v in losses.items()}
        assert list(got) == [str(k) for k in d["loss_names"]] == list(ref_losses)
        for k in got:
            tol = 1e-4 if step == 0 else 2e-2
            print(step, k, got[k], ref_losses[k])
            assert abs(got[k] - float(ref_losses[k])) <= tol * max(abs(float(ref_losses[k])), 1e-3), (step, k, got[k])
        if step == 0:
            ref = float(d["step0_loss_box_reg_r3"])
            assert abs(got["loss_box_reg_r3"] - ref) <= 1e-4 * abs(ref), (got["loss_box_reg_r3"], ref)
            sd = dict(model.named_parameters())
            for n in ("weight", "bias"):
                key = "roi_heads.box_refinery_3.bbox_pred." + n
                err = _relerr(sd[key].grad.detach().cpu().numpy(), d["grad0." + key], floor=0.0)
                print(key, "relerr vs the reference %.3e" % err)
                assert err <= 1e-4, (key, err)
            for k in range(3):  # unused layers: no gradient, as in the reference
                assert sd["roi_heads.box_refinery_%d.bbox_pred.weight" % k].grad is None
            for n_, prm in model.named_parameters():
                if prm.requires_grad and n_ in ref_grads:
                    rg, g = ref_grads[n_].numpy(), prm.grad.detach().cpu().numpy()
                    if np.abs(rg).max() < 1e-6:
                        assert np.abs(g).max() < 1e-5, n_
                    else:
                        assert _relerr(g, rg) < 2e-3, n_
        opt.step()
    torch.cuda.synchronize()
    names = set(O.trainable_names(p, ocfg, 5))
    assert "roi_heads.box_refinery_3.bbox_pred.weight" in names and "roi_heads.box_refinery_2.bbox_pred.weight" not in names
    for n_, prm in model.named_parameters():
        if prm.requires_grad and n_ in names:
            assert _relerr(prm.detach().cpu().numpy(), p[n_].numpy()) < 5e-3, n_


def test_inference_against_the_reference():
    """the golden's all_scores / all_boxes / detections at the seeded parameters with every bbox_pred weight scaled (boxes move by
    more than 13 px), within the bounds tests/test_model_gpu.py applies to model_r50c4_reg_tiny; OICR's rule (last branch
    undivided) would miss by 40 px"""
    ocfg, d, cfg, model = _setup(float(d_scale()))
    batch = G.batch_from(d)
    R, K = len(batch[0]["proposal_boxes"]), ocfg.num_classes
    model.eval()
    res, all_scores, all_boxes = model.inference(G.drn_inputs(batch, False), do_postprocess=False)
    ref_scores = torch.from_numpy(d["all_scores0"]).reshape(R, K + 1)
    ref_boxes = torch.from_numpy(d["all_boxes0"]).reshape(R, 4 * K)
    assert _relerr(all_scores[0][0].cpu().numpy(), ref_scores.numpy()) < 1e-4
    assert torch.allclose(all_boxes[0][0].cpu(), ref_boxes, rtol=1e-4, atol=1e-3)
    rs, rc = torch.from_numpy(d["det0_scores"]), torch.from_numpy(d["det0_classes"])
    n = min(len(rs), len(res[0]))
    gs = res[0].scores.cpu()
    assert abs(len(rs) - len(res[0])) <= 2 and n > 0
    assert torch.allclose(gs[:n], rs[:n], rtol=1e-3, atol=1e-6)
    gaps = (rs[:-1] - rs[1:]).abs() if len(rs) > 1 else torch.zeros(0)
    stable = torch.ones(n, dtype=torch.bool)
    if n > 1:
        small = gaps[: n - 1] < 1e-5 * rs[: n - 1].abs()
        stable[:-1] &= ~small
        stable[1:] &= ~small
    assert torch.equal(res[0].pred_classes.cpu()[stable], rc[:n][stable])
    # the TTA path (scores_only) returns the same scores and boxes without detections
    model.roi_heads.scores_only = True
    try:
        _, s2, b2 = model.inference(G.drn_inputs(batch, False), do_postprocess=False)
    finally:
        model.roi_heads.scores_only = False
    assert torch.equal(s2[0], all_scores[0]) and torch.equal(b2[0], all_boxes[0])


def d_scale():
    return G.load(PR.NAME)["bbox_scale"]


def _run_steps(mode, n=3, capacity=None, annotated_ring=False):
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer

    ocfg, d, cfg, model = _setup()
    batch = G.drn_inputs(G.batch_from(d))
    model.train()
    if capacity is not None:
        model.roi_heads.set_annotated_capacity(capacity)
    if annotated_ring:
        model.roi_heads.enable_metrics(slots=8, annotated=True, max_gt=capacity or 64)
    opt = build_optimizer(cfg, model)
    out = []
    if mode == "graph":
        stepper = GraphedTrainStep(model, opt, batch)
        for _ in range(n):
            out.append({k: float(v.detach()) for k, v in stepper.step(batch, batch).items()})
    else:
        stepper = None
        for _ in range(n):
            opt.zero_grad()
            losses = model(batch)
            sum(losses.values()).backward()
            opt.step()
            out.append({k: float(v.detach()) for k, v in losses.items()})
    torch.cuda.synchronize()
    return out, model, stepper


def test_graphed_step_equals_eager_bit_for_bit():
    """three steps: every loss of GraphedTrainStep equals the eager step's bit for bit; the captured label buffer holds the
    annotated words; changing the capacity after priming is refused"""
    from drn_wsod_pytorch_amd._cabi import DrnError

    eager, _, _ = _run_steps("eager")
    graph, model, stepper = _run_steps("graph")
    for x, y in zip(eager, graph):
        assert list(x) == list(y) and "loss_box_reg_r3" in x
        for k in x:
            assert x[k] == y[k], (k, x[k], y[k])
    assert stepper._ann_gt == 64 and "ann_boxes" in stepper.gt
    with pytest.raises(DrnError, match="primed"):
        model.roi_heads.set_annotated_capacity(32)
    # the ring's annotated block and the regression share ONE block: same losses, and the ring's capacity is the block's
    both, model, stepper = _run_steps("graph", capacity=8, annotated_ring=True)
    assert stepper._ann_gt == 8
    for x, y in zip(eager, both):
        for k in x:
            assert x[k] == y[k], (k, x[k], y[k])


def test_too_many_annotated_boxes_refused_on_the_host():
    from drn_wsod_pytorch_amd._cabi import DrnError

    ocfg, d, cfg, model = _setup()
    model.train()
    model.roi_heads.set_annotated_capacity(3)  # the fixture's image has four annotated boxes
    with pytest.raises(DrnError, match="has 4 annotated boxes"):
        model(G.drn_inputs(G.batch_from(d)))


def test_image_batches_mean_over_images():
    """enable_image_batches: a 2-image step's loss_box_reg_r3 = fp32(((double)l_0 + (double)l_1) / 2) of the two single-image
    losses, and its bbox_pred gradients = the mean of theirs to fp32 rounding.  Bound: dW[j, c] = sum_r dS[r, j] H2[r, c] with
    |dS[r, j]| <= 1 / (2 M_i(r)); the batch GEMM and the two single ones sum the same products in other orders, each within
    gamma_M of B[c] = sum_r |H2[r, c]| / (2 M_i(r)), and the halving is exact: |batch - mean| <= 2 gamma_{M + 2} B[c] (bias: H2 = 1)."""
    ocfg, d, cfg, model = _setup()
    first = G.batch_from(d)[0]
    second = dict(first, proposal_boxes=first["proposal_boxes"][3:40].clone(),
                  objectness_logits=first["objectness_logits"][3:40].clone(), gt_boxes=first["gt_boxes"][:2].clone(),
                  gt_classes=first["gt_classes"][:2].clone())
    a, b = G.drn_inputs([first]), G.drn_inputs([second])
    model.train()
    keys = ["roi_heads.box_refinery_3.bbox_pred.weight", "roi_heads.box_refinery_3.bbox_pred.bias"]
    sd = dict(model.named_parameters())
    singles = []
    for x in (a, b):
        model.zero_grad()
        losses = model(x)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        singles.append((np.float32(losses["loss_box_reg_r3"].detach().cpu().numpy()), {k: sd[k].grad.detach().clone() for k in keys}))
    assert singles[0][0] > 0 and singles[1][0] > 0  # both images have foreground rows
    model.roi_heads.enable_image_batches(True)
    model.zero_grad()
    losses = model(a + b)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    got = np.float32(losses["loss_box_reg_r3"].detach().cpu().numpy())
    want = np.float32((np.float64(singles[0][0]) + np.float64(singles[1][0])) / np.float64(2.0))
    print("batch %.9g singles %.9g %.9g defined mean %.9g" % (got, singles[0][0], singles[1][0], want))
    assert got == want
    st = model.roi_heads._last_state
    M0, M1 = len(first["proposal_boxes"]), len(second["proposal_boxes"])
    M = M0 + M1
    H2 = st["w"]["H2"][:M, : sd[keys[0]].shape[1]].float().abs().cpu().double()
    wrow = torch.cat([torch.full((M0,), 1.0 / (2 * M0)), torch.full((M1,), 1.0 / (2 * M1))]).double()
    B = (H2 * wrow[:, None]).sum(0)
    for k in keys:
        mean = ((singles[0][1][k].double() + singles[1][1][k].double()) / 2.0).cpu()
        g = sd[k].grad.detach().cpu().double()
        bound = 2 * gamma(M + 2) * (B[None, :] if k.endswith("weight") else wrow.sum()) + 1e-12
        err = (g - mean).abs()
        print(k, "max err %.3e, max bound %.3e, max |g| %.3e" % (float(err.max()), float(torch.as_tensor(bound).max()),
                                                                  float(g.abs().max())))
        assert bool((err <= bound).all()), k
        assert float(g.abs().max()) > 0


RECIPE_OPTS = ["MODEL.ROI_BOX_HEAD.DAN_DIM", "[48, 64]"]


@pytest.mark.parametrize("yaml_rel", PR.REG_YAMLS)
def test_recorded_recipes_train_and_infer(yaml_rel, tmp_path):
    """a model built from each recorded reg/pcl recipe (full trunk, the neck narrowed to keep it quick) trains a step eagerly and
    under GraphedTrainStep - same losses - and runs inference with boxes that left the proposals"""
    import json
    import os

    import yaml

    from drn_wsod_pytorch_amd.config import add_wsl_config, get_cfg
    from drn_wsod_pytorch_amd.engine import GraphedTrainStep, build_optimizer
    from drn_wsod_pytorch_amd.modeling import build_model

    pkg = load_package()
    pkg.set_precision("fp32")
    with open(os.path.join(G.GOLDEN, "ref_yaml_cfgs_pcl_reg.json")) as f:
        rec = json.load(f)[yaml_rel]
    path = tmp_path / os.path.basename(yaml_rel)
    path.write_text(yaml.safe_dump(rec))
    d = G.load(PR.NAME)
    first = G.batch_from(d)[0]
    K = 20
    first = dict(first, gt_classes=first["gt_classes"] + 7)  # any of the recipe's 20 classes
    out = []
    for mode in ("eager", "graph"):
        cfg = get_cfg()
        add_wsl_config(cfg)
        cfg.merge_from_file(str(path))
        cfg.merge_from_list(["MODEL.DEVICE", "cuda", "MODEL.WEIGHTS", ""] + RECIPE_OPTS)
        assert cfg.MODEL.ROI_HEADS.NUM_CLASSES == K
        torch.manual_seed(5)
        model = build_model(cfg)
        model.roi_heads.box_head.dropout_p = 0.0
        with torch.no_grad():
            model.roi_heads.box_refinery[3].bbox_pred.weight.mul_(50.0)
        batch = G.drn_inputs([first])
        model.train()
        opt = build_optimizer(cfg, model)
        if mode == "graph":
            losses = GraphedTrainStep(model, opt, batch).step(batch, batch)
        else:
            opt.zero_grad()
            losses = model(batch)
            sum(losses.values()).backward()
            opt.step()
        got = {k: float(v.detach()) for k, v in losses.items()}
        assert "loss_box_reg_r3" in got and all(np.isfinite(v) for v in got.values()), got
        out.append(got)
        if mode == "eager":
            model.eval()
            res, sc, bx = model.inference(G.drn_inputs([first], False), do_postprocess=False)
            props = first["proposal_boxes"]
            assert bx[0][0].shape == (len(props), 4 * K) and sc[0][0].shape == (len(props), K + 1)
            assert bool(torch.isfinite(bx[0][0]).all())
            assert float((bx[0][0].cpu().view(len(props), K, 4) - props[:, None, :]).abs().max()) > 0
    for k in out[0]:  # (the tolerance of tests/test_model_gpu.py::test_pcl_heads_reject_batches_and_graph_capture_ok)
        assert abs(out[0][k] - out[1][k]) <= 1e-6 * max(1.0, abs(out[0][k])), (k, out[0][k], out[1][k])
